"""tvm_sponge_sample_indices (csrc/proof_tail.hip: k_sponge_tail without items) against ProofStream.sample_indices continued from the
same sponge state: the same indices and the same state afterwards, including states that make the sampler skip elements."""
import numpy as np
import pytest

from triton_vm_amd import field, proof_tail
from triton_vm_amd.prover import ProofStream

P_MINUS_1 = field.to_mont(field.P - 1)   # the Montgomery word of the one element Tip5::sample_indices skips


def _host(ctx, state, upper_bound, n):
    ps = ProofStream(ctx.lib)
    ps.state[:] = state
    return ps.sample_indices(upper_bound, n), ps.state.copy()


def _check(ctx, state, upper_bound, n):
    want, want_state = _host(ctx, state, upper_bound, n)
    got, got_state = proof_tail.sponge_sample_indices(ctx, state, upper_bound, n)
    assert got.tolist() == want and (got_state == want_state).all(), (upper_bound, n)
    return got


@pytest.mark.parametrize("upper_bound", [2, 1 << 10, 1 << 23, 1 << 32])
def test_indices_and_state_equal_the_host_sampler(ctx, orc, upper_bound):
    rng = np.random.default_rng(upper_bound % 1009)
    for n in (1, 10, 11, 173, 320):
        got = _check(ctx, orc.random_elements(rng, 16), upper_bound, n)
        assert len(got) == n and int(got.max()) < upper_bound
    assert len(set(_check(ctx, orc.random_elements(rng, 16), upper_bound, 320).tolist())) > (1 if upper_bound == 2 else 100)


def test_elements_equal_to_p_minus_one_are_skipped(ctx, orc):
    rng = np.random.default_rng(41)
    assert field.from_mont(P_MINUS_1) == field.P - 1
    for positions in [(0,), (4,), (9,), (0, 4, 9), tuple(range(10))]:
        state = orc.random_elements(rng, 16)
        state[list(positions)] = P_MINUS_1
        for n in (1, 10, 11, 173):   # the first squeeze runs short by len(positions): n = 10 needs a second one, n = 1 may too
            _check(ctx, state, 1 << 23, n)
    # all ten rate words: the first squeeze yields nothing, and the indices are those of the state one permutation later
    state = orc.random_elements(rng, 16)
    state[:10] = P_MINUS_1
    later = state.copy()
    ctx.lib.tvm_host_tip5_permutation(later.ctypes.data)
    assert proof_tail.sponge_sample_indices(ctx, state, 1 << 10, 7)[0].tolist() == _host(ctx, later, 1 << 10, 7)[0]


def test_no_index_and_bad_arguments(ctx, orc):
    from triton_vm_amd.capi import TritonHipError

    state = orc.random_elements(np.random.default_rng(42), 16)
    got, after = proof_tail.sponge_sample_indices(ctx, state, 16, 0)
    assert len(got) == 0 and (after == state).all()   # nothing squeezed, nothing permuted
    for upper_bound in (0, 12, 1 << 33):
        with pytest.raises(TritonHipError):
            proof_tail.sponge_sample_indices(ctx, state, upper_bound, 4)
