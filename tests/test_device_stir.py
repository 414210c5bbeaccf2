"""The rounds of a STIR proof in one device call (csrc/stir_rounds.hip: tvm_stir_prove_rounds; the C++ host under
TVMH_OPTION_DEVICE_STIR).  Kernel level: every output equals what the prover with the host in the loop gives (low_degree_test.Stir.prove:
the host's sponge, sampling and de-duplication, tvm_gather_elements, stark.auth_nodes).  Host level: the same proof word for word with
the option off and on, the counter, the fallback where the entry point does not apply, the native verifier's acceptance."""
import ctypes as C

import numpy as np
import pytest

from tests.test_stir import odom, small_stir
from triton_vm_amd import native_host, stir_rounds
from triton_vm_amd.prover import ProofStream

# (log2 of the degree bound, query pairs of the full rounds and the final one, seed of the codeword)
INSTANCES = [
    (6, [(3, 1), (2, 0)], 6),
    (8, [(5, 2), (3, 1), (4, 0)], 8),
    (8, [(5, 0), (3, 1), (4, 0)], 8),     # a full round with an empty StirOutOfDomainValues item
    (4, [(3, 0)], 4),                     # no full round, only the final one
    (8, [(40, 2), (6, 1), (4, 0)], 8),    # 40 indices into a folded domain of 256 points: repeats; k = u + 2 < 64 = the folded length
    (8, [(3, 1), (300, 0)], 8),           # a final round beyond the interpolation's 256 points (it has no quotient set), more indices than leaves
]
IDS = ["6-3.1", "8-5.2", "8-empty-ood", "4-final-only", "8-40-repeats", "8-final-300"]


class _Recorded(ProofStream):
    """the host's stream, remembering what it sampled"""

    def __init__(self, lib, state):
        super().__init__(lib)
        self.state[:] = state
        self.sampled_indices = []

    def sample_indices(self, upper_bound, n):
        out = super().sample_indices(upper_bound, n)
        self.sampled_indices.append([int(i) for i in out])
        return out


def _codeword(ctx, orc, stir, log2_bound, seed):
    """an honest codeword: a polynomial of degree < 2^log2_bound on the initial domain"""
    poly = orc.random_elements(np.random.default_rng(seed), (1 << log2_bound, 3))
    return ctx.to_device(orc.coset_evaluate(poly, odom(orc, stir.initial_domain), 3).reshape(-1, 3))


@pytest.mark.parametrize("log2_bound,queries,seed", INSTANCES, ids=IDS)
def test_every_output_equals_what_the_host_loop_gives(ctx, orc, log2_bound, queries, seed):
    stir = small_stir(log2_bound, queries)
    d_codeword = _codeword(ctx, orc, stir, log2_bound, seed)
    state = orc.random_elements(np.random.default_rng(100 + seed), 16)
    ps = _Recorded(ctx.lib, state)
    first = stir.prove(ctx, d_codeword, ps)

    got = stir_rounds.prove_rounds(ctx, state, d_codeword, stir)

    R = len(queries) - 1
    assert got is not None and len(stir.rounds) == R
    roots = [p for label, p, _ in ps.log if label == "stir root"]
    assert len(roots) == R + 1 and (got["roots"] == np.array(roots)).all()
    for r, want in enumerate(stir.rounds):
        assert (got["folding_randomness"][r] == want["folding_randomness"]).all(), r
        assert (got["degree_correction_randomness"][r] == want["degree_correction_randomness"]).all(), r
        assert got["ood_queries"][r].shape == (queries[r][1], 3) and (got["ood_queries"][r] == want["ood_queries"]).all(), r
        assert (got["ood_values"][r] == np.asarray(want["ood_values"]).reshape(-1, 3)).all(), r
        assert got["queried_indices"][r] == [int(i) for i in want["queried_indices"]], r
        assert got["folded_queried"][r] == [int(i) for i in want["folded_queried"]], r      # order: first occurrences
    assert (got["folding_randomness"][R] == stir.final_folding_randomness).all()
    assert got["queried_indices"] == ps.sampled_indices and got["queried_indices"][0] == [int(i) for i in first]
    length = stir.initial_domain.length
    for t in range(R + 1):   # (the final round's list is not kept by the prover: from its sampled indices)
        assert got["folded_queried"][t] == list(dict.fromkeys(i % ((length >> t) // 4) for i in ps.sampled_indices[t])), t
    assert got["final_polynomial"].shape == stir.final_polynomial.shape and (got["final_polynomial"] == stir.final_polynomial).all()
    assert (got["state"] == ps.state).all()
    want_payloads = [p.reshape(-1) for label, p, _ in ps.log if label.startswith("stir response")]
    assert len(want_payloads) == len(got["payloads"]) == 2 * (R + 1)
    offset = 0
    for k, (w, g) in enumerate(zip(want_payloads, got["payloads"])):
        assert got["directory"][k].tolist() == [offset, w.size], k
        assert (g == w).all(), k
        offset += w.size
    assert got["words"] == offset
    if queries[0][0] == 40:   # without a repeated folded index the order of the de-duplication is not tested
        folded = [i % (length // 4) for i in ps.sampled_indices[0]]
        assert len(set(folded)) < len(folded) and got["folded_queried"][0] != sorted(got["folded_queried"][0])
        assert len(got["folded_queried"][0]) + 2 < 64


# ---------------------------------------------------------------------------------------------------- the C++ host
@pytest.fixture()
def host(ctx):
    from tests.test_native_host import _host_library

    lib = _host_library(ctx)
    assert lib.tvmh_get_option(native_host.OPTION_DEVICE_STIR) == 0
    yield lib
    assert lib.tvmh_get_option(native_host.OPTION_DEVICE_STIR) == 0   # whatever a test did, the option is off again


def _off_and_on(host, prove):
    """prove() with the option off and on -> (result off, result on, how many calls of Stir::prove took the device's rounds off / on)"""
    before = host.tvmh_device_stir_proofs()
    off = prove()
    between = host.tvmh_device_stir_proofs()
    with native_host.host_option(host, native_host.OPTION_DEVICE_STIR, 1):
        on = prove()
    return off, on, between - before, host.tvmh_device_stir_proofs() - between


@pytest.mark.parametrize("log2_bound,queries,seed", INSTANCES, ids=IDS)
def test_stir_proof_is_the_same_word_for_word(ctx, orc, host, log2_bound, queries, seed):
    stir = small_stir(log2_bound, queries)
    d_codeword = _codeword(ctx, orc, stir, log2_bound, seed)
    (first_off, off), (first_on, on), taken_off, taken_on = _off_and_on(host, lambda: native_host.stir_prove(ctx, host, stir, d_codeword))
    assert (taken_off, taken_on) == (0, 1)
    assert first_off == first_on and len(first_on) == queries[0][0]
    assert off.size == on.size and (off == on).all()


def test_a_round_beyond_the_limits_is_not_applicable_and_keeps_the_hosts_loop(ctx, orc, host):
    """300 + 1 queries exceed the one-workgroup interpolation's 256 points: the entry point refuses before anything is queued"""
    log2_bound, queries = 12, [(300, 1), (4, 0)]
    stir = small_stir(log2_bound, queries)
    d_codeword = _codeword(ctx, orc, stir, log2_bound, 12)
    lib, rounds = ctx.lib, np.array(stir.round_queries, np.uint64)
    assert lib.tvm_stir_prove_rounds_payload_bound(stir.initial_domain.c(), 4, 1, rounds.ctypes.data, 4) == 0
    sentinel = 0xA5A5A5A5A5A5A5A5
    outs = [np.full(n, sentinel, np.uint64) for n in (16, 10, 3 * 4, 3, 304, 304, 2, 3 * (1 << 10), 8, 64)]
    words = np.full(1, sentinel, np.uint64)
    state = orc.random_elements(np.random.default_rng(1), 16)
    status = lib.tvm_stir_prove_rounds(ctx.handle, state.ctypes.data, d_codeword.ptr, stir.initial_domain.c(), 4, 1, rounds.ctypes.data, 4,
                                       stir.final_degree, *[o.ctypes.data for o in outs[:9]], outs[9].ctypes.data, outs[9].size, words.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert status == stir_rounds.NOT_APPLICABLE
    assert all((o == sentinel).all() for o in outs) and words[0] == sentinel
    assert stir_rounds.prove_rounds(ctx, state, d_codeword, stir) is None
    (first_off, off), (first_on, on), taken_off, taken_on = _off_and_on(host, lambda: native_host.stir_prove(ctx, host, stir, d_codeword))
    assert (taken_off, taken_on) == (0, 0)
    assert first_off == first_on and off.size == on.size and (off == on).all()


def test_more_in_domain_queries_than_the_limit_is_not_applicable(ctx, orc):
    stir = small_stir(12, [(stir_rounds.MAX_INDICES + 1, 0)])
    assert stir_rounds.prove_rounds(ctx, np.zeros(16, np.uint64), _codeword(ctx, orc, stir, 12, 3), stir) is None


def test_whole_stir_proofs_are_the_same_word_for_word_and_verify(ctx, orc, host):
    if ctx.kind == "emu":
        pytest.skip("STIR proofs at security level 160 take minutes on the emulation (CPU suite time); on the GPU")
    import json
    import os

    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays
    from triton_vm_amd.proof_stream import Proof
    from triton_vm_amd.prover import Prover, StarkParameters

    p = StarkParameters(3, ldt="stir")   # as tests/test_device_tail.py::test_stir_proofs_keep_the_hosts_path builds it
    py = Prover(ctx, p, seed=12)
    native = native_host.NativeProver(ctx, host, p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace, py.aux.d_randomizers,
                                      py.quotient_randomizer)
    off, on, taken_off, taken_on = _off_and_on(host, native.prove)
    assert (taken_off, taken_on) == (0, 1)
    assert off.size == on.size and (off == on).all()
    # the program, claim and seed of the committed STIR digest (tests/test_wider_pins.py), from the execution trace
    program, aet, public_input, output = vf.run("tiny")
    claim, arrays = snap.claim_of(orc, program, public_input, output), aet_arrays(orc, aet)
    prove = lambda: native_host.prove_execution(ctx, host, arrays, aet.padded_height(), claim, snap.prover_seed(snap.SEED_U64), ldt="stir")
    off, on, taken_off, taken_on = _off_and_on(host, prove)
    assert (taken_off, taken_on) == (0, 1)
    assert off.size == on.size and (off == on).all()
    with open(os.path.join(os.path.dirname(__file__), "golden", "stir_regression_digests.json")) as f:
        assert [int(w) for w in Proof(on).digest(ctx.lib)] == json.load(f)["tiny"]["digest"]
    assert len(native_host.verify(ctx, host, claim, on, ldt="stir")) > 0   # the revealed first-round indices; raises on a rejection
