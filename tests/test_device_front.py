"""Main root to AIR quotient with the sponge on the device (csrc/proof_front.hip: tvm_front_challenges, tvm_front_quotient_weights,
tvm_front_block; the _device_args twins of the extension and quotient entry points; tvm_out_of_domain_to_deep_device_state; the C++
host under TVMH_OPTION_DEVICE_FRONT).  Kernel level: every word of the front's block equals the Python ProofStream replayed from the
same random state, prover.derive_challenges and tvm_host_xfe_powers; every twin equals the entry point that stages host arrays.  Host
level: the same proof word for word with the option off and on, alone and chained with the middle and the tail, the reference-pinned
digest, the native verifier's acceptance, and the provers that keep the host's path.  All comparisons are exact: integer field
arithmetic."""
import ctypes as C

import numpy as np
import pytest

from triton_vm_amd import capi, field, native_host, proof_front, proof_middle, stark
from triton_vm_amd.prover import Claim, ProofStream, Prover, StarkParameters, derive_challenges, xfe_powers

ERR_INVALID_ARGUMENT = 1


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


# The public input's length, the output's taken from the same list one further: the edges of the chunking over the 64 lanes -- no
# symbol at all, fewer symbols than lanes (empty lanes), 63 / 64 / 65 (one symbol per lane: the last lane empty, all equal, two
# per lane and half the lanes empty), 127 / 128 / 129 likewise at two per lane, and 1000 (16 per lane, the last lanes short and empty).
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000]


class _Front:
    """a random sponge state, a random claim, two random [2 * 2][5] node arrays as the main and the aux tree; tvm_front_challenges and
    tvm_front_quotient_weights queued on one block, and the host's replay of both"""

    def __init__(self, ctx, orc, n_input, n_output):
        rng = np.random.default_rng(1000 * n_input + n_output)
        self.ctx = ctx
        self.state = orc.random_elements(rng, 16)
        self.claim = Claim(orc.random_elements(rng, 5), orc.random_elements(rng, n_input), orc.random_elements(rng, n_output))
        self.main_nodes, self.aux_nodes = orc.random_elements(rng, (4, 5)), orc.random_elements(rng, (4, 5))
        self.d_main_nodes, self.d_aux_nodes = ctx.to_device(self.main_nodes), ctx.to_device(self.aux_nodes)
        assert ctx.lib.tvm_front_block_words() == proof_front.BLOCK_WORDS
        self.d_front = ctx.to_device(np.full(proof_front.BLOCK_WORDS, 0x5A5A5A5A, np.uint64))   # (no word of it is expected to be zero)

    def challenges(self):
        proof_front.front_challenges(self.ctx, self.d_main_nodes, self.state, self.claim.program_digest, self.claim.input, self.claim.output,
                                     self.d_front)

    def weights(self):
        proof_front.front_quotient_weights(self.ctx, self.d_aux_nodes, self.d_front)

    def replay(self):
        """-> (the 63 challenges, the state after them, the weight scalar, the state after it) on the Python ProofStream"""
        lib = self.ctx.lib
        ps = ProofStream(lib)
        ps.state[:] = self.state
        ps.enqueue("main root", self.main_nodes[1])
        ch = derive_challenges(lib, ps.sample_scalars(59), self.claim)
        state_after_challenges = ps.state.copy()
        ps.enqueue("aux root", self.aux_nodes[1])
        w = _h(ps.sample_scalars(1)[0])
        return _h(ch).reshape(63, 3), state_after_challenges, w, ps.state.copy()

    def free(self):
        for b in (self.d_main_nodes, self.d_aux_nodes, self.d_front):
            b.free()


@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_challenges_and_terminals(ctx, orc, k):
    f = _Front(ctx, orc, LENGTHS[k], LENGTHS[(k + 1) % len(LENGTHS)])
    try:
        f.challenges()
        got = proof_front.split_block(proof_front.front_block(ctx, f.d_front, proof_front.HEAD_WORDS))
        ch, state, _, _ = f.replay()
        assert (got["challenges"][:59] == ch[:59]).all()
        for j, name in enumerate(("input", "output", "lookup", "digest")):
            assert (got["challenges"][59 + j] == ch[59 + j]).all(), name
        assert (got["main_root"] == f.main_nodes[1]).all()
        assert (got["state"] == state).all()
    finally:
        f.free()


@pytest.fixture(scope="module")
def front(ctx, orc):
    """both calls queued on one block, the whole block downloaded once; shared by the tests that only read it"""
    f = _Front(ctx, orc, 3, 2)
    f.challenges()
    f.weights()
    f.whole = proof_front.front_block(ctx, f.d_front)
    yield f
    f.free()


def test_quotient_weights(ctx, front):
    got = proof_front.split_block(front.whole)
    ch, _, w, state = front.replay()
    assert (got["challenges"] == ch).all() and (got["main_root"] == front.main_nodes[1]).all()   # left alone by the second call
    assert (got["aux_root"] == front.aux_nodes[1]).all()
    assert (got["weight_scalar"] == w).all()
    assert (got["state"] == state).all()
    assert (got["weights"] == xfe_powers(ctx.lib, w, 0, 604)).all()
    assert (got["weights"][0] == [field.ONE, 0, 0]).all()


def test_a_base_field_weight_scalar(ctx, orc):
    """a scalar with two zero extension words (as a sponge state can make it): the powers stay in the base field"""
    d_front = ctx.to_device(np.zeros(proof_front.BLOCK_WORDS, np.uint64))   # Tip5::init(): a state of zeros
    try:
        d_nodes = ctx.to_device(orc.random_elements(np.random.default_rng(5), (4, 5)))
        proof_front.front_quotient_weights(ctx, d_nodes, d_front)
        got = proof_front.split_block(proof_front.front_block(ctx, d_front))
        ps = ProofStream(ctx.lib)
        ps.enqueue("aux root", d_nodes.download()[5:10])
        w = _h(ps.sample_scalars(1)[0])
        assert (got["weight_scalar"] == w).all() and (got["state"] == ps.state).all()
        assert (got["weights"] == xfe_powers(ctx.lib, w, 0, 604)).all()
        d_nodes.free()
    finally:
        d_front.free()


def test_front_block_head_and_whole_and_without_waiting(ctx, front):
    head = proof_front.front_block(ctx, front.d_front, proof_front.HEAD_WORDS)
    assert head.size == proof_front.HEAD_WORDS and (head == front.whole[:proof_front.HEAD_WORDS]).all()
    assert set(proof_front.split_block(head)) == {"main_root", "aux_root", "challenges", "weight_scalar", "state"}
    later = np.zeros(proof_front.BLOCK_WORDS, np.uint64)
    proof_front.front_block(ctx, front.d_front, wait=False, out=later)
    ctx._check(ctx.lib.tvm_sync(ctx.handle), "tvm_sync")
    assert (later == front.whole).all()
    assert ctx.lib.tvm_front_block_words() == proof_front.BLOCK_WORDS == proof_front.WEIGHTS + 3 * 604


# ---------------------------------------------------------------------------------------------------- the _device_args twins
def test_extend_and_derived_aux_columns_from_device_challenges(ctx, orc):
    """the "tiny" program's padded trace: columns 0..48 by the extension, 49..89 by the degree-lowering fill"""
    from tests import vm_fixture as vf

    main, _, ch, _ = vf.valid_tables("tiny")
    n = main.shape[1]
    ch = _h(ch).reshape(63, 3)
    lib, d_main, d_ch = ctx.lib, ctx.to_device(main), ctx.to_device(ch)
    d_want, d_got = ctx.to_device(np.zeros((91, n, 3), np.uint64)), ctx.to_device(np.zeros((91, n, 3), np.uint64))
    ctx._check(lib.tvm_extend_aux_table(ctx.handle, d_main.ptr, d_want.ptr, n, ch.ctypes.data), "tvm_extend_aux_table")
    proof_front.extend_aux_table_device_args(ctx, d_main, d_got, n, d_ch)
    after_extend = d_got.download((91, n, 3))
    assert (after_extend == d_want.download((91, n, 3))).all() and after_extend[:49].any()
    ctx._check(lib.tvm_fill_derived_aux_columns(ctx.handle, d_main.ptr, d_want.ptr, n, ch.ctypes.data), "tvm_fill_derived_aux_columns")
    proof_front.fill_derived_aux_columns_device_args(ctx, d_main, d_got, n, d_ch)
    after_fill = d_got.download((91, n, 3))
    assert (after_fill == d_want.download((91, n, 3))).all() and after_fill[49:90].any()
    for b in (d_main, d_ch, d_want, d_got):
        b.free()


def _coefficients_twin(ctx, main, aux, trace_dom, quot, ch, w):
    """tvm_all_quotients_coefficients on host arrays -> (status, the number of coefficients, the output array over a sentinel)"""
    out, n = ctx.to_device(np.full((len(quot), 3), 0x5A5A5A5A, np.uint64)), C.c_uint64(77)
    status = ctx.lib.tvm_all_quotients_coefficients(ctx.handle, main._need_table(), aux._need_table(), trace_dom.c(), quot.c(), ch.ctypes.data,
                                                    w.ctypes.data, out.ptr, len(quot), C.byref(n))
    return status, n.value, out.download((len(quot), 3))


def _coefficients_device(ctx, main, aux, trace_dom, quot, d_ch, d_w):
    out, n = ctx.to_device(np.full((len(quot), 3), 0x5A5A5A5A, np.uint64)), C.c_uint64(77)
    status = ctx.lib.tvm_all_quotients_coefficients_device_args(ctx.handle, main._need_table(), aux._need_table(), trace_dom.c(), quot.c(), d_ch.ptr,
                                                                d_w.ptr, out.ptr, len(quot), C.byref(n))
    return status, n.value, out.download((len(quot), 3))


@pytest.mark.parametrize("valid", [False, True])
@pytest.mark.parametrize("log2_rows,log2_expansion", [(3, 2), (4, 2), (3, 4), (4, 4)])
def test_both_quotient_entries_from_device_arrays(ctx, orc, log2_rows, log2_expansion, valid):
    """random tables (the twin is the yardstick): the codeword word for word; the coefficient form's status, count and words -- at these
    sizes it is TVM_NOT_APPLICABLE, zero and nothing written, from the twin as from the entry point"""
    rng = np.random.default_rng(10 * log2_rows + log2_expansion)
    p = StarkParameters(log2_rows, num_trace_randomizers=3, num_collinearity_checks=2, log2_expansion=log2_expansion)
    n = p.trace.length
    py = Prover(ctx, p, orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3)), seed=3)
    py.main.maybe_low_degree_extend_all_columns()
    py.aux.maybe_low_degree_extend_all_columns()
    ch, w = _h(orc.random_elements(rng, (63, 3))), _h(orc.random_elements(rng, (604, 3)))
    d_ch, d_w = ctx.to_device(ch), ctx.to_device(w)
    ctx.assume_valid_trace(valid)
    try:
        want = stark.all_quotients_combined(ctx, py.main, py.aux, p.trace, p.quotient, ch, w).download((len(p.quotient), 3))
        got = proof_front.all_quotients_combined_device_args(ctx, py.main, py.aux, p.trace, p.quotient, d_ch, d_w).download((len(p.quotient), 3))
        assert (got == want).all() and want.any()
        want_c = _coefficients_twin(ctx, py.main, py.aux, p.trace, p.quotient, ch, w)
        got_c = _coefficients_device(ctx, py.main, py.aux, p.trace, p.quotient, d_ch, d_w)
        assert got_c[:2] == want_c[:2] and (got_c[2] == want_c[2]).all()
        assert want_c[:2] == (stark.NOT_APPLICABLE, 0)
        assert proof_front.all_quotients_coefficients_device_args(ctx, py.main, py.aux, p.trace, p.quotient, d_ch, d_w) is None
    finally:
        ctx.assume_valid_trace(False)
    d_ch.free()
    d_w.free()


def test_quotient_coefficients_from_device_arrays_where_the_route_applies(ctx, orc):
    """the valid 256-row trace with the gate lowered (tests/test_quotient_coefficients.py): 4N + n1 coefficients from both"""
    from tests.test_quotient_coefficients import _Options, _valid

    main, aux, trace_dom, quot, ch, weights, _ = _valid(ctx, orc)
    ch, w = _h(ch).reshape(63, 3), _h(weights).reshape(604, 3)
    d_ch, d_w = ctx.to_device(ch), ctx.to_device(w)
    with _Options(ctx):
        want = _coefficients_twin(ctx, main, aux, trace_dom, quot, ch, w)
        got = _coefficients_device(ctx, main, aux, trace_dom, quot, d_ch, d_w)
    assert want[0] == 0 and want[1] == 4 * len(trace_dom) + 16
    assert got[:2] == want[:2] and (got[2] == want[2]).all()
    # the wrapper's three answers: (buffer, 4N + 16) here, None where the route does not apply (the test above), a raise on a refusal
    with _Options(ctx):
        d_coeffs, n_coeffs = proof_front.all_quotients_coefficients_device_args(ctx, main, aux, trace_dom, quot, d_ch, d_w, capacity=want[1])
        assert n_coeffs == want[1] and (d_coeffs.download((n_coeffs, 3)) == want[2][:n_coeffs]).all()
        d_coeffs.free()
        with pytest.raises(capi.TritonHipError) as refusal:
            proof_front.all_quotients_coefficients_device_args(ctx, main, aux, trace_dom, quot, d_ch, d_w, capacity=want[1] - 1)
        assert refusal.value.status == ERR_INVALID_ARGUMENT
        # a capacity one short of 4N + n1, on the route where that check is reached: refused, the count 0, nothing written
        sentinel = np.full((len(quot), 3), 0x5A5A5A5A, np.uint64)
        out, n = ctx.to_device(sentinel), C.c_uint64(77)
        status = ctx.lib.tvm_all_quotients_coefficients_device_args(ctx.handle, main._need_table(), aux._need_table(), trace_dom.c(), quot.c(),
                                                                    d_ch.ptr, d_w.ptr, out.ptr, want[1] - 1, C.byref(n))
        assert status == ERR_INVALID_ARGUMENT and n.value == 0 and (out.download((len(quot), 3)) == sentinel).all()
        out.free()
    with pytest.raises(capi.TritonHipError) as refusal:   # bad arguments: no weights
        proof_front.all_quotients_coefficients_device_args(ctx, main, aux, trace_dom, quot, d_ch, None)
    assert refusal.value.status == ERR_INVALID_ARGUMENT
    d_ch.free()
    d_w.free()


@pytest.fixture(scope="module")
def middle_inputs(ctx, orc):
    """the _Inputs shapes of tests/test_device_middle.py at 2^4 rows: 3 and 7 base-field columns"""
    from tests.test_device_middle import _Inputs

    made = {}
    for expansion, n_main in ((8, 3), (4, 7)):
        rng = np.random.default_rng(100 * 4 + 10 * expansion + n_main)
        made[n_main] = (_Inputs(ctx, orc, rng, 4, expansion, n_main), orc.random_elements(rng, 16))
    yield made
    for inputs, _ in made.values():
        inputs.free()


@pytest.mark.parametrize("with_tree", [True, False])
@pytest.mark.parametrize("n_main", [3, 7])
def test_the_middle_from_a_device_state(ctx, middle_inputs, n_main, with_tree):
    i, state = middle_inputs[n_main]
    if not with_tree:   # the state already holds the root
        ps = ProofStream(ctx.lib)
        ps.state[:] = state
        ps.enqueue("quot root", i.root)
        state = ps.state.copy()
    want_deep, want = i.device_middle(state, with_tree)
    d_state = ctx.to_device(_h(state))
    got_deep, got = proof_front.out_of_domain_to_deep_device_state(ctx, i.traces[0], i.n_main, i.rnd[0], i.traces[1], i.n_aux, i.rnd[1], i.n, 3,
                                                                   i.trace_dom, i.segments.polys, i.segments.poly_len, i.segments.table,
                                                                   i.d_nodes if with_tree else None, i.short, d_state)
    for name in want:
        assert (got[name] == want[name]).all(), name
    assert (got_deep.download()[:3 * i.short.length] == want_deep.download()[:3 * i.short.length]).all()
    assert (d_state.download()[:16] == want["state"]).all() and (want["state"] != state).any()
    d_state.free()


def test_bad_arguments_queue_nothing(ctx, orc, front, middle_inputs):
    lib, h = ctx.lib, ctx.handle
    sentinel = np.full(proof_front.BLOCK_WORDS, 12345, np.uint64)
    d_front = ctx.to_device(sentinel)
    st, digest, words = _h(front.state), _h(front.claim.program_digest), _h(front.claim.input)
    nodes = front.d_main_nodes.ptr

    def challenges(nodes=nodes, state=st.ctypes.data, digest=digest.ctypes.data, inp=words.ctypes.data, n_in=words.size, out=None, n_out=0,
                   block=d_front.ptr, c=h):
        return lib.tvm_front_challenges(c, nodes, state, digest, inp, n_in, out, n_out, block)

    for bad in (dict(nodes=None), dict(state=None), dict(digest=None), dict(inp=None), dict(out=None, n_out=1), dict(block=None), dict(c=None)):
        assert challenges(**bad) == ERR_INVALID_ARGUMENT, bad
    assert lib.tvm_front_quotient_weights(h, None, d_front.ptr) == ERR_INVALID_ARGUMENT
    assert lib.tvm_front_quotient_weights(h, nodes, None) == ERR_INVALID_ARGUMENT
    assert lib.tvm_front_quotient_weights(None, nodes, d_front.ptr) == ERR_INVALID_ARGUMENT
    back = np.full(proof_front.BLOCK_WORDS + 1, 777, np.uint64)
    for bad in ((None, back.ctypes.data, 5), (d_front.ptr, None, 5), (d_front.ptr, back.ctypes.data, 0),
                (d_front.ptr, back.ctypes.data, proof_front.BLOCK_WORDS + 1)):
        assert lib.tvm_front_block(h, *bad, 1) == ERR_INVALID_ARGUMENT, bad
    assert (back == 777).all()
    # the twins: null arrays, and a short capacity
    n, d = 16, d_front.ptr
    assert lib.tvm_extend_aux_table_device_args(h, d, d, n, None) == ERR_INVALID_ARGUMENT
    assert lib.tvm_extend_aux_table_device_args(h, None, d, n, d) == ERR_INVALID_ARGUMENT
    assert lib.tvm_fill_derived_aux_columns_device_args(h, d, d, n, None) == ERR_INVALID_ARGUMENT
    assert lib.tvm_fill_derived_aux_columns_device_args(h, d, None, n, d) == ERR_INVALID_ARGUMENT
    from triton_vm_amd.arithmetic_domain import ArithmeticDomain

    dom, n_coeffs = ArithmeticDomain.of_length(16), C.c_uint64(77)
    assert lib.tvm_all_quotients_combined_device_args(h, None, None, dom.c(), dom.c(), d, d, d) == ERR_INVALID_ARGUMENT
    assert lib.tvm_all_quotients_coefficients_device_args(h, None, None, dom.c(), dom.c(), d, d, d, 16, C.byref(n_coeffs)) == ERR_INVALID_ARGUMENT
    assert lib.tvm_all_quotients_coefficients_device_args(h, None, None, dom.c(), dom.c(), d, d, d, 16, None) == ERR_INVALID_ARGUMENT
    i, state = middle_inputs[3]
    block = np.full(proof_middle.block_words(i.n_main, i.n_aux), 12345, np.uint64)
    d_out, d_state = ctx.alloc(3 * i.short.length), ctx.to_device(_h(state))

    def middle(main_trace=i.traces[0].ptr, d_state=d_state.ptr, capacity=block.size):
        return lib.tvm_out_of_domain_to_deep_device_state(h, main_trace, i.n_main, i.rnd[0].ptr, i.traces[1].ptr, i.n_aux, i.rnd[1].ptr, i.n, 3,
                                                          i.trace_dom.c(), i.segments.polys.ptr, i.segments.poly_len, i.segments.table, i.d_nodes.ptr,
                                                          i.short.c(), stark.ZETA, d_state, d_out.ptr, block.ctypes.data, capacity)

    assert middle(main_trace=None) == ERR_INVALID_ARGUMENT
    assert middle(d_state=None) == ERR_INVALID_ARGUMENT
    assert middle(capacity=block.size - 1) == ERR_INVALID_ARGUMENT
    ctx._check(lib.tvm_sync(h), "tvm_sync")
    assert (block == 12345).all() and (d_state.download()[:16] == state).all()   # nothing was written
    assert (d_front.download()[:proof_front.BLOCK_WORDS] == sentinel).all()
    assert challenges() == 0 and lib.tvm_front_quotient_weights(h, nodes, d_front.ptr) == 0
    assert (proof_front.front_block(ctx, d_front) != sentinel).all()
    for b in (d_front, d_out, d_state):
        b.free()


# ---------------------------------------------------------------------------------------------------- the C++ host
FRONT, MIDDLE, TAIL, STIR = (native_host.OPTION_DEVICE_FRONT, native_host.OPTION_DEVICE_MIDDLE, native_host.OPTION_DEVICE_TAIL,
                             native_host.OPTION_DEVICE_STIR)


@pytest.fixture(autouse=True)
def option_hygiene(ctx):
    """the four options read 0 before and after every test of this file, whatever the test did"""
    from tests.test_native_host import _host_library

    lib = _host_library(ctx)
    assert [lib.tvmh_get_option(o) for o in (FRONT, MIDDLE, TAIL, STIR)] == [0, 0, 0, 0]   # the defaults
    yield lib
    assert [lib.tvmh_get_option(o) for o in (FRONT, MIDDLE, TAIL, STIR)] == [0, 0, 0, 0]


@pytest.fixture()
def host(option_hygiene):
    return option_hygiene


def _with_options(host, options, prove):
    previous = [host.tvmh_get_option(o) for o in options]
    for o in options:
        host.tvmh_set_option(o, 1)
    try:
        return prove()
    finally:
        for o, v in zip(options, previous):
            host.tvmh_set_option(o, v)


def _in_settings(host, prove, settings):
    """prove() under each tuple of options -> (the proofs, tvmh_device_front_proofs() after each, counted from before the first)"""
    before, proofs, taken = host.tvmh_device_front_proofs(), [], []
    for options in settings:
        proofs.append(_with_options(host, options, prove))
        taken.append(host.tvmh_device_front_proofs() - before)
    return proofs, taken


def _all_equal(proofs):
    return all(q.size == proofs[0].size and (q == proofs[0]).all() for q in proofs[1:])


@pytest.mark.parametrize("log2_rows,h,checks,log2_expansion", [(3, 3, 2, 2), (4, 5, 4, 2), (3, 3, 3, 4)])
def test_hot_path_proof_is_the_same_word_for_word(ctx, orc, host, log2_rows, h, checks, log2_expansion):
    """random traces through tvmh_prove: off, FRONT, FRONT + MIDDLE, FRONT + MIDDLE + TAIL"""
    rng = np.random.default_rng(log2_rows)
    p = StarkParameters(log2_rows, num_trace_randomizers=h, num_collinearity_checks=checks, log2_expansion=log2_expansion)
    n = p.trace.length
    claim = Claim(orc.random_elements(rng, 5), orc.random_elements(rng, 3), orc.random_elements(rng, 2))
    py = Prover(ctx, p, orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3)), seed=9, claim=claim)
    native = native_host.NativeProver(ctx, host, p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace, py.aux.d_randomizers,
                                      py.quotient_randomizer, claim)
    middle_before = host.tvmh_device_middle_proofs()
    proofs, taken = _in_settings(host, native.prove, ((), (FRONT,), (FRONT, MIDDLE), (FRONT, MIDDLE, TAIL)))
    assert taken == [0, 1, 2, 3]
    assert host.tvmh_device_middle_proofs() - middle_before == 2
    assert _all_equal(proofs)


@pytest.fixture(scope="module")
def tiny(orc):
    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays

    program, aet, public_input, output = vf.run("tiny")
    return snap.claim_of(orc, program, public_input, output), aet_arrays(orc, aet), aet.padded_height(), snap.prover_seed(snap.SEED_U64)


@pytest.mark.parametrize("options", [(FRONT,), (FRONT, MIDDLE)], ids=["front", "front+middle"])
def test_the_reference_pinned_proof_with_the_option_on(ctx, host, tiny, options):
    """the program, claim and seed of the reference's proof-digest snapshot (tests/test_proof_snapshot.py): the case with extend_device"""
    from tests import test_proof_snapshot as snap
    from triton_vm_amd.proof_stream import Proof

    claim, arrays, padded_height, seed = tiny
    taken = host.tvmh_device_front_proofs()
    on = _with_options(host, options, lambda: native_host.prove_execution(ctx, host, arrays, padded_height, claim, seed, ldt="fri"))
    assert host.tvmh_device_front_proofs() - taken == 1
    assert Proof(on).digest(ctx.lib) == snap.SNAPSHOT
    assert len(native_host.verify(ctx, host, claim, on, ldt="fri")) == 173


def test_exact_air_with_the_option_on(ctx, host, tiny):
    claim, arrays, padded_height, seed = tiny
    prove = lambda: native_host.prove_execution(ctx, host, arrays, padded_height, claim, seed, ldt="fri")
    EXACT = native_host.OPTION_EXACT_AIR
    (off, on), taken = _in_settings(host, prove, ((EXACT,), (EXACT, FRONT)))
    assert taken == [0, 1]
    assert off.size == on.size and (off == on).all()
    assert host.tvmh_get_option(EXACT) == 0


def test_a_checked_proof_keeps_the_hosts_front(ctx, host, tiny):
    from tests import test_proof_snapshot as snap
    from triton_vm_amd.proof_stream import Proof

    claim, arrays, padded_height, seed = tiny
    CHECK = native_host.OPTION_CHECK_TRACE
    taken = host.tvmh_device_front_proofs()
    on = _with_options(host, (CHECK, FRONT), lambda: native_host.prove_execution(ctx, host, arrays, padded_height, claim, seed, ldt="fri"))
    assert host.tvmh_device_front_proofs() == taken
    assert Proof(on).digest(ctx.lib) == snap.SNAPSHOT   # the option-off proof (tests/test_proof_snapshot.py)
    assert host.tvmh_get_option(CHECK) == 0


def test_forced_stir_with_front_middle_and_device_stir(ctx, orc, host):
    p = StarkParameters(3, ldt="stir")   # as tests/test_device_stir.py builds it
    py = Prover(ctx, p, seed=12)
    native = native_host.NativeProver(ctx, host, p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace, py.aux.d_randomizers,
                                      py.quotient_randomizer)
    (off, on), taken = _in_settings(host, native.prove, ((), (FRONT, MIDDLE, STIR)))
    assert taken == [0, 1]
    assert off.size == on.size and (off == on).all()


@pytest.mark.parametrize("ldt", ["fri", "stir"])
def test_prove_fib_at_1024_rows_is_the_same_word_for_word_and_verifies(ctx, orc, host, ldt):
    if ctx.kind == "emu":
        pytest.skip("three proofs of a 2^10-row trace at security level 160 take minutes on the emulation (CPU suite time); on the GPU")
    from oracle.vm import workload
    from triton_vm_amd.master_table import aet_to_device

    e = workload.execution("fib", 10)
    assert e["padded_height"] == 1 << 10
    claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
    aet = aet_to_device(ctx, e["aet"])
    prove = lambda: native_host.prove_execution(ctx, host, aet, e["padded_height"], claim, bytes(range(32)), ldt=ldt)
    (off, on), taken = _in_settings(host, prove, ((), (FRONT, MIDDLE, TAIL, STIR)))
    assert taken == [0, 1]
    assert off.size == on.size and (off == on).all()
    assert native_host.verify(ctx, host, claim, on, ldt=ldt)


def test_the_sharded_prover_keeps_the_hosts_path(ctx, orc, host):
    """two in-process ranks with the option on: the counter does not move, and the proof is the single-GPU one"""
    from tests import test_sharded_host as sh

    p = sh._params("fri")
    main_trace, aux_trace = sh._inputs(orc, p)
    py, want = sh._single_proof(ctx, host, p, main_trace, aux_trace)
    comms = native_host.LocalComms(host, 2)
    try:
        def rank_body(rank):
            c = sh._new_context(ctx)   # one context per proving thread
            try:
                mine = Prover(c, p, main_trace, aux_trace, seed=sh.SEED)
                return native_host.prove_sharded(c, host, comms.ptrs[rank], p, mine.main.d_trace, mine.main.d_randomizers, mine.aux.d_trace,
                                                 mine.aux.d_randomizers, mine.quotient_randomizer, split_tree_min_leaves=0)
            finally:
                c.close()

        with native_host.host_option(host, FRONT, 1):
            taken = host.tvmh_device_front_proofs()
            proofs = sh._run_ranks(2, rank_body, comms)
            assert host.tvmh_device_front_proofs() == taken
    finally:
        comms.close()
    for rank, got in enumerate(proofs):
        assert got.size == want.size and (got == want).all(), rank
