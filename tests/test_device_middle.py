"""Out-of-domain rows to DEEP in one device round trip (csrc/proof_middle.hip: tvm_out_of_domain_to_deep; the C++ host under
TVMH_OPTION_DEVICE_MIDDLE).  Kernel level: every word of the block that comes back and of the DEEP codeword equals the composition of
the existing calls -- tvm_out_of_domain_rows, tvm_evaluate_polys_at_points, tvm_weighted_sum_of_columns, tvm_xfe_add_assign,
tvm_evaluate, tvm_table_linear_combination, tvm_evaluate_at_points, tvm_deep_codeword -- with the host's sponge replayed from the same
state.  Host level: the same proof word for word with the option off and on, the reference-pinned digest, the native verifier's
acceptance, and the provers that keep the host's path.  All comparisons are exact: integer field arithmetic."""
import ctypes as C

import numpy as np
import pytest

from triton_vm_amd import field, native_host, proof_middle, stark
from triton_vm_amd.arithmetic_domain import ArithmeticDomain
from triton_vm_amd.prover import Claim, ProofStream, Prover, StarkParameters

H = 3   # trace randomizers per column
ERR_INVALID_ARGUMENT = 1


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _xfe_mul(lib, a, b):
    out = np.zeros(3, np.uint64)
    lib.tvm_host_xfe_mul(_h(a).ctypes.data, _h(b).ctypes.data, out.ctypes.data)
    return out


def _xfe_powers(lib, x, first, n):
    out = np.zeros((n, 3), np.uint64)
    lib.tvm_host_xfe_powers(_h(x).ctypes.data, first, n, out.ctypes.data)
    return out


def _scale(lib, x, s):
    return _xfe_mul(lib, x, [s, 0, 0])


def _dot(lib, weights, values):
    acc = np.zeros(3, np.uint64)
    for w, v in zip(weights, values):
        prod = _xfe_mul(lib, w, v)
        acc = _h([(int(a) + int(b)) % field.P for a, b in zip(acc, prod)])   # canonical Montgomery words add as integers mod p
    return acc


class _Inputs:
    """random traces with their randomizers (a base-field table of n_main columns, an extension-field one of 5) over a trace domain of
    n rows, their tables through tvm_lde_table as the prover holds them, and a segment table with its polynomials and tree through
    stark.quotient_segments on the quotient domain (4 n points) inside the LDT domain (expansion * n points)"""

    def __init__(self, ctx, orc, rng, log_n, expansion, n_main, n_aux=5):
        n = 1 << log_n
        self.ctx, self.n, self.n_main, self.n_aux = ctx, n, n_main, n_aux
        self.trace_dom = ArithmeticDomain.of_length(n)
        self.ldt = ArithmeticDomain.of_length(expansion * n).with_offset(field.to_mont(7))
        self.quotient = ArithmeticDomain.of_length(4 * n).with_offset(field.to_mont(7))
        self.short = self.quotient if self.quotient.length <= self.ldt.length else self.ldt
        self.traces, self.rnd, self.tables = [], [], []
        for fk, n_cols in ((1, n_main), (3, n_aux)):
            self.traces.append(ctx.to_device(orc.random_elements(rng, n_cols * n * fk)))
            self.rnd.append(ctx.to_device(orc.random_elements(rng, n_cols * H * fk)))
            t = C.c_void_p()
            ctx._check(ctx.lib.tvm_lde_table(ctx.handle, fk, self.traces[-1].ptr, n, n_cols, self.rnd[-1].ptr, H, self.trace_dom.c(), self.ldt.c(),
                                             C.byref(t)), "tvm_lde_table")
            self.tables.append(t.value)
        self.segments = stark.quotient_segments(ctx, ctx.to_device(orc.random_elements(rng, (self.quotient.length, 3))), self.quotient, self.ldt,
                                                orc.random_elements(rng, (4, 3)))
        self.d_nodes = ctx.alloc(10 * self.ldt.length)
        ctx._check(ctx.lib.tvm_table_merkle_tree(ctx.handle, self.segments.table, self.ldt.length, self.d_nodes.ptr), "tvm_table_merkle_tree")
        self.root = self.d_nodes.download()[5:10]

    def device_middle(self, state, with_tree):
        return proof_middle.out_of_domain_to_deep(self.ctx, self.traces[0], self.n_main, self.rnd[0], self.traces[1], self.n_aux, self.rnd[1], self.n, H,
                                                  self.trace_dom, self.segments.polys, self.segments.poly_len, self.segments.table,
                                                  self.d_nodes if with_tree else None, self.short, state)

    def existing_calls(self, state):
        """steps 12-16 of Prover::prove through the entry points the host path uses, the Python ProofStream as the transcript
        -> (the block's fields, the DEEP codeword)"""
        ctx, lib, n = self.ctx, self.ctx.lib, self.n
        ps = ProofStream(lib)
        ps.state[:] = state
        ps.enqueue("quot root", self.root)
        alpha = ps.sample_scalars(1)[0]
        alpha_next = _scale(lib, alpha, self.trace_dom.generator)
        a4 = _xfe_powers(lib, alpha, 4, 1)[0]
        za4 = _xfe_powers(lib, _scale(lib, alpha, stark.ZETA), 4, 1)[0]
        points = _h([alpha, alpha_next, a4, za4])
        rows = []
        for fk, n_cols, trace, rnd in ((1, self.n_main, *self._tr(0)), (3, self.n_aux, *self._tr(1))):
            out = np.zeros((2, n_cols, 3), np.uint64)
            ctx._check(lib.tvm_out_of_domain_rows(ctx.handle, fk, trace.ptr, n, n_cols, rnd.ptr, H, self.trace_dom.c(), points[:2].ctypes.data, 2,
                                                  out.ctypes.data), "tvm_out_of_domain_rows")
            rows.append(out)
        seg, poly_len = np.zeros((5, 2, 3), np.uint64), self.segments.poly_len
        pts = _h(points[2:])
        ctx._check(lib.tvm_evaluate_polys_at_points(ctx.handle, self.segments.polys.ptr, poly_len, poly_len, 5, pts.ctypes.data, 2, seg.ctypes.data),
                   "tvm_evaluate_polys_at_points")
        ps.enqueue("ood main", rows[0][0])
        ps.enqueue("ood aux", rows[1][0])
        ps.enqueue("ood main next", rows[0][1])
        ps.enqueue("ood aux next", rows[1][1])
        ps.enqueue("ood quot p", seg[:4, 0])
        ps.enqueue("ood quot r", seg[1:, 1])
        w3 = _h(ps.sample_scalars(3))
        w_ma = _xfe_powers(lib, w3[0], 0, self.n_main + self.n_aux)
        w_q, w_d = _xfe_powers(lib, w3[1], 0, 5), _xfe_powers(lib, w3[2], 0, 4)
        comb, comb_aux = ctx.alloc(2 * n * 3), ctx.alloc(2 * n * 3)
        for fk, n_cols, trace, rnd, w, out in ((1, self.n_main, *self._tr(0), w_ma[:self.n_main], comb), (3, self.n_aux, *self._tr(1), w_ma[self.n_main:], comb_aux)):
            w = _h(w)
            ctx._check(lib.tvm_weighted_sum_of_columns(ctx.handle, fk, trace.ptr, n, n_cols, rnd.ptr, H, self.trace_dom.c(), w.ctypes.data, out.ptr),
                       "tvm_weighted_sum_of_columns")
        ctx._check(lib.tvm_xfe_add_assign(ctx.handle, comb.ptr, comb_aux.ptr, 2 * n), "tvm_xfe_add_assign")
        main_aux_codeword = self.short.evaluate(ctx, comb, n + H, 3)
        wp, wr = w_q.copy(), w_q.copy()
        wp[4], wr[0] = 0, 0
        cw_p, cw_r = self.segments.linear_combination(wp, self.short.length), self.segments.linear_combination(wr, self.short.length)
        ma_values = stark.evaluate_at_points(ctx, comb, n + H, points[:2])
        p_value, r_value = _dot(lib, w_q[:4], seg[:4, 0]), _dot(lib, w_q[1:], seg[1:, 1])
        values = _h([ma_values[0], ma_values[1], p_value, r_value])
        deep = stark.deep_codeword(ctx, [main_aux_codeword, main_aux_codeword, cw_p, cw_r], self.short, points, values, w_d)
        want = dict(root=self.root, points=points, main_rows=rows[0], aux_rows=rows[1], segments=seg, values=values, weights=w3, state=ps.state.copy())
        return want, deep.download()[:3 * self.short.length]

    def _tr(self, which):
        return self.traces[which], self.rnd[which]

    def free(self):
        for t in self.tables:
            self.ctx.lib.tvm_table_free(self.ctx.handle, t)
        self.segments.free()
        for b in self.traces + self.rnd + [self.d_nodes]:
            b.free()


# (log2 of the trace length, LDT expansion, base-field columns): 2^4 is the smallest shape the table kernels take; 3 base-field columns
# make the item 1 + 3 * 3 = 10 words, a whole block, so its padding is a block of its own; 7 columns (22 words) and the 5
# extension-field columns (16 words) end inside a block.  Expansion 8: the quotient domain is the short one, a stride view of the
# segment table; expansion 4: the LDT domain itself.
CASES = [(4, 8, 3), (4, 4, 7), (6, 4, 3), (6, 8, 7), (10, 8, 7), (10, 4, 3)]


@pytest.fixture(scope="module")
def inputs_of(ctx, orc):
    """one set of inputs and ONE reference per case, shared by the tree-given and the null-tree test (they are only read)"""
    cache = {}

    def get(case):
        if case not in cache:
            log_n, expansion, n_main = case
            rng = np.random.default_rng(100 * log_n + 10 * expansion + n_main)
            inputs = _Inputs(ctx, orc, rng, log_n, expansion, n_main)
            state = orc.random_elements(rng, 16)
            cache[case] = (inputs, state, inputs.existing_calls(state))
        return cache[case]

    yield get
    for inputs, _, _ in cache.values():
        inputs.free()


def _same(got_block, got_deep, want, want_deep, root):
    for name in ("points", "main_rows", "aux_rows", "segments", "values", "weights", "state"):
        assert (got_block[name] == want[name]).all(), name
    assert (got_block["root"] == root).all()
    assert (got_deep == want_deep).all()


@pytest.mark.parametrize("case", CASES)
def test_every_output_equals_what_the_existing_calls_give(ctx, inputs_of, case):
    inputs, state, (want, want_deep) = inputs_of(case)
    d_deep, block = inputs.device_middle(state, with_tree=True)
    _same(block, d_deep.download()[:3 * inputs.short.length], want, want_deep, want["root"])


@pytest.mark.parametrize("case", CASES[:2] + CASES[-1:])
def test_without_a_tree_the_state_already_holds_the_root(ctx, inputs_of, case):
    inputs, state, (want, want_deep) = inputs_of(case)
    ps = ProofStream(ctx.lib)
    ps.state[:] = state
    ps.enqueue("quot root", inputs.root)
    d_deep, block = inputs.device_middle(ps.state, with_tree=False)
    _same(block, d_deep.download()[:3 * inputs.short.length], want, want_deep, np.zeros(5, np.uint64))


@pytest.mark.parametrize("length", [2, 4, 8, 1024])
@pytest.mark.parametrize("n_components", [1, 2, 3, 4])
def test_deep_codeword_with_device_arguments(ctx, orc, length, n_components):
    """length 2 is the only way to the _short kernel; at 4 and 8 one and two work-items own all the points; 1024: more than a workgroup"""
    rng = np.random.default_rng(10 * length + n_components)
    dom = ArithmeticDomain.of_length(length).with_offset(field.to_mont(7))
    codewords = [ctx.to_device(orc.random_elements(rng, (length, 3))) for _ in range(n_components)]
    points, values, weights = (orc.random_elements(rng, (n_components, 3)) for _ in range(3))
    want = stark.deep_codeword(ctx, codewords, dom, points, values, weights).download()[:3 * length]
    got = proof_middle.deep_codeword_device_args(ctx, codewords, dom, ctx.to_device(points), ctx.to_device(values), ctx.to_device(weights))
    assert (got.download()[:3 * length] == want).all()


@pytest.mark.parametrize("n_columns", [1, 64, 65, 470])
def test_weight_vectors_are_the_hosts_powers(ctx, orc, n_columns):
    """w0 a base-field value (two zero extension words, as a sponge state can make it), w1 and w2 general"""
    rng = np.random.default_rng(n_columns)
    lib = ctx.lib
    scalars, segments = orc.random_elements(rng, (3, 3)), orc.random_elements(rng, (5, 2, 3))
    scalars[0, 1:] = 0
    got = proof_middle.combination_weight_vectors(ctx, scalars, segments, n_columns)
    w_q = _xfe_powers(lib, scalars[1], 0, 5)
    assert (got["w_columns"] == _xfe_powers(lib, scalars[0], 0, n_columns)).all()
    assert (got["w_columns"][:, 1:] == 0).all()
    assert (got["wp"][:4] == w_q[:4]).all() and (got["wp"][4] == 0).all()
    assert (got["wr"][1:] == w_q[1:]).all() and (got["wr"][0] == 0).all()
    assert (got["wd"] == _xfe_powers(lib, scalars[2], 0, 4)).all()
    assert (got["pr_values"][0] == _dot(lib, w_q[:4], segments[:4, 0])).all()
    assert (got["pr_values"][1] == _dot(lib, w_q[1:], segments[1:, 1])).all()


def test_a_base_field_out_of_domain_point(ctx, inputs_of):
    """a state whose first three words -- the scalar the next squeeze hands out -- are a base-field value: alpha^4 and (zeta alpha)^4
    are base-field values too, and every output still equals the existing calls'"""
    inputs, state, _ = inputs_of(CASES[0])
    state = state.copy()
    state[1:3] = 0
    ps = ProofStream(ctx.lib)
    ps.state[:] = state
    alpha = ps.sample_scalars(1)[0]
    assert alpha[0] == state[0] and (_h(alpha)[1:] == 0).all()
    _, block = inputs.device_middle(state, with_tree=False)
    assert (block["points"][0] == alpha).all() and (block["points"][:, 1:] == 0).all()
    assert (block["points"][2] == _xfe_powers(ctx.lib, alpha, 4, 1)[0]).all()


def test_bad_arguments_queue_nothing(ctx, inputs_of):
    inputs, state, _ = inputs_of(CASES[0])
    lib, i = ctx.lib, inputs
    block = np.full(proof_middle.block_words(i.n_main, i.n_aux), 12345, np.uint64)
    d_out = ctx.alloc(3 * i.short.length)
    st = _h(state)

    def call(main_trace=i.traces[0].ptr, short=i.short.c(), capacity=block.size):
        return lib.tvm_out_of_domain_to_deep(ctx.handle, main_trace, i.n_main, i.rnd[0].ptr, i.traces[1].ptr, i.n_aux, i.rnd[1].ptr, i.n, H,
                                             i.trace_dom.c(), i.segments.polys.ptr, i.segments.poly_len, i.segments.table, i.d_nodes.ptr, short,
                                             stark.ZETA, st.ctypes.data, d_out.ptr, block.ctypes.data, capacity)

    from triton_vm_amd.capi import Domain

    assert call(main_trace=None) == ERR_INVALID_ARGUMENT
    assert call(short=Domain(i.short.offset, i.short.generator, i.short.length - 1)) == ERR_INVALID_ARGUMENT
    assert call(short=Domain(i.short.offset, i.short.generator, 2 * i.ldt.length)) == ERR_INVALID_ARGUMENT   # beyond the segment table
    assert call(capacity=block.size - 1) == ERR_INVALID_ARGUMENT
    assert (block == 12345).all()   # nothing was written
    assert call() == 0 and (block != 12345).any()
    assert lib.tvm_deep_codeword_device_args(ctx.handle, 5, (C.c_void_p * 5)(*[d_out.ptr] * 5), i.short.c(), d_out.ptr, d_out.ptr, d_out.ptr,
                                             d_out.ptr) == ERR_INVALID_ARGUMENT
    assert lib.tvm_deep_codeword_device_args(ctx.handle, 1, (C.c_void_p * 1)(d_out.ptr), i.short.c(), None, d_out.ptr, d_out.ptr,
                                             d_out.ptr) == ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------- the C++ host
MIDDLE, TAIL, STIR = native_host.OPTION_DEVICE_MIDDLE, native_host.OPTION_DEVICE_TAIL, native_host.OPTION_DEVICE_STIR


@pytest.fixture()
def host(ctx):
    from tests.test_native_host import _host_library

    lib = _host_library(ctx)
    assert lib.tvmh_get_option(MIDDLE) == 0   # the default
    yield lib
    assert lib.tvmh_get_option(MIDDLE) == 0   # whatever a test did, the option is off again


def _in_three_settings(host, prove, other):
    """prove() with the option off, on, and on together with `other` (DEVICE_TAIL for FRI, DEVICE_STIR for STIR)
    -> (the three proofs, tvmh_device_middle_proofs() after each, counted from before the first)"""
    before, proofs, taken = host.tvmh_device_middle_proofs(), [], []
    for options in ((), (MIDDLE,), (MIDDLE, other)):
        previous = [host.tvmh_get_option(o) for o in options]
        for o in options:
            host.tvmh_set_option(o, 1)
        try:
            proofs.append(prove())
        finally:
            for o, v in zip(options, previous):
                host.tvmh_set_option(o, v)
        taken.append(host.tvmh_device_middle_proofs() - before)
    return proofs, taken


@pytest.mark.parametrize("log2_rows,h,checks,log2_expansion", [(3, 3, 2, 2), (4, 5, 4, 2), (3, 3, 3, 4)])
def test_hot_path_proof_is_the_same_word_for_word(ctx, orc, host, log2_rows, h, checks, log2_expansion):
    """random traces through tvmh_prove; expansion 16: the quotient domain is the short one, and the combination is extended afterwards"""
    rng = np.random.default_rng(log2_rows)
    p = StarkParameters(log2_rows, num_trace_randomizers=h, num_collinearity_checks=checks, log2_expansion=log2_expansion)
    n = p.trace.length
    claim = Claim(orc.random_elements(rng, 5), orc.random_elements(rng, 3), orc.random_elements(rng, 2))
    py = Prover(ctx, p, orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3)), seed=9, claim=claim)
    native = native_host.NativeProver(ctx, host, p, py.main.d_trace, py.main.d_randomizers, py.aux.d_trace, py.aux.d_randomizers,
                                      py.quotient_randomizer, claim)
    (off, on, both), taken = _in_three_settings(host, native.prove, TAIL)
    assert taken == [0, 1, 2]
    assert off.size == on.size == both.size and (off == on).all() and (off == both).all()


def test_the_reference_pinned_proof_with_the_option_on(ctx, orc, host):
    """the program, claim and seed of the reference's proof-digest snapshot (tests/test_proof_snapshot.py)"""
    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays
    from triton_vm_amd.proof_stream import Proof

    program, aet, public_input, output = vf.run("tiny")
    claim, arrays = snap.claim_of(orc, program, public_input, output), aet_arrays(orc, aet)
    with native_host.host_option(host, MIDDLE, 1):
        taken = host.tvmh_device_middle_proofs()
        on = native_host.prove_execution(ctx, host, arrays, aet.padded_height(), claim, snap.prover_seed(snap.SEED_U64), ldt="fri")
        assert host.tvmh_device_middle_proofs() - taken == 1
    assert Proof(on).digest(ctx.lib) == snap.SNAPSHOT
    assert len(native_host.verify(ctx, host, claim, on, ldt="fri")) == 173


@pytest.mark.parametrize("ldt", ["fri", "stir"])
def test_prove_fib_at_1024_rows_is_the_same_word_for_word_and_verifies(ctx, orc, host, ldt):
    """no STIR digest is committed for this size (tests/golden/oracle_proof_digests.json starts at 2^16 rows): against option off"""
    if ctx.kind == "emu":
        pytest.skip("three proofs of a 2^10-row trace at security level 160 take minutes on the emulation (CPU suite time); on the GPU")
    from oracle.vm import workload
    from triton_vm_amd.master_table import aet_to_device

    e = workload.execution("fib", 10)
    assert e["padded_height"] == 1 << 10
    claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
    aet = aet_to_device(ctx, e["aet"])
    prove = lambda: native_host.prove_execution(ctx, host, aet, e["padded_height"], claim, bytes(range(32)), ldt=ldt)
    (off, on, both), taken = _in_three_settings(host, prove, TAIL if ldt == "fri" else STIR)
    assert taken == [0, 1, 2]
    assert off.size == on.size == both.size and (off == on).all() and (off == both).all()
    assert native_host.verify(ctx, host, claim, on, ldt=ldt)   # (the three are the same words)


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

        with native_host.host_option(host, MIDDLE, 1):
            taken = host.tvmh_device_middle_proofs()
            proofs = sh._run_ranks(2, rank_body, comms)
            assert host.tvmh_device_middle_proofs() == taken
    finally:
        comms.close()
    for rank, got in enumerate(proofs):
        assert got.size == want.size and (got == want).all(), rank
