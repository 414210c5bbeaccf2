"""The combined quotient in coefficient form (tvm_all_quotients_coefficients) and the segments taken from it
(tvm_quotient_segments_from_coefficients): what Prover::prove uses instead of a quotient codeword where valid-trace mode already
holds the quotient as coefficients.

The gate is the remainder-coset one, lowered to the 256-row trace through TVM_OPTION_AIR_REMAINDER_MIN_ROWS as in
tests/test_air_remainder_coset.py: n1 = 16 rows per block there, and h = 3 trace randomizers leave class 0 -- the initial /
terminal quotients of the degree-4 constraints, fewer than 4N + 4h - 3 coefficients -- 9 <= 16 coefficients beyond its four
cosets.  Class 0 is evaluated on the cosets 0, 2, 4, 6 and on block 0 of coset 1."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, capi, field, stark


def _tables(ctx, orc, main_trace, aux_trace, h, seed):
    rng = np.random.default_rng(seed)
    n = main_trace.shape[1]
    trace_dom = ArithmeticDomain.of_length(n)
    quot = ArithmeticDomain.of_length(8 * n).with_offset(field.generator())
    main = MasterTable(ctx, main_trace, orc.random_elements(rng, (379, h)), trace_dom, quot, quot, 1)
    aux = MasterTable(ctx, aux_trace, orc.random_elements(rng, (91, h, 3)), trace_dom, quot, quot, 3)
    main.maybe_low_degree_extend_all_columns()
    aux.maybe_low_degree_extend_all_columns()
    return main, aux, trace_dom, quot, rng


class _Options:
    """valid-trace mode, parts on one stream (so that the 2048-row quotient domain is split into the classes), the gate at 16 rows"""

    def __init__(self, ctx, valid=True, remainder=True, min_rows=16):
        self.ctx, self.valid, self.remainder, self.min_rows = ctx, valid, remainder, min_rows

    def __enter__(self):
        self.ctx.assume_valid_trace(self.valid)
        self.ctx.air_fork_max_workgroups(0)
        self.ctx.air_remainder_coset(self.remainder, self.min_rows)

    def __exit__(self, *a):
        self.ctx.assume_valid_trace(False)
        self.ctx.air_fork_max_workgroups(256)
        self.ctx.air_remainder_coset(True, 0)


def _valid(ctx, orc):
    from tests import vm_fixture as vf

    main_trace, aux_trace, ch, _ = vf.valid_tables("tiny")
    main, aux, trace_dom, quot, rng = _tables(ctx, orc, main_trace, aux_trace, 3, 3)
    return main, aux, trace_dom, quot, ch, orc.random_elements(rng, (604, 3)), rng


def test_coefficients_evaluate_to_the_codeword(ctx, orc):
    """On the valid 256-row trace: 4N + n1 coefficients, and their values on the quotient domain are the codeword of
    tvm_all_quotients_combined -- which is the oracle's row-by-row evaluation -- word for word."""
    main, aux, trace_dom, quot, ch, weights, _ = _valid(ctx, orc)
    n = len(trace_dom)
    with _Options(ctx):
        codeword = stark.all_quotients_combined(ctx, main, aux, trace_dom, quot, ch, weights).download((len(quot), 3))
        d_coeffs, n_coeffs = stark.all_quotients_coefficients(ctx, main, aux, trace_dom, quot, ch, weights)
    assert n_coeffs == 4 * n + 16
    got = quot.evaluate(ctx, d_coeffs, n_coeffs, 3).download((len(quot), 3))
    assert (got == codeword).all()
    want = orc.quotients_combined(main.low_degree_extended_table(), aux.low_degree_extended_table(),
                                  orc.Domain(trace_dom.offset, trace_dom.generator, trace_dom.length),
                                  orc.Domain(quot.offset, quot.generator, quot.length), ch, weights)
    assert (got == want).all()
    # the quotient has fewer than 4N + 4h - 3 coefficients: the rest of the remainder block is zero
    coeffs = d_coeffs.download((len(quot), 3))[:n_coeffs]
    assert not coeffs[4 * n + 9:].any() and coeffs[4 * n:4 * n + 9].any()
    # the smallest capacity that holds them is accepted, one less is refused
    with _Options(ctx):
        tight, n_tight = stark.all_quotients_coefficients(ctx, main, aux, trace_dom, quot, ch, weights, capacity=n_coeffs)
        assert n_tight == n_coeffs and (tight.download((n_coeffs, 3)) == coeffs).all()
        with pytest.raises(capi.TritonHipError) as refusal:
            stark.all_quotients_coefficients(ctx, main, aux, trace_dom, quot, ch, weights, capacity=n_coeffs - 1)
        assert refusal.value.status == 1                        # TVM_ERR_INVALID_ARGUMENT


def test_segments_from_coefficients_equal_the_segments_of_the_codeword(ctx, orc):
    """the same segment table and the same five polynomials as tvm_quotient_segments on the codeword, onto an LDT domain that is
    the quotient domain and onto a longer one"""
    main, aux, trace_dom, quot, ch, weights, rng = _valid(ctx, orc)
    with _Options(ctx):
        d_codeword = stark.all_quotients_combined(ctx, main, aux, trace_dom, quot, ch, weights)
        d_coeffs, n_coeffs = stark.all_quotients_coefficients(ctx, main, aux, trace_dom, quot, ch, weights)
    randomizer = orc.random_elements(rng, (7, 3))
    for ldt in (quot, ArithmeticDomain.of_length(2 * len(quot)).with_offset(field.generator())):
        poly_len = len(quot) // 4
        want = stark.quotient_segments(ctx, d_codeword, quot, ldt, randomizer, poly_len)
        got = stark.quotient_segments_from_coefficients(ctx, d_coeffs, n_coeffs, ldt, randomizer, poly_len)
        assert (got.polys.download((5, poly_len, 3)) == want.polys.download((5, poly_len, 3))).all()
        assert (got.codewords() == want.codewords()).all()
        assert (got.merkle_tree() == want.merkle_tree()).all()
        got.free()
        want.free()


def test_not_applicable_where_the_gate_is_shut(ctx, orc):
    """TVM_NOT_APPLICABLE, the count zero and the output untouched: without valid-trace mode, with the remainder-coset option off,
    at the default size bound (2^18 rows), with the parts forked (a short quotient domain), and with h = 5 randomizers, whose
    class-1 remainder (18 coefficients) exceeds the block of 16."""
    import ctypes as C

    main, aux, trace_dom, quot, ch, weights, _ = _valid(ctx, orc)
    chh, w = np.ascontiguousarray(ch, np.uint64).reshape(63, 3), np.ascontiguousarray(weights, np.uint64).reshape(604, 3)
    sentinel = np.full((len(quot), 3), 0x5A5A5A5A, np.uint64)

    def refused(m, a):
        out = ctx.to_device(sentinel)
        n = C.c_uint64(77)
        status = ctx.lib.tvm_all_quotients_coefficients(ctx.handle, m._need_table(), a._need_table(), trace_dom.c(), quot.c(),
                                                        chh.ctypes.data, w.ctypes.data, out.ptr, len(quot), C.byref(n))
        return status == stark.NOT_APPLICABLE and n.value == 0 and (out.download((len(quot), 3)) == sentinel).all()

    with _Options(ctx, valid=False):
        assert refused(main, aux)
    with _Options(ctx, remainder=False):
        assert refused(main, aux)
    with _Options(ctx, min_rows=0):
        assert refused(main, aux)
    with _Options(ctx):
        ctx.air_fork_max_workgroups(256)
        assert refused(main, aux)
    from tests import vm_fixture as vf

    main_trace, aux_trace, _, _ = vf.valid_tables("tiny")
    main5, aux5, _, _, _ = _tables(ctx, orc, main_trace, aux_trace, 5, 12)
    with _Options(ctx):
        assert refused(main5, aux5)
        assert stark.all_quotients_coefficients(ctx, main5, aux5, trace_dom, quot, ch, weights) is None
        # ... and the gate open again on the first tables: the context is as usable as before
        assert stark.all_quotients_coefficients(ctx, main, aux, trace_dom, quot, ch, weights)[1] == 4 * len(trace_dom) + 16
