"""Valid-trace mode with one coset fewer per class of constraints (csrc/capi.hip: quotients_by_remainder_coset): class 1 on three
cosets of the trace domain, class 3 on two, class 2 on one, each plus one block T of 16 rows of coset 6 that pays for the few
coefficients beyond the whole cosets.  The gate is lowered to the 256-row trace through TVM_OPTION_AIR_REMAINDER_MIN_ROWS.

With h trace randomizers the classes' quotients have at most 4h - 2, 3h - 1 and 2h coefficients beyond their whole cosets: h = 3
fits a block of n1 = 16 rows, h = 5 (18 for class 1) does not, and the gate falls back to the whole cosets."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field, stark


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


def _quotients(ctx, main, aux, trace_dom, quot, challenges, weights, remainder, min_rows=16):
    """valid-trace mode, parts on one stream (so that the 2048-row quotient domain is split into the classes)"""
    ctx.assume_valid_trace(True)
    ctx.air_fork_max_workgroups(0)
    ctx.air_remainder_coset(remainder, min_rows)
    try:
        return stark.all_quotients_combined(ctx, main, aux, trace_dom, quot, challenges, weights).download((len(quot), 3))
    finally:
        ctx.assume_valid_trace(False)
        ctx.air_fork_max_workgroups(256)
        ctx.air_remainder_coset(True, 0)


def _t_rows(n):
    """the domain rows of T: block 0 of coset 6 -- rows j = n2 * j2 of the trace domain, j2 < n1 (context.h)"""
    log_n = n.bit_length() - 1
    n1, n2 = 1 << (log_n // 2), 1 << (log_n - log_n // 2)
    return 8 * n2 * np.arange(n1) + 6


def test_remainder_coset_is_exact_on_a_valid_trace(ctx, orc):
    """On the valid 256-row trace of a real execution the codeword equals the oracle's row-by-row evaluation bit for bit, and the
    whole-coset split's.  The polynomial the new path assembles has fewer than 4N coefficients and agrees with the true quotients on
    all 8N points, so it IS them: in particular B's coefficients s .. M-1 (V B = q - R) are zero."""
    from tests import vm_fixture as vf

    main_trace, aux_trace, ch, _ = vf.valid_tables("tiny")
    main, aux, trace_dom, quot, rng = _tables(ctx, orc, main_trace, aux_trace, 3, 3)
    weights = orc.random_elements(rng, (604, 3))
    got = _quotients(ctx, main, aux, trace_dom, quot, ch, weights, True)
    old = _quotients(ctx, main, aux, trace_dom, quot, ch, weights, False)
    want = orc.quotients_combined(main.low_degree_extended_table(), aux.low_degree_extended_table(),
                                  orc.Domain(trace_dom.offset, trace_dom.generator, trace_dom.length),
                                  orc.Domain(quot.offset, quot.generator, quot.length), ch, weights)
    assert (got == want).all()
    assert (old == want).all()


def test_remainder_coset_path_and_its_switches(ctx, orc):
    """On random tables the quotients are rational functions, so which rows come out exact tells the paths apart.  The new path
    evaluates every class on coset 0 and on T only: those rows agree with the row-by-row values, coset 4 (where the whole-coset
    split evaluates class 2 and class 3) does not.  TVM_OPTION_AIR_REMAINDER_COSET = 0, or the default size bound (2^18 rows),
    restores the whole-coset split word for word; so does h = 5, whose class-1 remainder (18 coefficients) exceeds the block."""
    rng = np.random.default_rng(11)
    n = 256
    main_trace, aux_trace = orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3))
    challenges, weights = orc.random_elements(rng, (63, 3)), orc.random_elements(rng, (604, 3))
    main, aux, trace_dom, quot, _ = _tables(ctx, orc, main_trace, aux_trace, 3, 12)
    new = _quotients(ctx, main, aux, trace_dom, quot, challenges, weights, True)
    off = _quotients(ctx, main, aux, trace_dom, quot, challenges, weights, False)
    default_bound = _quotients(ctx, main, aux, trace_dom, quot, challenges, weights, True, min_rows=0)
    want = orc.quotients_combined(main.low_degree_extended_table(), aux.low_degree_extended_table(),
                                  orc.Domain(trace_dom.offset, trace_dom.generator, trace_dom.length),
                                  orc.Domain(quot.offset, quot.generator, quot.length), challenges, weights)
    t = _t_rows(n)
    assert (new[0::8] == want[0::8]).all() and (new[t] == want[t]).all()
    assert (new[4::8] != want[4::8]).any(axis=1).all()
    assert (off[0::4] == want[0::4]).all()                 # the whole-coset split (tests/test_kernels_air.py)
    assert (off == default_bound).all() and (off != new).any()
    # h = 5: class 1 has 4h - 2 = 18 > 16 coefficients beyond its three cosets -> the gate falls back
    main5, aux5, _, _, _ = _tables(ctx, orc, main_trace, aux_trace, 5, 12)
    on5 = _quotients(ctx, main5, aux5, trace_dom, quot, challenges, weights, True)
    off5 = _quotients(ctx, main5, aux5, trace_dom, quot, challenges, weights, False)
    assert (on5 == off5).all()
