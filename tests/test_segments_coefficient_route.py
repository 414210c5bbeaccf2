"""The quotient-segment table from the segments' coefficients (csrc/capi.hip: quotient_segments_of_coefficients; csrc/ntt.hip:
lde_coefficient_form): a segment of n + h coefficients, n a power of two and h <= n, is (lo + hi) + (X^n - 1) hi -- an interpolant
of n coefficients plus zerofier times randomizer.  One relayout pass writes lo + hi in the library's coefficient form and hi as the
randomizers, and the table extension runs its forward half alone (TVM_LDE_FORWARD_ONLY).  TVM_OPTION_SEGMENTS_FROM_COEFFICIENTS = 0
restores the route through the values on the roots of unity.

The relayout has no entry point of its own, so its output is checked through the pass that reads it: the forward half of the extension
is an injective linear map of (interpolant, randomizer) while n + h does not exceed the domain, and every word is canonical, so equal
tables mean equal coefficient forms and equal randomizers."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field, stark

P = np.uint64(field.P)
HEIGHTS = {4: "generic", 13: "v3", 16: "fused<8>", 18: "fused<9>", 19: "fused<10>"}   # log2 n -> the family of pass 2 (csrc/lde_plan.h)


def odom(orc, d):
    return orc.Domain(d.offset, d.generator, d.length)


def n1_of(log_n):
    return 1 << (log_n // 2)   # csrc/ntt.hip: split_for


def field_add(a, b):
    s = a + b   # (wraps: a + b < 2p < 2^65)
    return np.where((s < a) | (s >= P), s - P, s)


def segments_of(ctx, rng, orc, n_coeffs, n_rand, ldt, poly_len):
    q = orc.random_elements(rng, (n_coeffs, 3))
    rnd = orc.random_elements(rng, (n_rand, 3))
    qs = stark.quotient_segments_from_coefficients(ctx, ctx.to_device(q), n_coeffs, ldt, rnd, poly_len)
    return q, rnd, qs


@pytest.fixture
def old_route(ctx, request):
    """switches the module's context to the route through the values; the default comes back after the test"""
    request.addfinalizer(lambda: ctx.segments_from_coefficients(True))
    return lambda on=True: ctx.segments_from_coefficients(not on)


@pytest.mark.parametrize("h_kind", ["0", "1", "n1"])
@pytest.mark.parametrize("log_n", sorted(HEIGHTS))
def test_relayout_is_the_inverse_half_of_the_extension(ctx, orc, log_n, h_kind):
    """Five random polynomials of n + h coefficients over the extension field (the randomized segments of a random quotient with a
    randomizer of n + h coefficients).  Reference: the values of lo + hi on the n-th roots of unity through tvm_lde_column_coefficients
    (TVM_LDE_INVERSE_ONLY: the coefficient form) and from there, with hi as the randomizers, through tvm_lde_table_add_columns -- the
    same forward half the segment route runs on what the relayout wrote.  The two tables must agree word for word."""
    if log_n > 13 and ctx.kind == "emu":
        pytest.skip("CPU suite time: the 256-, 512- and 1024-point axes run on the GPU")
    n, h = 1 << log_n, {"0": 0, "1": 1, "n1": n1_of(log_n)}[h_kind]
    rng = np.random.default_rng(1000 * log_n + h)
    ldt = ArithmeticDomain.of_length(2 * n).with_offset(field.generator())
    _, _, qs = segments_of(ctx, rng, orc, 4 * (n + h), n + h, ldt, n + h)
    polys = qs.polys.download((5, n + h, 3))
    got = qs.codewords()
    qs.free()
    lo, hi = polys[:, :n], polys[:, n:]
    assert not h or all(hi[k].any() for k in range(5))
    folded = lo.copy()
    folded[:, :h] = field_add(lo[:, :h], hi)
    trace_dom = ArithmeticDomain.of_length(n)
    values = np.stack([trace_dom.evaluate(ctx, ctx.to_device(folded[k]), n, 3).download((n, 3)) for k in range(5)])
    mt = MasterTable(ctx, values, np.ascontiguousarray(hi), trace_dom, ldt, ldt, 3)
    mt.low_degree_extend_by_column_blocks(1)
    want = mt.low_degree_extended_table()
    mt.clear_cache()
    assert (got == want).all()


def check_against_oracle(ctx, orc, rng, n_coeffs, n_rand, log_ldt, poly_len):
    ldt = ArithmeticDomain.of_length(1 << log_ldt).with_offset(field.generator())
    q, rnd, qs = segments_of(ctx, rng, orc, n_coeffs, n_rand, ldt, poly_len)
    seg_len = (n_coeffs + 3) // 4
    padded = np.zeros((4 * seg_len, 3), np.uint64)
    padded[:n_coeffs] = q
    seg = np.ascontiguousarray(padded.reshape(seg_len, 4, 3).transpose(1, 0, 2))
    want_polys, want_cws = orc.randomize_quotient_segments(seg, rnd, odom(orc, ldt), poly_len)
    assert (qs.polys.download((5, poly_len, 3)) == want_polys).all()
    assert (qs.codewords() == want_cws).all()
    digests = orc.hash_rows(want_cws.reshape(len(ldt), 15))
    assert (qs.merkle_tree()[1] == orc.merkle_tree(digests)[1]).all()
    w = orc.random_elements(rng, (5, 3))
    got = qs.linear_combination(w).download((len(ldt), 3))
    rows = range(len(ldt)) if len(ldt) <= 256 else [0, 1, len(ldt) - 1] + [int(i) for i in rng.integers(0, len(ldt), 61)]
    for i in rows:
        acc = np.zeros(3, np.uint64)
        for k in range(5):
            acc = orc.xfe_add(acc, orc.xfe_mul(want_cws[i, k], w[k]))
        assert (got[i] == acc).all(), i
    qs.free()


@pytest.mark.parametrize("h_kind", ["0", "1", "n1", "n1+1"])
@pytest.mark.parametrize("log_n,log_ldt", [(4, 6), (8, 10), (13, 15), (16, 18)])
def test_segments_against_the_oracle(ctx, orc, log_n, log_ldt, h_kind):
    """A quotient of 4 (n + h) coefficients and a randomizer of h: segments of n + h coefficients, polynomials, codewords, Merkle root
    and one linear combination against the oracle.  h = n1 + 1 is the first randomizer count that the row kernels of pass 2 do not take
    (the plan falls to the tile kernel)."""
    if log_n > 8 and ctx.kind == "emu":
        pytest.skip("CPU suite time: the longer axes run on the GPU")
    n, h = 1 << log_n, {"0": 0, "1": 1, "n1": n1_of(log_n), "n1+1": n1_of(log_n) + 1}[h_kind]
    check_against_oracle(ctx, orc, np.random.default_rng(77 * log_n + h), 4 * (n + h), h, log_ldt, n + h)


@pytest.mark.parametrize("n_coeffs,n_rand,log_ldt,poly_len", [
    (64, 40, 7, 40),     # poly_len > 2 n for n = n_coeffs / 4: the split is made at the largest power of two in the length (32 + 8)
    (128, 32, 5, 32),    # more coefficients than points (a rank's share of the domain): folded first, then through the values
    (64, 0, 4, 16),      # one coset only: through the values
    (256, 7, 12, 100),   # 64 times as many points as coefficients, above the extension's 32 cosets: through the values
    (20, 3, 6, 9),       # fewer than 16 coefficients: padded to the shortest table axis
    (256, 7, 11, 100),   # poly_len beyond the coefficients there are: zero from 64 on, the split is 64 + 0
])
def test_segments_at_the_edges_of_the_split(ctx, orc, n_coeffs, n_rand, log_ldt, poly_len):
    """where the split does not apply (the route through the values runs as before) and where it applies in another shape than
    n_coeffs / 4 + n_rand"""
    check_against_oracle(ctx, orc, np.random.default_rng(n_coeffs + n_rand), n_coeffs, n_rand, log_ldt, poly_len)


def test_both_routes_agree_at_2p19(ctx, orc, old_route):
    """n = 2^19, L = 2^22: the smallest height whose pass 2 is k_lde_pass2_fused<10>, forward only -- codewords and tree root with the
    option off and on, word for word"""
    if ctx.kind == "emu":
        pytest.skip("CPU suite time: 2^22 rows run on the GPU")
    n, h = 1 << 19, n1_of(19)
    ldt = ArithmeticDomain.of_length(1 << 22).with_offset(field.generator())
    q = orc.random_elements(np.random.default_rng(19), (4 * (n + h), 3))
    rnd = orc.random_elements(np.random.default_rng(20), (h, 3))
    d_q = ctx.to_device(q)
    results = []
    for old in (True, False):
        old_route(old)
        qs = stark.quotient_segments_from_coefficients(ctx, d_q, len(q), ldt, rnd, n + h)
        results.append((qs.codewords(), qs.merkle_tree()[1].copy()))
        qs.free()
    assert (results[0][1] == results[1][1]).all()
    assert (results[0][0] == results[1][0]).all()


@pytest.mark.parametrize("log_n,log_ldt,h", [(4, 6, 3), (8, 11, 17), (6, 7, 63)])
def test_both_routes_agree_on_small_tables(ctx, orc, old_route, log_n, log_ldt, h):
    """the same at sizes the CPU emulation runs, h = n - 1 (the longest randomizer part) among them"""
    n = 1 << log_n
    ldt = ArithmeticDomain.of_length(1 << log_ldt).with_offset(field.generator())
    q = orc.random_elements(np.random.default_rng(log_n), (4 * (n + h) - 1, 3))
    rnd = orc.random_elements(np.random.default_rng(h), (n + h, 3))
    d_q = ctx.to_device(q)
    results = []
    for old in (True, False):
        old_route(old)
        qs = stark.quotient_segments_from_coefficients(ctx, d_q, len(q), ldt, rnd, n + h)
        results.append((qs.codewords(), qs.merkle_tree()[1].copy(), qs.polys.download((5, n + h, 3))))
        qs.free()
    for a, b in zip(*results):
        assert (a == b).all()
