"""The verifier's device work for many proofs per call (csrc/verify_batch.hip): every batched entry point against its one-group
counterpart called once per group, on seeded random canonical words.  All comparisons are exact."""
import ctypes as C

import numpy as np

from triton_vm_amd import field, stark
from triton_vm_amd.arithmetic_domain import ArithmeticDomain
from triton_vm_amd.capi import Domain
from triton_vm_amd.verifier import deep_values
from triton_vm_amd.verifier_ldt import fri_folds, stir_answers

NOT_APPLICABLE = 5
MAX_LAST_CODEWORD = 1024   # TVM_VERIFIER_MAX_LAST_CODEWORD
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)


def words(rng, *shape):
    return np.ascontiguousarray(rng.integers(0, field.P, size=shape, dtype=np.uint64))


def pointers(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data if a is not None and a.size else None for a in arrays])


def u64s(values):
    return np.ascontiguousarray(values, dtype=np.uint64)


def domain(rng, log2_length):
    return ArithmeticDomain.of_length(1 << log2_length).with_offset(int(words(rng, 1)[0]) or field.ONE)


# ---------------------------------------------------------------------------------------------------------------- FRI folds
def fri_group(rng, rounds, checks, log2_length):
    dom = domain(rng, log2_length)
    return dict(dom=dom, ch=words(rng, rounds, 3), idx=u64s(rng.integers(0, dom.length, checks)), a=words(rng, checks, 3),
                b=words(rng, rounds, checks, 3))


def fri_folds_batch(ctx, groups):
    n = len(groups)
    doms = (Domain * n)(*[g["dom"].c() for g in groups])
    rounds = np.ascontiguousarray([len(g["ch"]) for g in groups], dtype=np.uint32)
    checks = u64s([len(g["idx"]) for g in groups])
    out = [np.full((len(g["idx"]), 3), SENTINEL) for g in groups]
    flags = np.full(n, 77, np.uint32)
    rc = ctx.lib.tvm_verifier_fri_folds_batch(ctx.handle, n, C.addressof(doms), rounds.ctypes.data, checks.ctypes.data,
                                              pointers([g["ch"] for g in groups]), pointers([g["idx"] for g in groups]),
                                              pointers([g["a"] for g in groups]), pointers([g["b"] for g in groups]), pointers(out),
                                              flags.ctypes.data)
    assert rc == 0
    return out, flags


def test_fri_folds_of_many_groups_are_the_folds_of_each(ctx):
    """group boundaries inside a wavefront (1, 2, 65), on one (64, 130 + 126 = 256) and across workgroups"""
    rng = np.random.default_rng(31)
    shapes = [(0, 1, 3), (1, 1, 1), (3, 63, 9), (5, 65, 11), (2, 256, 7), (7, 300, 12)]
    groups = [fri_group(rng, r, q, lg) for r, q, lg in shapes]
    want = [fri_folds(ctx, g["dom"], g["ch"], g["idx"], g["a"], g["b"]) for g in groups]
    got, flags = fri_folds_batch(ctx, groups)
    assert not flags.any()
    for g, (w, o) in enumerate(zip(want, got)):
        assert np.array_equal(w, o), shapes[g]
    for g in (0, 5):   # one group alone
        got, flags = fri_folds_batch(ctx, [groups[g]])
        assert not flags.any() and np.array_equal(got[0], want[g])
    # a malformed group (an index outside its domain) between two good ones: flagged, nothing written, the others as before
    bad = dict(groups[2], idx=groups[2]["idx"].copy())
    bad["idx"][5] = bad["dom"].length
    got, flags = fri_folds_batch(ctx, [groups[3], bad, groups[4]])
    assert list(flags) == [0, 1, 0] and (got[1] == SENTINEL).all()
    assert np.array_equal(got[0], want[3]) and np.array_equal(got[2], want[4])


# ---------------------------------------------------------------------------------------------------------------- FRI last rounds
def last_round_reference(ctx, codeword, x):
    """tvm_codeword_merkle_tree's root; tvm_interpolate + tvm_evaluate_at_points over ArithmeticDomain::of_length"""
    length = len(codeword)
    d_cw = ctx.alloc(3 * length).upload(codeword)
    root = stark.merkle_root(ctx, stark.merkle_tree_from_codeword(ctx, d_cw, length))
    coeffs = ArithmeticDomain.of_length(length).interpolate(ctx, d_cw, 3)
    return root, stark.evaluate_at_points(ctx, coeffs, length, x)[0]


def test_fri_last_rounds_give_the_root_and_the_value_of_the_three_calls(ctx):
    rng = np.random.default_rng(32)
    lengths = [1, 2, 64, MAX_LAST_CODEWORD, 2 * MAX_LAST_CODEWORD, 64, 8]
    codewords = [words(rng, n, 3) for n in lengths]
    points = words(rng, len(lengths), 3)
    points[5, 1:] = 0                                                  # a base-field point in the extension
    points[6] = (field.primitive_root_of_unity(8), 0, 0)               # ... and one that is a point of the domain
    roots, values = np.full((len(lengths), 5), SENTINEL), np.full((len(lengths), 3), SENTINEL)
    flags = np.full(len(lengths), 77, np.uint32)
    rc = ctx.lib.tvm_verifier_fri_last_rounds(ctx.handle, len(lengths), u64s(lengths).ctypes.data, pointers(codewords), points.ctypes.data,
                                              roots.ctypes.data, values.ctypes.data, flags.ctypes.data)
    assert rc == 0
    assert list(flags) == [0, 0, 0, 0, NOT_APPLICABLE, 0, 0]
    assert (roots[4] == SENTINEL).all() and (values[4] == SENTINEL).all()      # beyond the bound: nothing written
    for g, n in enumerate(lengths):
        if flags[g]:
            continue
        root, value = last_round_reference(ctx, codewords[g], points[g])
        assert np.array_equal(roots[g], root), n
        assert np.array_equal(values[g], value), n
    assert np.array_equal(values[6], codewords[6][1])


# ---------------------------------------------------------------------------------------------------------------- interpolation
def interpolate_batch(ctx, groups):
    n = len(groups)
    k = np.ascontiguousarray([len(p) for p, _ in groups], dtype=np.uint32)
    out = [np.full((len(p), 3), SENTINEL) for p, _ in groups]
    flags = np.full(n, 77, np.uint32)
    rc = ctx.lib.tvm_xfe_interpolate_batch(ctx.handle, n, k.ctypes.data, pointers([p for p, _ in groups]), pointers([v for _, v in groups]),
                                           pointers(out), flags.ctypes.data)
    assert rc == 0
    return out, flags


def quotient_set_like(rng, k):
    """k pairwise distinct points, all but two in the base field, as a STIR quotient set has them"""
    points = np.zeros((k, 3), np.uint64)
    points[:, 0] = [i * 0x9E3779B97F4A7C15 % field.P for i in range(1, k + 1)]   # (distinct: the factor is invertible)
    points[max(k - 2, 0):] = words(rng, k - max(k - 2, 0), 3)
    return points


def test_interpolations_of_many_groups_are_the_interpolation_of_each(ctx):
    rng = np.random.default_rng(33)
    groups = [(quotient_set_like(rng, k), words(rng, k, 3)) for k in (1, 2, 255, 256)]
    repeated = (quotient_set_like(rng, 40), words(rng, 40, 3))
    repeated[0][17] = repeated[0][3]
    groups = groups[:2] + [repeated] + groups[2:] + [(words(rng, 257, 3), words(rng, 257, 3)), (words(rng, 0, 3), words(rng, 0, 3))]
    got, flags = interpolate_batch(ctx, groups)
    assert list(flags) == [0, 0, 1, 0, 0, NOT_APPLICABLE, 0]
    assert (got[2] == SENTINEL).all() and (got[5] == SENTINEL).all()
    for g in (0, 1, 3, 4):   # the neighbours of the flagged group among them
        points, values = groups[g]
        want = np.zeros((len(points), 3), np.uint64)
        assert ctx.lib.tvm_xfe_interpolate(ctx.handle, points.ctypes.data, values.ctypes.data, len(points), want.ctypes.data) == 0
        assert np.array_equal(got[g], want), len(points)
    assert ctx.lib.tvm_xfe_interpolate(ctx.handle, repeated[0].ctypes.data, repeated[1].ctypes.data, 40, np.zeros((40, 3), np.uint64).ctypes.data) != 0


# ---------------------------------------------------------------------------------------------------------------- STIR answers
def stir_group(rng, ff, k, queries, log2_length=10, rc=None):
    dom = domain(rng, log2_length)
    folded = dom.length // ff
    idx = rng.integers(0, folded, queries)
    roots = u64s([field.mont_mul(field.mont_pow(dom.generator, int(i)), dom.offset) for i in idx])
    previous = None
    if k:
        previous = (quotient_set_like(rng, k), words(rng, k, 3), words(rng, 3) if rc is None else rc(roots))
    return dict(values=words(rng, queries, ff, 3), roots=roots, kth_root=field.mont_pow(dom.generator, folded), r=words(rng, 3), previous=previous)


def stir_answers_batch(ctx, groups):
    n = len(groups)
    ff = np.ascontiguousarray([g["values"].shape[1] for g in groups], dtype=np.uint32)
    kth = u64s([g["kth_root"] for g in groups])
    r = u64s([g["r"] for g in groups])
    k = np.ascontiguousarray([len(g["previous"][0]) if g["previous"] else 0 for g in groups], dtype=np.uint32)
    rc = u64s([g["previous"][2] if g["previous"] else [0, 0, 0] for g in groups])
    queries = u64s([len(g["roots"]) for g in groups])
    out = [np.full((len(g["roots"]), 3), SENTINEL) for g in groups]
    flags = np.full(n, 77, np.uint32)
    status = ctx.lib.tvm_verifier_stir_answers_batch(
        ctx.handle, n, ff.ctypes.data, kth.ctypes.data, r.ctypes.data, k.ctypes.data,
        pointers([g["previous"][0] if g["previous"] else None for g in groups]),
        pointers([g["previous"][1] if g["previous"] else None for g in groups]), rc.ctypes.data, queries.ctypes.data,
        pointers([g["values"] for g in groups]), pointers([g["roots"] for g in groups]), pointers(out), flags.ctypes.data)
    assert status == 0
    return out, flags


def test_stir_answers_of_many_groups_are_the_answers_of_each(ctx):
    rng = np.random.default_rng(34)

    def inverse_of_a_coset_point(roots):   # rc x = 1 at the first point of the first query's coset: the degree correction's other branch
        return u64s([field.mont_inv(int(roots[0])), 0, 0])

    groups = [stir_group(rng, 4, 0, 70), stir_group(rng, 2, 1, 1), stir_group(rng, 16, 200, 70, log2_length=12),
              stir_group(rng, 4, 300, 1), stir_group(rng, 16, 0, 1), stir_group(rng, 4, 7, 3, rc=inverse_of_a_coset_point),
              stir_group(rng, 2, 200, 5)]
    want = [stir_answers(ctx, g["values"], g["roots"], g["kth_root"], g["r"], g["previous"]) for g in groups]
    got, flags = stir_answers_batch(ctx, groups)
    assert not flags.any()
    for g, (w, o) in enumerate(zip(want, got)):
        assert np.array_equal(w, o), g
    # the rc x = 1 branch was taken: another randomness gives another answer for that query only through that branch
    other = dict(groups[5], previous=(groups[5]["previous"][0], groups[5]["previous"][1], words(rng, 3)))
    assert not np.array_equal(stir_answers_batch(ctx, [other])[0][0][0], want[5][0])
    # a malformed group (a folding factor above 16) flags that group only
    bad = dict(groups[0], values=words(rng, 2, 17, 3), roots=groups[0]["roots"][:2])
    got, flags = stir_answers_batch(ctx, [groups[1], bad, groups[3]])
    assert list(flags) == [0, 1, 0] and (got[1] == SENTINEL).all()
    assert np.array_equal(got[0], want[1]) and np.array_equal(got[2], want[3])


# ---------------------------------------------------------------------------------------------------------------- DEEP values
def deep_group(rng, rows, log2_length):
    dom = domain(rng, log2_length)
    return dict(dom=dom, main=words(rng, rows, 379), aux=words(rng, rows, 91, 3), quot=words(rng, rows, 5, 3),
                idx=u64s(rng.integers(0, dom.length, rows)), w_ma=words(rng, 470, 3), w_q=words(rng, 5, 3), w_d=words(rng, 4, 3),
                points=words(rng, 4, 3), values=words(rng, 4, 3))


def deep_values_batch(ctx, groups):
    n = len(groups)
    doms = (Domain * n)(*[g["dom"].c() for g in groups])
    flat = lambda key: u64s(np.concatenate([g[key].reshape(-1) for g in groups]))
    w_q, w_d, points, values = flat("w_q"), flat("w_d"), flat("points"), flat("values")
    rows = u64s([len(g["idx"]) for g in groups])
    out = [np.full((len(g["idx"]), 3), SENTINEL) for g in groups]
    flags = np.full(n, 77, np.uint32)
    rc = ctx.lib.tvm_verifier_deep_values_batch(ctx.handle, n, C.addressof(doms), pointers([g["w_ma"] for g in groups]), w_q.ctypes.data,
                                                w_d.ctypes.data, points.ctypes.data, values.ctypes.data, rows.ctypes.data,
                                                pointers([g["main"] for g in groups]), pointers([g["aux"] for g in groups]),
                                                pointers([g["quot"] for g in groups]), pointers([g["idx"] for g in groups]), pointers(out),
                                                flags.ctypes.data)
    assert rc == 0
    return out, flags


def test_deep_values_of_many_groups_are_the_deep_values_of_each(ctx):
    rng = np.random.default_rng(35)
    groups = [deep_group(rng, 1, 5), deep_group(rng, 5, 11), deep_group(rng, 64, 14)]
    want = [deep_values(ctx, g["main"], g["aux"], g["quot"], g["idx"], g["dom"], g["w_ma"], g["w_q"], g["w_d"], g["points"], g["values"])
            for g in groups]
    got, flags = deep_values_batch(ctx, groups)
    assert not flags.any()
    for w, o in zip(want, got):
        assert np.array_equal(w, o)
    bad = dict(groups[1], idx=groups[1]["idx"].copy())
    bad["idx"][0] = bad["dom"].length
    got, flags = deep_values_batch(ctx, [groups[2], bad, groups[0]])
    assert list(flags) == [0, 1, 0] and (got[1] == SENTINEL).all()
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[2], want[0])


def test_null_arguments_are_an_error_status_and_no_group_is_no_work(ctx):
    flags = np.zeros(1, np.uint32)
    assert ctx.lib.tvm_xfe_interpolate_batch(ctx.handle, 1, None, None, None, None, flags.ctypes.data) == 1
    assert ctx.lib.tvm_verifier_fri_last_rounds(ctx.handle, 0, None, None, None, None, None, None) == 1
