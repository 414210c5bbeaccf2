"""The verifier's batch work outside the revealed rows over the C ABI (csrc/verify_ldt.hip): Merkle inclusion for all trees of a
proof in one call, the FRI collinearity folds, the in-domain answers of a STIR round.  Thin wrappers: host arrays in, host arrays
out; the decisions stay with the caller (triton_vm_amd/host/verifier.cpp is the product caller, the tests are the other)."""
import ctypes as C

import numpy as np


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def merkle_roots(ctx, jobs):
    """jobs: [(n_leaves, leaf indices [q], leaf digests [q][5], authentication structure [a][5])] -> (roots [n][5], flags [n]);
    flags[j] != 0: job j is malformed (its root is all zero)"""
    n = len(jobs)
    keep = [(_h(idx).reshape(-1), _h(leaves).reshape(-1, 5), _h(auth).reshape(-1, 5)) for _, idx, leaves, auth in jobs]
    for idx, leaves, _ in keep:
        if len(idx) != len(leaves):
            raise ValueError("one digest per leaf index")
    sizes = _h([j[0] for j in jobs])
    n_idx, n_auth = _h([len(k[0]) for k in keep]), _h([len(k[2]) for k in keep])
    pointers = lambda which: (C.c_void_p * n)(*[k[which].ctypes.data if k[which].size else None for k in keep])
    p_idx, p_leaves, p_auth = pointers(0), pointers(1), pointers(2)
    roots, flags = np.zeros((n, 5), np.uint64), np.zeros(n, np.uint32)
    ctx._check(ctx.lib.tvm_verifier_merkle_roots(ctx.handle, n, sizes.ctypes.data, n_idx.ctypes.data, p_idx, p_leaves, n_auth.ctypes.data,
                                                 p_auth, roots.ctypes.data, flags.ctypes.data), "tvm_verifier_merkle_roots")
    return roots, flags


def fri_folds(ctx, first_domain, challenges, indices, a_leaves, b_leaves):
    """challenges [rounds][3], indices [q] into first_domain, a_leaves [q][3], b_leaves [rounds][q][3] -> folded values [q][3]"""
    ch, idx, a = _h(challenges).reshape(-1, 3), _h(indices).reshape(-1), _h(a_leaves).reshape(-1, 3)
    b = _h(b_leaves).reshape(len(ch), len(idx), 3)
    if len(a) != len(idx):
        raise ValueError("one A-leaf per index")
    out = np.zeros((len(idx), 3), np.uint64)
    ctx._check(ctx.lib.tvm_verifier_fri_folds(ctx.handle, first_domain.c(), len(ch), ch.ctypes.data, idx.ctypes.data, len(idx),
                                              a.ctypes.data, b.ctypes.data, out.ctypes.data), "tvm_verifier_fri_folds")
    return out


def stir_answers(ctx, values, coset_roots, kth_root, folding_randomness, previous=None):
    """values [q][ff][3], coset_roots [q]; previous: None (the first round) or (quotient set [k][3], answer polynomial [k][3],
    degree-correction randomness [3]) -> the in-domain answers [q][3]"""
    values, roots, r = _h(values), _h(coset_roots).reshape(-1), _h(folding_randomness).reshape(3)
    q, ff = values.shape[0], values.shape[1]
    if values.shape != (q, ff, 3) or len(roots) != q:
        raise ValueError("values [q][ff][3] and one coset root per query")
    out = np.zeros((q, 3), np.uint64)
    if previous is None:
        k, qs, ans, rc = 0, None, None, None
    else:
        qs, ans, rc = _h(previous[0]).reshape(-1, 3), _h(previous[1]).reshape(-1, 3), _h(previous[2]).reshape(3)
        k = len(qs)
        if len(ans) != k:
            raise ValueError("the answer polynomial has as many coefficients as the quotient set has points")
    ptr = lambda a: None if a is None else a.ctypes.data
    ctx._check(ctx.lib.tvm_verifier_stir_answers(ctx.handle, ff, q, values.ctypes.data, roots.ctypes.data, int(kth_root), r.ctypes.data, k,
                                                 ptr(qs), ptr(ans), ptr(rc), out.ctypes.data), "tvm_verifier_stir_answers")
    return out
