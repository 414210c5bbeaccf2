"""The rounds of a STIR proof with the transcript on the device, over the C ABI (csrc/stir_rounds.hip: tvm_stir_prove_rounds).  A thin
wrapper: host arrays in, host arrays out (the C++ host's Stir::prove is the product caller under TVMH_OPTION_DEVICE_STIR, the tests
are the other; low_degree_test.Stir.prove is the same prover with the host in the loop)."""
import ctypes as C

import numpy as np

NOT_APPLICABLE = 5  # TVM_NOT_APPLICABLE
MAX_INDICES = 1024  # TVM_TAIL_MAX_INDICES: in-domain queries of a round
MAX_QUOTIENT_SET = 256  # in-domain plus out-of-domain queries of a full round (the one-workgroup interpolation)


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def prove_rounds(ctx, sponge_state, d_codeword, stir):
    """tvm_stir_prove_rounds for the instance `stir` (low_degree_test.Stir) on the codeword d_codeword (a DeviceBuffer or a pointer),
    from the sponge state [16].
    -> dict(state, roots [R + 1][5], folding_randomness [R + 1][3], ood_queries / ood_values: per full round [n_ood][3],
    degree_correction_randomness [R][3], queried_indices / folded_queried: per tree the sampled indices and those mod the folded
    domain's length without repeats, final_polynomial [n][3], directory [2 (R + 1)][2], payloads: per tree (stacked leaves, authentication
    structure) as flat word arrays, words), or None where the entry point does not apply (nothing was written)"""
    ptr = lambda b: getattr(b, "ptr", b)
    rounds = _h(stir.round_queries).reshape(-1, 2)
    R, ff, dom = len(rounds), stir.folding_factor, stir.initial_domain
    queries = [int(q) for q in rounds[:, 0]] + [stir.final_num_in_domain_queries]
    n_ood = [int(q) for q in rounds[:, 1]]
    n_final = dom.length // ff ** (R + 1)
    state, after = _h(sponge_state).reshape(16), np.zeros(16, np.uint64)
    roots, scalars = np.zeros((R + 1, 5), np.uint64), np.zeros((2 * R + 1 + sum(n_ood), 3), np.uint64)
    ood_values = np.zeros((max(sum(n_ood), 1), 3), np.uint64)
    indices, unique, counts = np.zeros(sum(queries), np.uint64), np.zeros(sum(queries), np.uint64), np.zeros(R + 1, np.uint64)
    final, directory = np.zeros((max(n_final, 1), 3), np.uint64), np.zeros((2 * (R + 1), 2), np.uint64)
    capacity = ctx.lib.tvm_stir_prove_rounds_payload_bound(dom.c(), ff, R, rounds.ctypes.data, queries[-1])
    payload, words = np.zeros(max(capacity, 1), np.uint64), C.c_uint64(0)
    status = ctx.lib.tvm_stir_prove_rounds(ctx.handle, state.ctypes.data, ptr(d_codeword), dom.c(), ff, R, rounds.ctypes.data, queries[-1],
                                           stir.final_degree, after.ctypes.data, roots.ctypes.data, scalars.ctypes.data, ood_values.ctypes.data,
                                           indices.ctypes.data, unique.ctypes.data, counts.ctypes.data, final.ctypes.data, directory.ctypes.data,
                                           payload.ctypes.data, capacity, C.byref(words))
    if status == NOT_APPLICABLE:
        return None
    ctx._check(status, "tvm_stir_prove_rounds")
    out = dict(state=after, roots=roots, folding_randomness=[], ood_queries=[], ood_values=[], degree_correction_randomness=[],
               queried_indices=[], folded_queried=[], final_polynomial=final[:n_final], directory=directory, words=int(words.value),
               payloads=[payload[int(o):int(o) + int(w)].copy() for o, w in directory])
    at, at_ood, at_q = 0, 0, 0
    for r in range(R + 1):
        out["folding_randomness"].append(scalars[at])
        at += 1
        if r < R:
            out["ood_queries"].append(scalars[at:at + n_ood[r]])
            out["ood_values"].append(ood_values[at_ood:at_ood + n_ood[r]])
            out["degree_correction_randomness"].append(scalars[at + n_ood[r]])
            at, at_ood = at + n_ood[r] + 1, at_ood + n_ood[r]
        out["queried_indices"].append([int(i) for i in indices[at_q:at_q + queries[r]]])
        out["folded_queried"].append([int(i) for i in unique[at_q:at_q + int(counts[r])]])
        at_q += queries[r]
    return out
