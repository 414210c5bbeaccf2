"""The tail of a proof with the transcript on the device, over the C ABI (csrc/proof_tail.hip): Tip5::sample_indices from a sponge
state, the authentication structures of many trees in one launch, and everything of a FRI proof behind the commit phase together
with the trace openings.  Thin wrappers: host arrays in, host arrays out (the C++ host's ProofSteps::fri is the product caller
under TVMH_OPTION_DEVICE_TAIL, the tests are the other)."""
import ctypes as C

import numpy as np

NOT_APPLICABLE = 5  # TVM_NOT_APPLICABLE
MAX_INDICES = 1024  # TVM_TAIL_MAX_INDICES


def _h(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def sponge_sample_indices(ctx, state, upper_bound, n):
    """tvm_sponge_sample_indices: state [16] (Montgomery words) -> (n indices below upper_bound, the state afterwards)"""
    state = _h(state).reshape(16)
    indices, after = np.zeros(max(n, 1), np.uint64), np.zeros(16, np.uint64)
    ctx._check(ctx.lib.tvm_sponge_sample_indices(ctx.handle, state.ctypes.data, upper_bound, n, indices.ctypes.data, after.ctypes.data),
               "tvm_sponge_sample_indices")
    return indices[:n], after


def authentication_structures(ctx, jobs):
    """jobs: [(n_leaves, leaf indices, the tree's device node array -- a DeviceBuffer, a pointer or None)] ->
    [(heap indices of the authentication structure in descending order, their digests [k][5] or None)], or None where the entry
    point does not apply (a job with more than MAX_INDICES indices; nothing was computed)"""
    n = len(jobs)
    idx = [_h(j[1]).reshape(-1) for j in jobs]
    sizes, counts = _h([j[0] for j in jobs]), _h([len(i) for i in idx])
    ptr = lambda b: getattr(b, "ptr", b)
    room = [min(len(i), int(s)) * (int(s).bit_length() - 1) for i, s in zip(idx, sizes)]
    out_idx = [np.zeros(max(r, 1), np.uint64) for r in room]
    out_nodes = [np.zeros((max(r, 1), 5), np.uint64) if j[2] is not None else None for r, j in zip(room, jobs)]
    pointers = lambda arrays: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrays])
    p_idx, p_out_idx, p_out_nodes = pointers(idx), pointers(out_idx), pointers(out_nodes)
    p_nodes = (C.c_void_p * n)(*[ptr(j[2]) for j in jobs])
    n_out = np.zeros(n, np.uint64)
    status = ctx.lib.tvm_authentication_structures(ctx.handle, n, sizes.ctypes.data, p_idx, counts.ctypes.data, p_nodes, p_out_idx, p_out_nodes,
                                                   n_out.ctypes.data)
    if status == NOT_APPLICABLE:
        return None
    ctx._check(status, "tvm_authentication_structures")
    return [(out_idx[j][:int(n_out[j])], None if out_nodes[j] is None else out_nodes[j][:int(n_out[j])]) for j in range(n)]


def tail_items(n_rounds):
    """TVM_TAIL_ITEMS: the number of payloads tvm_fri_query_and_open writes"""
    return 2 * (n_rounds + 1 if n_rounds else 1) + 6


def fri_query_and_open(ctx, sponge_state, d_codeword, domain, d_codewords, d_nodes, n_checks, tables, d_table_nodes):
    """tvm_fri_query_and_open.  d_codeword: round 0's codeword; d_codewords: those of rounds 1 .. n_rounds; d_nodes: the trees of rounds
    0 .. n_rounds (DeviceBuffers or pointers, as tvm_fri_commit_phase filled them); tables: three table handles (main, aux,
    quotient segments) with their trees d_table_nodes, all over domain.length rows.
    -> dict(state, indices, last_codeword [n][3], last_polynomial [n][3], payloads: the tail_items(n_rounds) payloads in proof-item
    order, directory: their (offset, words)), or None where the entry point does not apply (n_checks > MAX_INDICES)"""
    ptr = lambda b: getattr(b, "ptr", b)
    n_rounds, n_items = len(d_codewords), tail_items(len(d_codewords))
    assert len(d_nodes) == n_rounds + 1 and len(tables) == 3 and len(d_table_nodes) == 3
    n_last = domain.length >> n_rounds
    state = _h(sponge_state).reshape(16)
    p_cw = (C.c_void_p * max(n_rounds, 1))(*[ptr(b) for b in d_codewords])
    p_nodes = (C.c_void_p * (n_rounds + 1))(*[ptr(b) for b in d_nodes])
    p_tables, p_table_nodes = (C.c_void_p * 3)(*[ptr(t) for t in tables]), (C.c_void_p * 3)(*[ptr(b) for b in d_table_nodes])
    after, indices = np.zeros(16, np.uint64), np.zeros(n_checks, np.uint64)
    last_cw, last_poly, directory = np.zeros((n_last, 3), np.uint64), np.zeros((n_last, 3), np.uint64), np.zeros((n_items, 2), np.uint64)
    capacity = ctx.lib.tvm_fri_query_and_open_payload_bound(domain.c(), n_rounds, n_checks, p_tables)
    payload, words = np.zeros(max(capacity, 1), np.uint64), C.c_uint64(0)
    status = ctx.lib.tvm_fri_query_and_open(ctx.handle, state.ctypes.data, ptr(d_codeword), domain.c(), n_rounds, p_cw, p_nodes, n_checks, p_tables,
                                            p_table_nodes, domain.length, after.ctypes.data, indices.ctypes.data, last_cw.ctypes.data,
                                            last_poly.ctypes.data, directory.ctypes.data, payload.ctypes.data, capacity, C.byref(words))
    if status == NOT_APPLICABLE:
        return None
    ctx._check(status, "tvm_fri_query_and_open")
    return dict(state=after, indices=indices, last_codeword=last_cw, last_polynomial=last_poly, directory=directory, words=int(words.value),
                payloads=[payload[int(o):int(o) + int(w)].copy() for o, w in directory])
