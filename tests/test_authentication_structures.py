"""tvm_authentication_structures (csrc/proof_tail.hip: k_authentication_structures) against the Python restatement of
MerkleTree::authentication_structure (stark.auth_node_indices): the same heap indices in the same order for trees of every height and
every shape of query set, the digests at those indices, the limits, and trees that exist only as a number of leaves."""
import numpy as np

from tests.test_verifier_ldt_kernels import _query_sets, _tree
from triton_vm_amd import proof_tail, stark


def _sets(rng, n):
    if n == 1:   # (_query_sets draws from n // 2 parents)
        return [[0], [0, 0], [0] * 80]
    return _query_sets(rng, n)


def test_index_lists_and_nodes_equal_auth_node_indices_for_every_height_in_one_call(ctx, orc):
    rng = np.random.default_rng(31)
    jobs, trees = [], []
    for log_n in range(0, 13):
        n = 1 << log_n
        nodes = _tree(ctx, orc, rng, n)
        d_nodes = ctx.to_device(nodes)
        for idx in _sets(rng, n):
            if len(idx) > proof_tail.MAX_INDICES:   # "every leaf" of the two tallest trees is beyond the limit: not applicable
                assert proof_tail.authentication_structures(ctx, [(n, idx, d_nodes)]) is None
                continue
            jobs.append((n, idx, d_nodes))
            trees.append(nodes)
    assert len(jobs) > 90
    got = proof_tail.authentication_structures(ctx, jobs)   # trees of every height in ONE call
    for (n, idx, _), nodes, (node_idx, digests) in zip(jobs, trees, got):
        want = stark.auth_node_indices(n, idx)
        assert node_idx.tolist() == want.tolist(), (n, len(idx))
        assert (digests == nodes[want.astype(np.int64)].reshape(-1, 5)).all(), (n, len(idx))
    # the same jobs without their trees: the lists alone; and one job per call
    plans = proof_tail.authentication_structures(ctx, [(n, idx, None) for n, idx, _ in jobs])
    assert all(p[1] is None and p[0].tolist() == g[0].tolist() for p, g in zip(plans, got))
    for j in rng.integers(len(jobs), size=6):
        (node_idx, digests), = proof_tail.authentication_structures(ctx, [jobs[j]])
        assert node_idx.tolist() == got[j][0].tolist() and (digests == got[j][1]).all()


def test_the_limit_of_indices_per_tree(ctx, orc):
    rng = np.random.default_rng(32)
    n = 1 << 12
    nodes = _tree(ctx, orc, rng, n)
    d_nodes = ctx.to_device(nodes)
    repeated = [int(rng.integers(n))] * 1024
    distinct = [int(i) for i in rng.permutation(n)[:1024]]
    got = proof_tail.authentication_structures(ctx, [(n, repeated, d_nodes), (n, distinct, d_nodes), (n, [], d_nodes)])
    for idx, (node_idx, digests) in zip((repeated, distinct, []), got):
        want = stark.auth_node_indices(n, idx)
        assert node_idx.tolist() == want.tolist()
        assert (digests == nodes[want.astype(np.int64)].reshape(-1, 5)).all()
    assert len(got[0][0]) == 12 and len(got[2][0]) == 0
    # one index too many: TVM_NOT_APPLICABLE, nothing written (the raw call: the outputs keep their pattern)
    import ctypes as C

    idx = np.array(distinct + [0], np.uint64)
    sizes, counts, n_out = np.array([n], np.uint64), np.array([len(idx)], np.uint64), np.full(1, 77, np.uint64)
    out_idx, out_nodes = np.full(1025 * 12, 99, np.uint64), np.full(1025 * 12 * 5, 98, np.uint64)
    one = lambda p: (C.c_void_p * 1)(p)
    status = ctx.lib.tvm_authentication_structures(ctx.handle, 1, sizes.ctypes.data, one(idx.ctypes.data), counts.ctypes.data, one(d_nodes.ptr),
                                                   one(out_idx.ctypes.data), one(out_nodes.ctypes.data), n_out.ctypes.data)
    assert status == proof_tail.NOT_APPLICABLE
    assert (out_idx == 99).all() and (out_nodes == 98).all() and n_out[0] == 77
    assert proof_tail.authentication_structures(ctx, [(n, list(idx), None)]) is None
    assert proof_tail.authentication_structures(ctx, [(n, [5], d_nodes)])[0][0].tolist() == stark.auth_node_indices(n, [5]).tolist()


def test_plans_for_trees_that_are_not_in_memory(ctx):
    """the index arithmetic above 32 bits: heap indices of trees of 2^23, 2^32 and 2^40 leaves"""
    from triton_vm_amd.capi import TritonHipError

    rng = np.random.default_rng(33)
    jobs = [(1 << log_n, [int(i) for i in rng.integers(1 << log_n, size=173)], None) for log_n in (23, 32, 40)]
    jobs.append((1 << 40, [0, (1 << 40) - 1, 1 << 39, (1 << 39) - 1], None))
    for (n, idx, _), (node_idx, digests) in zip(jobs, proof_tail.authentication_structures(ctx, jobs)):
        assert digests is None and node_idx.tolist() == stark.auth_node_indices(n, idx).tolist()
    assert max(int(i) for i in proof_tail.authentication_structures(ctx, jobs[2:3])[0][0]) > 1 << 40
    for bad in [(12, [1], None), (1 << 41, [1], None), (16, [16], None)]:   # not a power of two, too tall, an index outside the tree
        try:
            proof_tail.authentication_structures(ctx, [bad])
            assert False, bad
        except TritonHipError:
            pass
