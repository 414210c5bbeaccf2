"""The two forms of a Tip5 round on the matrix cores (csrc/tip5.h: tip5_mfma_recombine) through the C ABI, bit for bit against
the oracle: a round that hands st[1..3] on as folded 64-bit representatives (every round but the last of a permutation whose
state is read, and every round between two blocks of a row) and the round that makes all four words canonical.  Rows and
digests are built from the words where the carries of the recombination and of the Montgomery reduction switch; rows of one
repeated word (all 0, all p - 1) drive the ten position sums D_c of the MDS layer to their extremes.  Runs on the CPU fiber
emulation of the same sources (-m "not gpu") and on the MI355X (-m gpu)."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field

P = field.P
EDGE = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, P - (1 << 32), P - 2, P - 1]
N_ROWS = 64


def edge_rows(orc, rng, n_rows, width):
    """n_rows x width words: one row per edge word repeated, then rows drawn from the edge words alone, then rows that mix edge
    and random words, then random rows"""
    edge = np.array(EDGE, np.uint64)
    rows = orc.random_elements(rng, (n_rows, width))
    k = len(edge)
    rows[:k] = edge[:, None]
    rows[k:3 * k] = edge[rng.integers(0, k, (2 * k, width))]
    mixed = slice(3 * k, 3 * k + (n_rows - 3 * k) // 2)
    pick = rng.random(rows[mixed].shape) < 0.5
    rows[mixed] = np.where(pick, edge[rng.integers(0, k, rows[mixed].shape)], rows[mixed])
    return rows


# 1, 9: no full block (only the permutation whose digest is read); 10: exactly one block and the padding block; 11, 20, 29: full blocks
# and a partial one; 379: the main table's width, 37 permutations between blocks and the last one
@pytest.mark.parametrize("width", [1, 9, 10, 11, 20, 29, 379])
def test_hash_rows_on_edge_rows(ctx, orc, width):
    rng = np.random.default_rng(5000 + width)
    rows = edge_rows(orc, rng, N_ROWS, width)
    # the table IS the trace: evaluated on the trace domain itself the randomizer share (a multiple of the zerofier) vanishes
    dom = ArithmeticDomain.of_length(N_ROWS)
    mt = MasterTable(ctx, np.ascontiguousarray(rows.T), np.zeros((width, 1), np.uint64), dom, dom, dom, 1)
    mt.maybe_low_degree_extend_all_columns()
    assert (mt.low_degree_extended_table() == rows).all(), "the table under test is not the rows handed in"
    got = mt.hash_all_ldt_domain_rows()
    assert (got < np.uint64(P)).all(), "a digest word is not canonical"
    assert (got == orc.hash_rows(rows)).all()


def edge_digests(orc, rng, n):
    edge = np.array(EDGE, np.uint64)
    leaves = edge[rng.integers(0, len(edge), (n, 5))]
    leaves[:2 * len(edge)] = np.repeat(edge, 2)[:, None]   # parent i < 9 absorbs ten copies of one edge word
    return leaves


def test_merkle_tree_of_edge_digests(ctx, orc, request):
    """64 leaves: the last levels inside one workgroup (sixteen lanes per parent).  The level kernels have thresholds no option
    lowers to 64 leaves -- four lanes per parent on the matrix cores above 2^15 parents, sixteen lanes per parent with a launch per
    level above 64 with TVM_OPTION_MERKLE_SUBTREES = 0 -- so on the GPU a tree of 2^17 leaves takes the same words through them (a few
    milliseconds there, minutes on the fiber emulation)."""
    rng = np.random.default_rng(64)
    sizes = [(64, 1)] + ([(1 << 17, 1), (1 << 17, 0)] if ctx.kind == "gpu" else [])
    for n, subtrees in sizes:
        if not subtrees:
            ctx._check(ctx.lib.tvm_ctx_set_option(ctx.handle, 6, 0), "tvm_ctx_set_option")
            request.addfinalizer(lambda: ctx.lib.tvm_ctx_set_option(ctx.handle, 6, 1))
        leaves = edge_digests(orc, rng, n)
        d_nodes, d_leaves = ctx.alloc(10 * n), ctx.to_device(leaves)
        ctx._check(ctx.lib.tvm_merkle_tree(ctx.handle, d_leaves.ptr, n, d_nodes.ptr), "merkle")
        got = d_nodes.download((2 * n, 5))
        assert (got < np.uint64(P)).all(), "a node word is not canonical"
        assert (got == orc.merkle_tree(leaves)).all(), (n, subtrees)


def test_bfe_mul_on_non_canonical_inputs(ctx):
    """tip5_pow7 is handed folded words: bfe_mul (the device's asm form on the GPU, the plain C++ form on the emulation; tvm_field_op 2)
    must return SOME 64-bit representative of a b 2^-64 mod p for every pair of 64-bit words, canonical or not."""
    words = [P, P + 1, (1 << 64) - (1 << 32), (1 << 64) - 1, P - 1, 0, 1, (1 << 32) - 1]
    a = np.repeat(np.array(words, np.uint64), len(words))
    b = np.tile(np.array(words, np.uint64), len(words))
    out, da, db = ctx.alloc(a.size), ctx.to_device(a), ctx.to_device(b)
    ctx._check(ctx.lib.tvm_field_op(ctx.handle, 2, da.ptr, db.ptr, out.ptr, a.size), "field_op")
    r_inv = pow(1 << 64, P - 2, P)
    got = [int(v) % P for v in out.download()]
    want = [int(x) * int(y) * r_inv % P for x, y in zip(a, b)]
    assert got == want
