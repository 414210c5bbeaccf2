"""The context's cache of constant device tables (csrc/context.hip: cached_table -- powers, coset factors, the two table kinds
of k_lde_pass2_fused): a context that has extended tables over other domains before gives, word for word, what a fresh context
gives.  The cache is keyed by what a table depends on; a key that forgot one of those things would hand a later call the table
of an earlier one."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field

LDE_PASS2_TILES = 4   # include/triton_hip.h: TVM_OPTION_LDE_PASS2_TILES


def extend(ctx, trace, rnd, ev):
    mt = MasterTable(ctx, trace, rnd, ArithmeticDomain.of_length(trace.shape[1]), ev, ev, 1)
    mt.maybe_low_degree_extend_all_columns()
    got = mt.low_degree_extended_table()
    mt.clear_cache()
    return got


# 2^10 rows: the powers and coset-factor tables alone.  2^15 rows = 128 x 256: the smallest height whose rows of the middle pass
# have 256 points, where lde_table takes k_lde_pass2_fused and its twiddle and coset-factor tables (csrc/ntt.hip).
@pytest.mark.parametrize("log_n", [10, 15])
def test_a_used_context_extends_like_a_fresh_one(ctx, orc, log_n):
    rng = np.random.default_rng(4100 + log_n)
    n, h, n_cols = 1 << log_n, 17, 2
    trace, rnd = orc.random_elements(rng, (n_cols, n)), orc.random_elements(rng, (n_cols, h))
    g = field.generator()
    first = ArithmeticDomain.of_length(4 * n).with_offset(g)
    sequence = [first,                                                                      # expansion 4, offset g
                ArithmeticDomain.of_length(4 * n).with_offset(field.mont_mul(g, g)),        # the same generator, another offset
                ArithmeticDomain.of_length(8 * n).with_offset(g),                           # expansion 8
                first]                                                                      # the first domain again
    used = [extend(ctx, trace, rnd, ev) for ev in sequence]
    for step, ev in enumerate(sequence):
        fresh = type(ctx)(device=0, lib=ctx.lib)
        try:
            want = extend(fresh, trace, rnd, ev)
        finally:
            fresh.close()
        assert (used[step] == want).all(), f"step {step}: the used context's table differs from a fresh context's"
    assert (used[0] == used[3]).all()
    assert not (used[0] == used[1]).all(), "another offset is another table"
    if log_n <= 10:
        assert (used[0] == orc.lde_table(trace, rnd, orc.Domain(first.offset, first.generator, first.length), 1)).all()


def test_fused_and_tile_middle_pass_agree_at_the_shortest_fused_height(ctx, orc, request):
    """2^15 rows: TVM_OPTION_LDE_PASS2_TILES = 1 takes the tile kernels where the default takes k_lde_pass2_fused (so the
    default above did go through the fused kernel's tables); same sequence of domains on one context, the same tables."""
    rng = np.random.default_rng(4200)
    n, h, n_cols = 1 << 15, 17, 2
    trace, rnd = orc.random_elements(rng, (n_cols, n)), orc.random_elements(rng, (n_cols, h))
    g = field.generator()
    sequence = [ArithmeticDomain.of_length(4 * n).with_offset(g), ArithmeticDomain.of_length(4 * n).with_offset(field.mont_mul(g, g)),
                ArithmeticDomain.of_length(8 * n).with_offset(g)]
    set_option = lambda value: ctx._check(ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS2_TILES, value), "tvm_ctx_set_option")
    request.addfinalizer(lambda: ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS2_TILES, 0))
    fused = [extend(ctx, trace, rnd, ev) for ev in sequence]
    set_option(1)
    tiles = [extend(ctx, trace, rnd, ev) for ev in sequence]
    for step in range(len(sequence)):
        assert (fused[step] == tiles[step]).all(), f"step {step}: k_lde_pass2_fused and the tile kernels differ"
