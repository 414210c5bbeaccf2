"""csrc/ntt.hip: k_lde_pass1_rows<8 | 9 | 10, 16>, the first pass of tvm_lde_table on 256-, 512- and 1024-point axes, with fewer
workgroups than tiles -- workgroup g of G walks the (column, tile) items g, g + G, ... of a chunk with the next tile's input in
registers.  The default launch, and the other suites with it, gives every item a workgroup: no second trip through the loop.  Here
TVM_OPTION_LDE_PASS1_WORKGROUPS makes the grid short: one workgroup that walks every tile and crosses the column boundary, three
(loops of uneven length: some workgroups run out of next items before others), more than there are items and the default (both
one tile each) -- each against the oracle's extension and against one another, on the CPU emulation and on the GPU.  Expansion 1
(pass 1 does not depend on it; the table stays small)."""
import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field

LDE_PASS1_WORKGROUPS = 10   # include/triton_hip.h: TVM_OPTION_LDE_PASS1_WORKGROUPS
H = 198
ABOVE_THE_ITEMS = 1 << 20   # the most items here: 9 virtual columns x 64 tiles
# 2^16 / 2^18 / 2^20 rows: the smallest trace of each instantiation (256 x 256, 512 x 512, 1024 x 1024); 2^17: n2 = 2 n1
HEIGHTS = [16, 17, 18, 20]


def columns_at(log_n):
    return 2 if log_n == 20 else 3


class Case:
    """the inputs of one (height, field kind) and the oracle's rows (computed once, never written); the tests hang the first whole
    table each backend gave on it (first_emu / first_gpu)"""

    def __init__(self, orc, log_n, fk, n_cols):
        rng = np.random.default_rng(5000 + 10 * log_n + fk)
        self.n, self.fk, self.n_cols = 1 << log_n, fk, n_cols
        shape = lambda k: (n_cols, k) + ((3,) if fk == 3 else ())
        self.trace, self.rnd = orc.random_elements(rng, shape(self.n)), orc.random_elements(rng, shape(H))
        self.trace_dom = ArithmeticDomain.of_length(self.n)
        self.ev = ArithmeticDomain.of_length(self.n).with_offset(field.generator())
        self.rows = np.unique(np.concatenate([[0, 1, 15, 16, 17, self.n - 1], rng.integers(0, self.n, 3000)])).astype(np.uint64)
        want = orc.lde_table(self.trace, self.rnd, orc.Domain(self.ev.offset, self.ev.generator, self.ev.length), fk)
        self.want_rows = want[self.rows.astype(np.int64)]
        self.want_rows.setflags(write=False)

    def master_table(self, ctx):
        return MasterTable(ctx, self.trace, self.rnd, self.trace_dom, self.ev, self.ev, self.fk)


@pytest.fixture(scope="module")
def cases(orc):
    made = {}

    def get(log_n, fk, n_cols=None):
        n_cols = n_cols or columns_at(log_n)
        key = (log_n, fk, n_cols)
        if key not in made:
            made[key] = Case(orc, log_n, fk, n_cols)
        return made[key]

    return get


@pytest.fixture
def workgroups(ctx, request):
    """sets TVM_OPTION_LDE_PASS1_WORKGROUPS on the module's context; the default comes back after the test"""
    request.addfinalizer(lambda: ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS1_WORKGROUPS, 0))
    return lambda value: ctx._check(ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS1_WORKGROUPS, value), "tvm_ctx_set_option")


@pytest.mark.parametrize("option", [1, 3, ABOVE_THE_ITEMS, 0])
@pytest.mark.parametrize("fk", [1, 3])
@pytest.mark.parametrize("log_n", HEIGHTS)
def test_every_grid_gives_the_oracles_table(ctx, cases, workgroups, log_n, fk, option):
    """sampled rows against the oracle; the whole table, word for word, against the first grid's of the same shape (the four
    option values of a shape run one after the other, so every one is compared with every other through the first)"""
    case = cases(log_n, fk)
    workgroups(option)
    mt = case.master_table(ctx)
    mt.maybe_low_degree_extend_all_columns()
    assert (mt.reveal_rows(case.rows) == case.want_rows).all()
    table = mt.low_degree_extended_table()
    mt.clear_cache()
    first = getattr(case, "first_" + ctx.kind, None)
    if first is None:
        table.setflags(write=False)
        setattr(case, "first_" + ctx.kind, (option, table))
    else:
        assert first[0] != option and (table == first[1]).all(), (first[0], option)


@pytest.mark.parametrize("log_n,fk", [(16, 3), (18, 1), (20, 1)])
def test_split_at_the_coefficients_with_three_workgroups(ctx, cases, workgroups, log_n, fk):
    """tvm_lde_column_coefficients (the inverse-only split: pass 1 writes the caller's coefficient array, one range of columns at a
    time) with three workgroups: the table assembled from the coefficients == the table of the plain call, one case per instantiation"""
    case = cases(log_n, fk)
    mt = case.master_table(ctx)
    mt.maybe_low_degree_extend_all_columns()
    want = mt.low_degree_extended_table()
    assert (want[case.rows.astype(np.int64)] == case.want_rows).all()
    workgroups(3)
    mt.low_degree_extend_by_column_blocks(2, 1)
    got = mt.low_degree_extended_table()
    mt.clear_cache()
    assert (got == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("option", [0, 256])
def test_the_production_shape_on_the_device(cases, option):
    """2^20 rows, 9 columns: 576 items.  With the default grid, and with the 256 workgroups of a grid that fills an MI355X once --
    two and three trips through the loop, at the device's own pace.  On the GPU only, so on a context of its own and not on the
    two-backend fixture."""
    from triton_vm_amd import Context

    case = cases(20, 1, 9)
    ctx = Context(device=0)
    try:
        ctx._check(ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS1_WORKGROUPS, option), "tvm_ctx_set_option")
        mt = case.master_table(ctx)
        mt.maybe_low_degree_extend_all_columns()
        got = mt.reveal_rows(case.rows)
        mt.clear_cache()
    finally:
        ctx.close()
    assert (got == case.want_rows).all()
