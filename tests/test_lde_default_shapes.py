"""What a FRESH context runs in the table extension (csrc/context.hip: tvm_ctx_create): pass 1 with a workgroup per compute unit of its
device (TVM_OPTION_LDE_PASS1_WORKGROUPS starts at the compute-unit count; the CPU emulation reports none and starts at 0) and pass 2
with the coset scale absorbed (TVM_OPTION_LDE_PASS2_SCALE_ABSORBED starts at 1).  Neither may change a word: a context nobody has
touched against one with both options at 0, through tvm_lde_table; the grid pass 1 gets comes from csrc/lde_plan.h, walked by
tests/lde_pass1_grid_dump.cpp with the value the context reports (tvm_ctx_get_option)."""
import os
import subprocess

import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS1_WORKGROUPS, PASS2_SCALE_ABSORBED = 10, 12
# log2 rows -> columns, and what runs (csrc/lde_plan.h)
HEIGHTS = {16: 3, 18: 3, 20: 9}   # rows<8,16> fused<8> | rows<9,16> fused<9> | rows<10,16> fused<10>, 576 items of pass 1
EXPANSION = 4


def _fresh(kind):
    if kind == "emu":
        from tests.emu_fixture import emu_context

        return emu_context()
    from triton_vm_amd import Context

    return Context(device=0)


@pytest.fixture(scope="module")
def pair(ctx):
    """(a context nobody has touched, a context with both options at 0) of the module's kind"""
    fresh, plain = _fresh(ctx.kind), _fresh(ctx.kind)
    plain.lde_pass1_workgroups(0)
    plain.lde_pass2_scale_absorbed(False)
    yield fresh, plain
    fresh.close()
    plain.close()


def extension(c, trace, rnd, h, log_n, fk, ev, rows):
    n = 1 << log_n
    mt = MasterTable(c, trace, np.ascontiguousarray(rnd[:, :h]) if h else rnd[:, :0], ArithmeticDomain.of_length(n), ev, ev, fk)
    mt.maybe_low_degree_extend_all_columns()
    got = mt.low_degree_extended_table() if rows is None else mt.reveal_rows(rows)
    mt.clear_cache()
    return got


def compute_units():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("fk", [1, 3])
@pytest.mark.parametrize("log_n", sorted(HEIGHTS))
def test_a_fresh_context_extends_to_the_same_table(ctx, orc, pair, log_n, fk):
    """h = 0 and 198 randomizer rows; the whole table at 2^16 rows (also against the oracle), the edges of the first block of cosets,
    the last row and 500 random rows above"""
    if ctx.kind == "emu" and log_n > 16:
        pytest.skip("CPU suite time: 2^18 and 2^20 rows run on the GPU")
    fresh, plain = pair
    assert fresh.option(PASS2_SCALE_ABSORBED) == 1 and plain.option(PASS2_SCALE_ABSORBED) == 0 and plain.option(PASS1_WORKGROUPS) == 0
    assert fresh.option(PASS1_WORKGROUPS) == (0 if ctx.kind == "emu" else compute_units())
    n, cols = 1 << log_n, HEIGHTS[log_n]
    rng = np.random.default_rng(31 * log_n + fk)
    shape = lambda rows: (cols, rows) + ((3,) if fk == 3 else ())
    trace, rnd = orc.random_elements(rng, shape(n)), orc.random_elements(rng, shape(198))
    ev = ArithmeticDomain.of_length(EXPANSION * n).with_offset(field.generator())
    L = EXPANSION * n
    rows = None if log_n == 16 else np.unique(np.concatenate([[0, 1, EXPANSION - 1, EXPANSION, L - 1], rng.integers(0, L, 500)])).astype(np.uint64)
    for h in (0, 198):
        want = extension(plain, trace, rnd, h, log_n, fk, ev, rows)
        got = extension(fresh, trace, rnd, h, log_n, fk, ev, rows)
        assert (got == want).all(), h
        if log_n == 16 and h == 198 and (fk == 3 or ctx.kind == "gpu"):
            oracle_table = orc.lde_table(trace, rnd, orc.Domain(ev.offset, ev.generator, ev.length), fk)
            assert (got == oracle_table).all()


@pytest.fixture(scope="module")
def grid_of(tmp_path_factory):
    """(log_n, columns, option) -> (workgroups, items) of pass 1's launch, from csrc/lde_plan.h as the kernel walks it"""
    exe = str(tmp_path_factory.mktemp("lde_default_shapes") / "lde_pass1_grid_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lde_pass1_grid_dump.cpp"), "-o", exe])

    def grid(log_n, columns, option):
        line = subprocess.run([exe], input="%d %d %d\n" % (log_n, columns, option), text=True, check=True, stdout=subprocess.PIPE).stdout
        _, workgroups, items = line.split(" |")[0].split()
        return int(workgroups), int(items)

    return grid


@pytest.mark.gpu
def test_a_fresh_context_walks_pass_1_and_the_option_comes_back(grid_of):
    """2^20 rows x 9 columns: 576 (column, tile) items.  The value a fresh context reports is the device's compute-unit count, the
    grid that value gives has fewer workgroups than items (on an MI355X 256: more than one trip through the loop), and after
    set_option(.., 0) the grid is one workgroup per item again."""
    from triton_vm_amd import Context

    c = Context(device=0)
    try:
        start = c.option(PASS1_WORKGROUPS)
        assert start == compute_units() and start > 0
        workgroups, items = grid_of(20, 9, start)
        assert items == 576 and workgroups == min(start, items) and workgroups < items
        c.lde_pass1_workgroups(0)
        assert c.option(PASS1_WORKGROUPS) == 0
        assert grid_of(20, 9, c.option(PASS1_WORKGROUPS)) == (576, 576)
    finally:
        c.close()


def test_the_emulation_starts_with_a_workgroup_per_item(grid_of):
    """a device that reports no compute units: the start value stays 0"""
    c = _fresh("emu")
    try:
        assert c.option(PASS1_WORKGROUPS) == 0 and grid_of(20, 9, 0) == (576, 576)
    finally:
        c.close()
