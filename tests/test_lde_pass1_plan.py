"""csrc/lde_plan.h: the grid of pass 1's persistent row kernels (k_lde_pass1_rows<8 | 9 | 10, 16>).  A launch has columns x n2 / 16
work items (column, tile), tile-fastest inside a column; workgroup g of G takes g, g + G, ...  tests/lde_pass1_grid_dump.cpp (g++,
nothing else of the project) walks them as the kernel does: every (column, tile) exactly once, for every workgroup count the device
suite sets (tests/test_lde_pass1_persistent.py) and for the default, a workgroup per item."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_KERNELS = {16: 8, 17: 8, 18: 9, 19: 9, 20: 10, 21: 10}   # log_n -> the instantiation's LOGN
COLUMNS = [1, 3, 9, 96]
OPTIONS = [1, 3, 256, 1 << 20, 0]   # (2^20: above every item count here; 0: the default)


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lde_pass1_grid") / "lde_pass1_grid_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lde_pass1_grid_dump.cpp"), "-o", exe])
    shapes = [(log_n, cols, opt) for log_n in list(ROW_KERNELS) + [15, 22] for cols in COLUMNS for opt in OPTIONS]
    out = subprocess.run([exe], input="".join("%d %d %d\n" % s for s in shapes), text=True, check=True,
                         stdout=subprocess.PIPE).stdout.splitlines()
    assert len(out) == len(shapes)
    parsed = {}
    for shape, line in zip(shapes, out):
        head, *groups = line.split(" |")
        kernel, G, items = head.split()
        parsed[shape] = (kernel, int(G), int(items), [[tuple(map(int, w.split(":"))) for w in g.split()] for g in groups])
    return parsed


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("columns", COLUMNS)
@pytest.mark.parametrize("log_n", sorted(ROW_KERNELS))
def test_the_grid_covers_every_item_exactly_once(walks, log_n, columns, option):
    kernel, G, items, groups = walks[(log_n, columns, option)]
    logn = ROW_KERNELS[log_n]
    tiles = (1 << (log_n - log_n // 2)) // 16
    assert kernel == str(logn) and items == columns * tiles
    assert G == min(option if option else items, items) and len(groups) == G and G < 65536 * 32768
    seen = [item for g in groups for item in g]
    assert len(seen) == items and set(seen) == {(c, t) for c in range(columns) for t in range(tiles)}
    for g, walk in enumerate(groups):   # workgroup g: items g, g + G, ... in the tile-fastest numbering; none without an item
        assert walk == [divmod(i, tiles) for i in range(g, items, G)] and walk


@pytest.mark.parametrize("log_n", [15, 22])
def test_other_heights_have_no_persistent_pass_1(walks, log_n):
    """2^15 rows: the generic kernel; 2^22: k_lde_pass1_rows<11,8>, one tile per workgroup as before"""
    assert walks[(log_n, 3, 0)][0] == "-"
