"""csrc/lde_plan.h: which kernel lde_table launches for each of its three passes, as a function of the shape alone.  The header is
plain C++: tests/lde_plan_dump.cpp (g++, nothing else of the project) prints the plan for the shapes below, and the tables here are
the selection DESIGN.md 4.1 documents -- the one the suites on the device rely on when they say which kernel a height exercises."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVERSE_ONLY, FORWARD_ONLY = 1, 2   # csrc/lde_plan.h: TVM_LDE_INVERSE_ONLY / TVM_LDE_FORWARD_ONLY
H_N1, H_N1_PLUS_1 = -1, -2          # lde_plan_dump.cpp: h = n1 (the most the fused kernel takes) / n1 + 1
X = 8

GENERIC = ("k_ntt2_pass1", "k_lde_pass2", "k_lde_pass3")
# standard roots, h <= n1, no split: log_n -> passes 1, 2, 3
DEFAULT = {
    13: ("generic", "v3<7,6>", "generic"),
    14: ("generic", "v3<7,6>", "v3<7,6>"),
    15: ("generic", "fused<8>", "v3<7,6>"),
    16: ("rows<8,16>", "fused<8>", "rows<8,8>"),
    17: ("rows<8,16>", "fused<9>", "rows<8,8>"),
    18: ("rows<9,16>", "fused<9>", "rows<9,8>"),
    19: ("rows<9,16>", "fused<10>", "rows<9,8>"),
    20: ("rows<10,16>", "fused<10>", "rows<10,8>"),
    21: ("rows<10,16>", "fused<11>", "rows<10,8>"),
    22: ("rows<11,8>", "fused<11>", "halves<8>"),
    23: ("rows<11,8>", "v3<12,10>", "halves<8>"),
    24: ("generic", "v3<12,10>", "v3<12,10>"),
}
DEFAULT.update({log_n: ("generic",) * 3 for log_n in range(1, 13)})
# TVM_OPTION_LDE_PASS2_TILES = 1 (heights not listed: as DEFAULT)
TILES = {
    15: ("generic", "v3<8,6>", "v3<7,6>"),
    16: ("generic", "v3<8,6>", "v3<8,6>"),
    17: ("generic", "generic", "v3<8,6>"),
    18: ("generic", "generic", "generic"),
    19: ("generic", "generic", "generic"),
    20: ("rows<10,16>", "generic", "rows<10,8>"),
    21: ("rows<10,16>", "v3<11,10>", "rows<10,8>"),
    22: ("generic", "v3<11,10>", "rows<11,8>"),
    23: ("generic", "v3<12,10>", "rows<11,8>"),
}
TILES = {**DEFAULT, **TILES}


def full_name(pass_no, short):
    if short == "generic":
        return GENERIC[pass_no]
    if short == "-":
        return "-"
    family = {"rows": ("k_lde_pass1_rows", None, "k_lde_pass3_rows"), "fused": (None, "k_lde_pass2_fused", None),
              "v3": (None, "k_lde_pass2_v3", "k_lde_pass3_v3"), "halves": (None, None, "k_lde_pass3_halves")}[short.split("<")[0]]
    return family[pass_no] + short[short.index("<"):]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(log_n, h, std_roots, tiles_option, mode) -> the three passes as dicts; one compilation, one process per call"""
    exe = str(tmp_path_factory.mktemp("lde_plan") / "lde_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lde_plan_dump.cpp"), "-o", exe])
    shapes = [(log_n, h, std, opt, mode) for log_n in range(1, 25) for h in (H_N1, H_N1_PLUS_1) for std in (1, 0) for opt in (0, 1)
              for mode in (0, INVERSE_ONLY, FORWARD_ONLY)]
    out = subprocess.run([exe], input="".join(f"{s[0]} {X} {s[1]} {s[2]} {s[3]} {s[4]}\n" for s in shapes), text=True, check=True,
                         stdout=subprocess.PIPE).stdout.splitlines()
    assert len(out) == len(shapes)
    plans = {}
    for shape, line in zip(shapes, out):
        passes = []
        for part in line.split(" | ")[1:]:
            kernel, block, lds, rows, tiles, grid_y = part.split()
            passes.append(dict(kernel=kernel, block=int(block), lds=int(lds), rows=int(rows), tiles=int(tiles), grid_y=int(grid_y)))
        plans[shape] = passes
    return lambda log_n, h=H_N1, std=1, opt=0, mode=0: plans[(log_n, h, std, opt, mode)]


def kernels(passes):
    return tuple(p["kernel"] for p in passes)


def expected(table, log_n):
    return tuple(full_name(i, s) for i, s in enumerate(table[log_n]))


@pytest.mark.parametrize("log_n", sorted(DEFAULT))
def test_default_selection(plan, log_n):
    assert kernels(plan(log_n)) == expected(DEFAULT, log_n)


@pytest.mark.parametrize("log_n", sorted(TILES))
def test_selection_with_the_tile_option(plan, log_n):
    assert kernels(plan(log_n, opt=1)) == expected(TILES, log_n)


@pytest.mark.parametrize("log_n", sorted(DEFAULT))
def test_more_randomizers_than_n1_leave_the_fused_kernel_only(plan, log_n):
    """h = n1 is the last height of the randomizers the fused kernel takes; with n1 + 1 the middle pass is the tile option's, the
    other two passes stay"""
    want = expected(DEFAULT, log_n)
    assert kernels(plan(log_n, h=H_N1)) == want
    assert kernels(plan(log_n, h=H_N1_PLUS_1)) == (want[0], expected(TILES, log_n)[1], want[2])
    assert kernels(plan(log_n, h=H_N1_PLUS_1, opt=1)) == expected(TILES, log_n)


def test_what_the_device_suites_say_about_their_heights(plan):
    # tests/test_table_cache.py: "2^15 rows ... the option takes the tile kernels where the default takes k_lde_pass2_fused"
    assert plan(15)[1]["kernel"] == "k_lde_pass2_fused<8>" and plan(15, opt=1)[1]["kernel"] == "k_lde_pass2_v3<8,6>"
    # tests/test_kernels_ntt.py: h = n1 "one more and the tile kernel takes over" -- (log_n, h) = (19, 513) and (21, 1025)
    assert plan(19, h=H_N1)[1]["kernel"] == "k_lde_pass2_fused<10>" and plan(19, h=H_N1_PLUS_1)[1]["kernel"] == "k_lde_pass2"
    assert plan(21, h=H_N1)[1]["kernel"] == "k_lde_pass2_fused<11>" and plan(21, h=H_N1_PLUS_1)[1]["kernel"] == "k_lde_pass2_v3<11,10>"


@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("log_n", sorted(DEFAULT))
def test_other_roots_take_the_generic_kernels(plan, log_n, opt):
    for h in (H_N1, H_N1_PLUS_1):
        assert kernels(plan(log_n, h=h, std=0, opt=opt)) == GENERIC


@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("std", [1, 0])
@pytest.mark.parametrize("log_n", sorted(DEFAULT))
def test_a_split_mode_skips_one_pass_and_changes_no_other(plan, log_n, std, opt):
    whole = plan(log_n, std=std, opt=opt)
    skipped = dict(kernel="-", block=0, lds=0, rows=0, tiles=0, grid_y=0)
    assert plan(log_n, std=std, opt=opt, mode=INVERSE_ONLY) == [whole[0], whole[1], skipped]
    assert plan(log_n, std=std, opt=opt, mode=FORWARD_ONLY) == [skipped, whole[1], whole[2]]


def row_words(n):   # csrc/lde_plan.h TVM_ROW_WORDS: a row of n points with a pad word per 16, odd pitch
    return n + n // 16 + 1


@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("log_n", sorted(DEFAULT))
def test_launch_shapes_of_the_row_and_fused_kernels(plan, log_n, opt):
    """block size = the kernel's __launch_bounds__, LDS bytes = the layout the kernel's source describes (csrc/ntt.hip), restated here
    from the template arguments; everything within the 160 KiB the kernels are given"""
    n1, n2 = 1 << (log_n // 2), 1 << (log_n - log_n // 2)
    p1, p2, p3 = plan(log_n, opt=opt)
    for p in (p1, p2, p3):
        assert p["block"] % 64 == 0 and 64 <= p["block"] <= 1024 and 0 < p["lds"] <= 160 * 1024
    if "rows" in p1["kernel"]:   # k_lde_pass1_rows<LOGN, ROWS>: ROWS rows, a row of twiddles, at 2048 points 512 words of pair flags
        logn, rows = map(int, p1["kernel"].split("<")[1][:-1].split(","))
        assert (1 << logn) == n1 and p1["rows"] == rows and p1["block"] == (n1 // 16) * rows
        assert p1["lds"] == 8 * (rows * row_words(n1) + n1 + (512 if logn == 11 else 0))
    else:
        assert p1["kernel"] == "k_ntt2_pass1" and p1["lds"] == 8 * n1 * p1["rows"]
    if "fused" in p2["kernel"]:   # k_lde_pass2_fused<LOGN>: 8 rows of pitch ROWW, 16 x 17 twiddles, one coset's factors, a word per row
        logn = int(p2["kernel"].split("<")[1][:-1])
        roww = {8: 296, 9: 552, 10: 1096, 11: 2184}[logn]
        assert (1 << logn) == n2 and p2["rows"] == 8 and p2["block"] == 8 * n2 // 16
        assert p2["lds"] == 8 * (8 * roww + 272 + row_words(n2) + 8 + (512 if logn == 11 else 0))
    if "rows" in p3["kernel"] or "halves" in p3["kernel"]:   # 8 wavefronts, a row each (halves: of 1024 points), and a row of twiddles
        points = 1024 if "halves" in p3["kernel"] else n1
        assert p3["rows"] == 8 and p3["block"] == 512 and p3["lds"] == 8 * (8 * row_words(points) + points)
    if p3["kernel"] == "k_lde_pass3":
        assert p3["tiles"] == 0 and p3["grid_y"] == 0
    else:   # the row and tile kernels of pass 3: the grid's second dimension covers every row once and fits a grid
        assert p3["tiles"] in (1, 4, 8, 16) and p3["tiles"] * p3["grid_y"] * p3["rows"] == X * n2 and p3["grid_y"] < 65536
