"""csrc/quotient_plan.h: which route the AIR quotient takes and on which cosets valid-trace mode evaluates each class of constraints,
as a function of the shape and the options alone.  The header is plain C++: tests/quotient_plan_dump.cpp (g++, nothing else of the
project but the public header) prints the plan for the sweep below.  The degree bound is restated here from its derivation, not
copied from the header: with columns of at most m coefficients, the consistency / transition quotients of degree-d constraints have
at most d (m - 1) + 2 - N coefficients, the initial / terminal ones of degree d - 1 (the same class) at most (d - 1)(m - 1) + 1; a
polynomial is determined by as many points as it has coefficients."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, HALF, QUARTER, THREE = 1, 2, 4, 8          # include/triton_hip.h: TVM_AIR_CLASS_*
DEGREE = {HALF: 4, THREE: 3, QUARTER: 2}         # the degree of a class's consistency / transition constraints
DEFAULT_MIN_ROWS = 1 << 18                       # include/triton_hip.h: TVM_OPTION_AIR_REMAINDER_MIN_ROWS


def n1_of(log_n):
    return 1 << (log_n // 2)


def class_fits(d, m, n, points):
    return max(d * (m - 1) + 2 - n, (d - 1) * (m - 1) + 1) <= points


def class_cosets(m, n):
    """what tvm_air_class_cosets answers: (half, quarter, three)"""
    return (4 if class_fits(4, m, n, 4 * n) else 0, 2 if class_fits(2, m, n, 2 * n) else 0, 3 if class_fits(3, m, n, 3 * n) else 0)


def heights(log_n):
    n, n1 = 1 << log_n, n1_of(log_n)
    return sorted({0, 1, 3, 5, n1 - 1, n1, n // 4, n // 2, n})


SHAPES = [(log_n, h, expansion, option, min_rows, forked, with_class_0)
          for log_n in range(1, 25) for h in heights(log_n) for expansion in (4, 8, 16) for option in (1, 0)
          for min_rows in (16, DEFAULT_MIN_ROWS) for forked in (0, 1) for with_class_0 in (0, 1)]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """shape -> dict(route, n_coeffs, cosets=(half, quarter, three), steps=[dict(mask, stride, n, cosets, t)]); one compilation, one process"""
    exe = str(tmp_path_factory.mktemp("quotient_plan") / "quotient_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "quotient_plan_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], input="".join(" ".join(map(str, s)) + "\n" for s in SHAPES), text=True, check=True,
                         stdout=subprocess.PIPE).stdout.splitlines()
    assert len(out) == len(SHAPES)
    result = {}
    for shape, line in zip(SHAPES, out):
        head, *parts = line.split(" | ")
        route, n_coeffs, c_half, c_quarter, c_three = head.split()
        steps = []
        for part in parts:
            mask, stride, n, cosets, t = part.split()
            steps.append(dict(mask=int(mask), stride=int(stride), n=int(n), t=int(t),
                              cosets=None if cosets == "-" else tuple(int(k) for k in cosets.split(","))))
        result[shape] = dict(route=route, n_coeffs=int(n_coeffs), cosets=(int(c_half), int(c_quarter), int(c_three)), steps=steps)
    return result


def plan_of(plans, log_n, h, expansion=8, option=1, min_rows=DEFAULT_MIN_ROWS, forked=0, with_class_0=0):
    return plans[(log_n, h, expansion, option, min_rows, forked, with_class_0)]


def test_class_cosets_are_the_degree_bound(plans):
    for (log_n, h, *_), plan in plans.items():
        n = 1 << log_n
        assert plan["cosets"] == class_cosets(n + h, n), (log_n, h)


def test_whole_coset_steps(plans):
    """the half class on the half domain in one step, the quarter class on the quarter domain in one, the three-coset class on the
    cosets 0, 2, 4 or with the half class; every class on as many cosets as its bound asks for -- at expansion 8 exactly the counts of
    tvm_air_class_cosets -- and wherever those counts hold at expansion 8, the route is class-wise"""
    seen = 0
    for shape, plan in plans.items():
        log_n, h, expansion, option, min_rows, forked, with_class_0 = shape
        n, m = 1 << log_n, (1 << log_n) + h
        half, quarter, three = class_cosets(m, n)
        if expansion == 8 and not forked and half and quarter and log_n >= 2:
            assert plan["route"] != "row_by_row", shape
        if plan["route"] != "whole_cosets":
            continue
        seen += 1
        steps = plan["steps"]
        assert plan["n_coeffs"] == expansion * n // 2 and not forked
        assert (steps[0]["stride"], steps[0]["n"]) == (2, expansion // 2) and steps[0]["mask"] & HALF
        assert (steps[1]["stride"], steps[1]["n"], steps[1]["mask"]) == (4, expansion // 4, QUARTER)
        if len(steps) == 3:
            assert steps[0]["mask"] == HALF and (steps[2]["mask"], steps[2]["stride"], steps[2]["cosets"]) == (THREE, 0, (0, 2, 4))
            assert steps[2]["n"] == 3 == three and expansion == 8
        else:
            assert len(steps) == 2 and steps[0]["mask"] == HALF | THREE
        for step in steps:
            for bit, d in DEGREE.items():
                if step["mask"] & bit:
                    assert class_fits(d, m, n, step["n"] * n), shape
        if expansion == 8:
            assert (steps[0]["n"], steps[1]["n"]) == (half, quarter)
    assert seen


def test_remainder_route_is_one_coset_fewer_per_class_plus_t(plans):
    """exactly where the option is on, the trace has the minimum rows, the tables' blocks are whole row blocks, the quotient domain is
    the eight cosets the tables hold and is not forked, and every class's quotient fits its cosets less one plus the n1 points of T"""
    seen = 0
    for shape, plan in plans.items():
        log_n, h, expansion, option, min_rows, forked, with_class_0 = shape
        n, m, n1 = 1 << log_n, (1 << log_n) + h, n1_of(log_n)
        whole = dict(zip((HALF, QUARTER, THREE), class_cosets(m, n)))
        expected = (option and not forked and expansion == 8 and n >= min_rows and n1 % 16 == 0 and all(whole.values()) and
                    all(class_fits(d, m, n, (whole[bit] - 1) * n + n1) for bit, d in DEGREE.items()) and 4 * (m - 1) + 1 <= 4 * n + n1)
        assert (plan["route"] == "remainder_coset") == bool(expected), shape
        if not expected:
            continue
        seen += 1
        steps = list(plan["steps"])
        if with_class_0:
            first = steps.pop(0)
            assert (first["mask"], first["stride"], first["cosets"], first["t"]) == (FULL, 0, (0, 2, 4, 6), 1)
        assert plan["n_coeffs"] == 4 * n + (n1 if with_class_0 else 0)
        assert [s["mask"] for s in steps] == [HALF, THREE, QUARTER]
        for step in steps:
            assert step["stride"] == 0 and step["n"] == whole[step["mask"]] - 1 and step["cosets"] == tuple(range(0, 2 * step["n"], 2))
            assert step["t"] == 6 and step["t"] not in step["cosets"]
    assert seen


def test_a_split_always_has_its_quarter_class(plans):
    """the half-domain conditions alone imply the quarter-domain ones for every trace of at least 4 rows (so the plan has no arm for
    a class-wise route without a quarter step), and every class-wise plan evaluates the quarter class in a step of its own"""
    for shape, plan in plans.items():
        log_n, h, expansion = shape[:3]
        n, m = 1 << log_n, (1 << log_n) + h
        half, quarter = expansion * n // 2, expansion * n // 4
        if log_n >= 2 and half >= 2 * n and class_fits(4, m, n, half):
            assert quarter >= 2 * n and class_fits(2, m, n, quarter), shape
        if plan["route"] != "row_by_row":
            assert [s["mask"] for s in plan["steps"]].count(QUARTER) == 1, shape


def test_named_shapes(plans):
    """the shapes the device tests rely on (tests/test_air_remainder_coset.py, tests/test_quotient_routes_snapshot.py, the benchmark)"""
    assert plan_of(plans, 8, 3, min_rows=16)["route"] == "remainder_coset"
    five = plan_of(plans, 8, 5, min_rows=16)
    assert five["route"] == "whole_cosets" and [s["mask"] for s in five["steps"]] == [HALF, QUARTER, THREE]
    assert plan_of(plans, 8, 3)["route"] == "whole_cosets"                     # the default minimum: 2^18 rows
    assert plan_of(plans, 8, 3, option=0, min_rows=16)["route"] == "whole_cosets"
    small = plan_of(plans, 4, 3)
    assert small["route"] == "whole_cosets" and [s["mask"] for s in small["steps"]] == [HALF | THREE, QUARTER]
    for h in heights(20):
        if h <= n1_of(20) // 4:
            assert plan_of(plans, 20, h)["route"] == "remainder_coset"
            assert plan_of(plans, 20, h, with_class_0=1)["n_coeffs"] == 4 * (1 << 20) + 1024
    for shape, plan in plans.items():
        if shape[5]:
            assert plan["route"] == "row_by_row" and not plan["steps"], shape
