"""csrc/ntt_shift.h: canon_plan, the compile-time plan of the lazy sums -- which sums of a 2^K-point butterfly group are
bfe_add_folded and which outputs come out canonical.  tests/canon_plan_dump.cpp (g++, host only) prints it for every form the LDE row
kernels instantiate (csrc/ntt.hip: row_ntt_group, k_lde_pass2_fused) and every form of the tvm_field_op hook; here the propagation
rules are restated independently, on the dataflow graph of the group instead of the plan's walk over register masks:

    a value is REQUIRED canonical if  it is an owed output,  or the subtrahend of a difference,  or an operand of a required sum,
                                      or the minuend of a required difference;
    a product by a power of two other than 1 is canonical whatever goes in and requires nothing;
    a sum is folded exactly when it is not required.

and the invariants are asserted on the graph directly: every folded sum has a canonical operand, every other sum has two, every
subtrahend is canonical, every owed output is canonical.  The counts are the table of DESIGN.md 4.1."""
import os
import subprocess

import pytest

from triton_vm_amd import field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (K, dit, inverse, shift, in_canon, owed): what the kernels instantiate at 256 .. 1024 points (csrc/ntt.hip)
KERNEL_FORMS = {
    # pass 3, decimation in time, forward roots: first group / middle group (x[0] free) / last group (x[0] canonicalised, all owed)
    "pass3 first 16": (4, 1, 0, 0, 0xFFFF, 0), "pass3 middle 16": (4, 1, 0, 0, 0xFFFE, 0), "pass3 last 4": (2, 1, 0, 0, 0xF, 0xF),
    "pass3 first 8": (3, 1, 0, 0, 0xFF, 0), "pass3 middle 8": (3, 1, 0, 0, 0xFE, 0), "pass3 last 8": (3, 1, 0, 0, 0xFF, 0xFF),
    # pass 1 and the inverse row step of pass 2, decimation in frequency, inverse roots: groups above the last owe nothing
    # (x[0] is canonicalised after the butterflies); the last group owes nothing (pass 1) or everything (pass 2)
    "inverse 16": (4, 0, 1, 0, 0xFFFF, 0), "inverse last 4": (2, 0, 1, 0, 0xF, 0), "inverse last 2": (1, 0, 1, 0, 0x3, 0),
    "inverse last 16 owed": (4, 0, 1, 0, 0xFFFF, 0xFFFF), "inverse last 4 owed": (2, 0, 1, 0, 0xF, 0xF), "inverse last 2 owed": (1, 0, 1, 0, 0x3, 0x3),
    # the coset loop of pass 2: first group (plain and at shifted points), middle group (table form: x2[0] free), last group
    "coset first": (4, 1, 0, 0, 0xFFFF, 0), "coset first 39": (4, 1, 0, 39, 0xFFFF, 0), "coset first 78": (4, 1, 0, 78, 0xFFFF, 0),
    "coset first 117": (4, 1, 0, 117, 0xFFFF, 0), "coset middle": (4, 1, 0, 0, 0xFFFE, 0), "coset middle absorbed": (4, 1, 0, 0, 0xFFFF, 0),
    "coset last 4": (2, 1, 0, 0, 0xF, 0), "coset last 2": (1, 1, 0, 0, 0x3, 0),
}
ALL = lambda K: (1 << (1 << K)) - 1
HOOK_FORMS = {f"hook {K} {dit} {inverse} {shift} {owed_all}": (K, dit, inverse, shift, None, ALL(K) if owed_all else 0)
              for K, dit, inverse, shift in [(K, d, i, 0) for K in (2, 3, 4) for d in (1, 0) for i in (0, 1)] + [(4, 1, 0, s) for s in (39, 78, 117)]
              for owed_all in (0, 1)}
# folded sums of all sums: DESIGN.md 4.1 (outputs owed to nobody, outputs all owed)
COUNTS = {(4, 1, 0): (21, 6, 32), (4, 1, 39): (32, 17, 32), (4, 1, 78): (32, 17, 32), (4, 1, 117): (32, 17, 32), (4, 0, 0): (15, 0, 32),
          (3, 1, 0): (8, 1, 12), (3, 0, 0): (7, 0, 12), (2, 1, 0): (3, 0, 4), (2, 0, 0): (3, 0, 4)}


def graph(K, dit, inverse, shift):
    """the group as values: ('in', e) | ('sum', a, b, T, e) | ('diff', minuend, subtrahend) | ('shl', x); returns (values, outputs)"""
    R = 1 << K
    values = [("in", e) for e in range(R)]
    reg = list(range(R))   # the value each register holds

    def new(v):
        values.append(v)
        return len(values) - 1

    for T in (range(K) if dit else range(K - 1, -1, -1)):
        h = 1 << T
        for M in range(h):
            # log2 of the layer's twiddle: w_16 = 2^156, its inverse 2^36, squared down to order 2^K; at the points 2^shift w^j
            E = (((36 if inverse else 156) << (4 - K)) * M + shift) * (R // (2 * h)) % 192
            for q in range(R // (2 * h)):
                e = q * 2 * h + M
                u, w = reg[e], reg[e + h]
                if dit:
                    v = new(("shl", w)) if E % 96 else w
                    s, d = new(("sum", u, v, T, e)), new(("diff", u, v))
                    reg[e], reg[e + h] = (s, d) if E < 96 else (d, s)
                else:
                    s = new(("sum", u, w, T, e))
                    d = new(("diff", u, w)) if E < 96 else new(("diff", w, u))
                    reg[e], reg[e + h] = s, (new(("shl", d)) if E % 96 else d)
    return values, reg


def restated_plan(K, dit, inverse, shift, in_canon, owed):
    values, outputs = graph(K, dit, inverse, shift)
    required = {outputs[e] for e in range(1 << K) if owed >> e & 1} | {v[2] for v in values if v[0] == "diff"}
    grew = True
    while grew:
        grew = False
        for i in list(required):
            v = values[i]
            more = {v[1], v[2]} if v[0] == "sum" else {v[1]} if v[0] == "diff" else set()
            if not more <= required:
                required |= more
                grew = True
    folded = {i for i, v in enumerate(values) if v[0] == "sum" and i not in required}
    canonical = {}
    for i, v in enumerate(values):   # (values are numbered in the order they are computed)
        canonical[i] = {"in": lambda: bool(in_canon >> v[1] & 1), "sum": lambda: i not in folded, "diff": lambda: canonical[v[1]],
                        "shl": lambda: True}[v[0]]()
    holds = all(canonical[v[2]] for v in values if v[0] == "diff")
    holds = holds and all((canonical[v[1]] or canonical[v[2]]) if i in folded else (canonical[v[1]] and canonical[v[2]])
                          for i, v in enumerate(values) if v[0] == "sum")
    holds = holds and all(canonical[outputs[e]] for e in range(1 << K) if owed >> e & 1)
    fold = [0] * 4
    for i in folded:
        fold[values[i][3]] |= 1 << values[i][4]
    return dict(fold=fold, need_in=sum(1 << v[1] for i, v in enumerate(values) if v[0] == "in" and i in required),
                out_canon=sum(1 << e for e in range(1 << K) if canonical[outputs[e]]), folded=len(folded), ok=holds)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("canon_plan") / "canon_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unused-parameter",
                           "-DTVM_EMU", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "canon_plan_dump.cpp"), "-o", exe])

    def dump(forms):
        text = "".join("%d %d %d %d %x %x\n" % f for f in forms)
        out = subprocess.run([exe], input=text, text=True, check=True, stdout=subprocess.PIPE).stdout.splitlines()
        assert len(out) == len(forms)
        plans = []
        for line in out:
            _, fold, rest = line.split(" | ")
            need_in, out_canon, folded, ok = rest.split()
            plans.append(dict(fold=[int(f, 16) for f in fold.split()], need_in=int(need_in, 16), out_canon=int(out_canon, 16),
                              folded=int(folded), ok=bool(int(ok))))
        return plans

    return dump


def resolved(form, dump):
    """a hook form declares canonical exactly the inputs the plan needs (csrc/capi.hip: k_pow2_points_lazy)"""
    K, dit, inverse, shift, in_canon, owed = form
    if in_canon is None:
        in_canon = dump([(K, dit, inverse, shift, ALL(K), owed)])[0]["need_in"]
    return (K, dit, inverse, shift, in_canon, owed)


@pytest.mark.parametrize("name", list(KERNEL_FORMS) + list(HOOK_FORMS))
def test_plan_is_the_restated_propagation_and_keeps_every_precondition(dumped, name):
    form = resolved({**KERNEL_FORMS, **HOOK_FORMS}[name], dumped)
    plan, want = dumped([form])[0], restated_plan(*form)
    print(name, form, plan)
    assert want["ok"], "the restated rules do not hold on their own graph"
    assert plan == want
    assert plan == field.lazy_pow2_points_plan(*form)   # (the wrapper's mirror, which tests/test_lazy_pow2_points.py takes the free inputs from)
    assert plan["ok"] and plan["need_in"] & ~form[4] == 0 and form[5] & ~plan["out_canon"] == 0


def test_a_plan_whose_inputs_are_not_what_it_needs_is_not_ok(dumped):
    """a last group cannot take x[0] as it comes; a decimation-in-frequency group cannot take any input as it comes"""
    for form in [(4, 1, 0, 0, 0xFFFE, 0xFFFF), (2, 1, 0, 0, 0xE, 0xF), (4, 0, 1, 0, 0xFFFD, 0), (4, 1, 0, 0, 0xFFFD, 0)]:
        plan = dumped([form])[0]
        assert not plan["ok"] and plan == restated_plan(*form)


def test_counts(dumped):
    """folded sums per group with all inputs canonical: the table of DESIGN.md 4.1 (inverse roots: the same counts)"""
    for (K, dit, shift), (free, owed, sums) in COUNTS.items():
        for inverse in ((0, 1) if not shift else (0,)):
            none, everything = dumped([(K, dit, inverse, shift, ALL(K), 0), (K, dit, inverse, shift, ALL(K), ALL(K))])
            print(f"K={K} {'DIT' if dit else 'DIF'} inverse={inverse} shift={shift}: {none['folded']} / {sums} owed to nobody, "
                  f"{everything['folded']} / {sums} all owed; per layer {[bin(f).count('1') for f in none['fold'][:K]]} and "
                  f"{[bin(f).count('1') for f in everything['fold'][:K]]}")
            assert (none["folded"], everything["folded"], K << (K - 1)) == (free, owed, sums)
