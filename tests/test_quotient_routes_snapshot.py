"""The words of every route of the AIR quotient (csrc/quotient.hip, the routes chosen by csrc/quotient_plan.h), pinned by digest.

tests/golden/quotient_routes_digests.json holds the SHA-256 of the downloaded output words of each case below.  The digests were
generated with the library of commit 26e230d ("LDE: adopt three small wins together; combination from coefficients") -- the parent
of the commit that gave the quotient its own unit -- on the CPU emulation, before anything was moved: the unit is checked against
its parent, not against itself.  (`python -m tests.test_quotient_routes_snapshot <commit>` writes the file again from the emulation of the library it finds.)

The tables are random (fixed seeds), so the quotients are rational functions and every route yields other words: a digest pins the
route taken as well as the arithmetic.  X = 8, quotient domain = LDT domain = 8N with offset field.generator(), as
tests/test_air_remainder_coset.py builds its tables; the smallest shapes at which each route exists (256 rows: the smallest trace
whose block of n1 = 16 rows is a whole number of row blocks; 16 rows: the smallest that splits at all with a quarter class).

  case  rows  h  valid-trace  fork limit  remainder option   what is hashed
  a       16  3  off          0           -                  codeword: row by row
  b       16  3  on           0           -                  codeword: whole cosets, quarter class, no three-coset class
  c      256  5  on           0           on, min rows 16    codeword: whole cosets with the three-coset class (h = 5 fails the remainder gate)
  d      256  3  on           0           off                codeword: the same route as c, by the switch
  e      256  3  on           0           on, min rows 16    codeword: remainder route
  f      256  3  on           0           on, min rows 16    tvm_all_quotients_coefficients: all 4N + n1 coefficients, and n_coeffs
  g      256  3  on           256         -                  codeword: the fork takes precedence, row by row
  h      256  3  -            -           -                  tvm_coset_values_to_coefficients of tvm_air_class_values: the half class on the
                                                             cosets 0, 2, 4, 6, then quarter | three on the cosets 1, 3, 5 added to it
  i      256  3  off          0           -                  codeword, TVM_OPTION_LDE_PASS2_TILES = 1: other LDE kernels under the same
                                                             tables -- the snapshot depends on the quotient code alone"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field, stark

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quotient_routes_digests.json")
CASES = "abcdefghi"
LDE_PASS2_TILES = 4                                   # include/triton_hip.h: TVM_OPTION_LDE_PASS2_TILES
CLASS_HALF, CLASS_QUARTER, CLASS_THREE = 2, 4, 8      # include/triton_hip.h: TVM_AIR_CLASS_*


def _digest(*arrays):
    sha = hashlib.sha256()
    for a in arrays:
        sha.update(np.ascontiguousarray(a, dtype="<u8").tobytes())
    return sha.hexdigest()


class _Inputs:
    """the random traces, challenges and weights (made once), and the extended tables by (rows, h, LDE option), made on first use"""

    def __init__(self, ctx, orc):
        self.ctx, self.orc, self.tables = ctx, orc, {}
        rng = np.random.default_rng(20261)
        self.traces = {n: (orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3))) for n in (16, 256)}
        self.challenges, self.weights = orc.random_elements(rng, (63, 3)), orc.random_elements(rng, (604, 3))

    def extended(self, n, h, pass2_tiles=0):
        key = (n, h, pass2_tiles)
        if key not in self.tables:
            ctx, rng = self.ctx, np.random.default_rng(1000 * n + h)
            trace_dom = ArithmeticDomain.of_length(n)
            quot = ArithmeticDomain.of_length(8 * n).with_offset(field.generator())
            main = MasterTable(ctx, self.traces[n][0], self.orc.random_elements(rng, (379, h)), trace_dom, quot, quot, 1)
            aux = MasterTable(ctx, self.traces[n][1], self.orc.random_elements(rng, (91, h, 3)), trace_dom, quot, quot, 3)
            ctx._check(ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS2_TILES, pass2_tiles), "tvm_ctx_set_option")
            try:
                main.maybe_low_degree_extend_all_columns()
                aux.maybe_low_degree_extend_all_columns()
            finally:
                ctx.lib.tvm_ctx_set_option(ctx.handle, LDE_PASS2_TILES, 0)
            self.tables[key] = (main, aux, trace_dom, quot)
        return self.tables[key]


class _Options:
    def __init__(self, ctx, valid, fork, remainder=True, min_rows=0):
        self.ctx, self.valid, self.fork, self.remainder, self.min_rows = ctx, valid, fork, remainder, min_rows

    def __enter__(self):
        self.ctx.assume_valid_trace(self.valid)
        self.ctx.air_fork_max_workgroups(self.fork)
        self.ctx.air_remainder_coset(self.remainder, self.min_rows)

    def __exit__(self, *a):
        self.ctx.assume_valid_trace(False)
        self.ctx.air_fork_max_workgroups(256)
        self.ctx.air_remainder_coset(True, 0)


def _codeword(inp, n, h, valid, fork, remainder=True, min_rows=0, pass2_tiles=0):
    main, aux, trace_dom, quot = inp.extended(n, h, pass2_tiles)
    with _Options(inp.ctx, valid, fork, remainder, min_rows):
        out = stark.all_quotients_combined(inp.ctx, main, aux, trace_dom, quot, inp.challenges, inp.weights)
    return _digest(out.download((len(quot), 3)))


def _coefficients(inp):
    main, aux, trace_dom, quot = inp.extended(256, 3)
    with _Options(inp.ctx, True, 0, True, 16):
        d_coeffs, n_coeffs = stark.all_quotients_coefficients(inp.ctx, main, aux, trace_dom, quot, inp.challenges, inp.weights)
    assert n_coeffs == 4 * 256 + 16
    return _digest(d_coeffs.download((len(quot), 3))[:n_coeffs], [n_coeffs])


def _classes_by_coset(inp):
    ctx = inp.ctx
    main, aux, trace_dom, quot = inp.extended(256, 3)
    n = len(trace_dom)
    ch = np.ascontiguousarray(inp.challenges, np.uint64).reshape(63, 3)
    w = np.ascontiguousarray(inp.weights, np.uint64).reshape(604, 3)
    d_coeffs = ctx.to_device(np.zeros((4 * n, 3), np.uint64))     # the entry point ADDS to it
    for cosets, mask in (((0, 2, 4, 6), CLASS_HALF), ((1, 3, 5), CLASS_QUARTER | CLASS_THREE)):
        values = [ctx.alloc(3 * n) for _ in cosets]
        for k, v in zip(cosets, values):
            ctx._check(ctx.lib.tvm_air_class_values(ctx.handle, main._need_table(), aux._need_table(), trace_dom.c(), quot.c(), k, mask,
                                                    ch.ctypes.data, w.ctypes.data, v.ptr), "tvm_air_class_values")
        offsets = np.array([quot.value(k) for k in cosets], np.uint64)
        pointers = (C.c_void_p * len(values))(*[v.ptr for v in values])
        ctx._check(ctx.lib.tvm_coset_values_to_coefficients(ctx.handle, trace_dom.c(), len(cosets), offsets.ctypes.data, pointers,
                                                            d_coeffs.ptr), "tvm_coset_values_to_coefficients")
    return _digest(d_coeffs.download((4 * n, 3)))


COMPUTE = {
    "a": lambda inp: _codeword(inp, 16, 3, False, 0),
    "b": lambda inp: _codeword(inp, 16, 3, True, 0),
    "c": lambda inp: _codeword(inp, 256, 5, True, 0, True, 16),
    "d": lambda inp: _codeword(inp, 256, 3, True, 0, False),
    "e": lambda inp: _codeword(inp, 256, 3, True, 0, True, 16),
    "f": _coefficients,
    "g": lambda inp: _codeword(inp, 256, 3, True, 256),
    "h": _classes_by_coset,
    "i": lambda inp: _codeword(inp, 256, 3, False, 0, pass2_tiles=1),
}


@pytest.fixture(scope="module")
def inputs(ctx, orc):
    return _Inputs(ctx, orc)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", CASES)
def test_route_words_are_the_parents(inputs, golden, case):
    assert COMPUTE[case](inputs) == golden[case], f"case {case}: other words than the parent commit's (see the table in the module docstring)"


def test_the_cases_tell_the_routes_apart(golden):
    """the fixture itself: on the same tables every route gave other words -- d (whole cosets), e (remainder) and g (row by row) --
    so a case that passes took its own route; g (forked) and i (valid-trace mode off, other LDE kernels) are the one pair that
    agrees: both are the row-by-row evaluation of the same tables"""
    assert golden["g"] == golden["i"]
    assert len({golden[k] for k in CASES}) == len(CASES) - 1


if __name__ == "__main__":
    import sys

    from oracle import oracle
    from tests.emu_fixture import emu_context

    oracle.build()
    context = emu_context()
    made = _Inputs(context, oracle)
    digests = {k: COMPUTE[k](made) for k in CASES}
    context.close()
    with open(GOLDEN, "w") as f:
        json.dump({"generated_by": f"commit {sys.argv[1]} on the CPU emulation", "digests": digests}, f, indent=1)
        f.write("\n")
    print(json.dumps(digests, indent=1))
