"""The LDE row kernels with lazy sums (csrc/ntt.hip: row_ntt_group with LZ, the coset loop of k_lde_pass2_fused; csrc/ntt_shift.h:
canon_plan): inside a butterfly group, and in LDS between the groups of a transform, words may be any 64-bit representative -- every
word that reaches memory is canonical and is the word the oracle computes.

  * lde_table on three base-field columns at 2^16, 2^18 and 2^20 rows (tests/test_lde_plan.py: the smallest heights at which all
    three passes run their <8>, <9> and <10> instantiations), expansion 8, h = 0 and 5 randomizers: a column of p - 1 in every row (the
    sums of sixteen of them wrap at every layer), a column of zeros with a single p - 1, a random column.  Every word of the table
    equals oracle.fast.lde_table's and is below p.
  * the split at the coefficients at 2^16 rows: tvm_lde_column_coefficients (TVM_LDE_INVERSE_ONLY, the inverse row step's words go to
    memory) returns N times the oracle's interpolant in the library's coefficient form, canonical; tvm_lde_table_add_columns
    (TVM_LDE_FORWARD_ONLY) makes the same table from them.
  * prove_fib at 2^10 rows hashes to the committed digest: that height runs none of the changed kernels -- a guard against collateral
    change in the generic ones, which share ntt_shift.h.
The same must hold with the compile-time switch TVM_LDE_LAZY_SUMS at 0 (the default: every word canonical everywhere) and at 1; the
suite runs whichever library is built, and a library built with -DTVM_LDE_LAZY_SUMS=1 passed it on the device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from triton_vm_amd import ArithmeticDomain, MasterTable, field

P = field.P
EXPANSION, COLS = 8, 3


@pytest.fixture(scope="module")
def case(orc):
    """(log_n, h) -> trace, randomizers, evaluation domain and the oracle's table, computed once and left unchanged"""
    made = {}

    def get(log_n, h):
        if (log_n, h) not in made:
            n = 1 << log_n
            rng = np.random.default_rng(log_n)   # (the same trace for both h)
            trace = np.zeros((COLS, n), np.uint64)
            trace[0, :] = P - 1
            trace[1, int(rng.integers(0, n))] = P - 1
            trace[2, :] = orc.random_elements(rng, n)
            rnd = np.ascontiguousarray(orc.random_elements(rng, (COLS, 5))[:, :h])
            ev = ArithmeticDomain.of_length(EXPANSION * n).with_offset(field.generator())
            want = orc.fast.lde_table(trace, rnd, orc.Domain(ev.offset, ev.generator, ev.length))
            for a in (trace, rnd, want):
                a.setflags(write=False)
            made[(log_n, h)] = (trace, rnd, ev, want)
        return made[(log_n, h)]

    return get


@pytest.mark.parametrize("h", [0, 5])
@pytest.mark.parametrize("log_n", [16, 18, 20])
def test_table_equals_the_oracles_and_is_canonical(ctx, case, log_n, h):
    if ctx.kind == "emu" and log_n > 16:
        pytest.skip("CPU suite time: 2^18 and 2^20 rows run on the GPU")
    trace, rnd, ev, want = case(log_n, h)
    mt = MasterTable(ctx, trace, rnd, ArithmeticDomain.of_length(1 << log_n), ev, ev, 1)
    mt.maybe_low_degree_extend_all_columns()
    got = mt.low_degree_extended_table()
    mt.clear_cache()
    assert got.shape == want.shape and (got < np.uint64(P)).all()
    assert (got == want).all()


def brev(values, bits):
    out = np.zeros_like(values)
    for i in range(bits):
        out |= ((values >> i) & 1) << (bits - 1 - i)
    return out


@pytest.mark.parametrize("h", [0, 5])
def test_split_at_the_coefficients(ctx, orc, case, h):
    log_n, n = 16, 1 << 16
    trace, rnd, ev, want = case(log_n, h)
    dom = ArithmeticDomain.of_length(n)
    mt = MasterTable(ctx, trace, rnd, dom, ev, ev, 1)
    # the inverse half: y[p n2 + q] = N c[brev(q) n1 + brev(p)] (csrc/ntt.hip, the coefficient form), c the interpolant
    coeffs = ctx.alloc(COLS * n)
    ctx._check(ctx.lib.tvm_lde_column_coefficients(ctx.handle, 1, mt.d_trace.ptr, n, COLS, dom.c(), 0, COLS, coeffs.ptr), "tvm_lde_column_coefficients")
    got = coeffs.download((COLS, n))
    assert (got < np.uint64(P)).all()
    log_n1 = log_n // 2
    n1, n2 = 1 << log_n1, 1 << (log_n - log_n1)
    p, q = np.divmod(np.arange(n, dtype=np.int64), n2)
    index = brev(q, log_n - log_n1) * n1 + brev(p, log_n1)
    for c in range(COLS):
        interpolant = [int(v) * n % P for v in orc.intt(trace[c])]
        assert got[c].tolist() == [interpolant[m] for m in index.tolist()], c
    # the forward half from those words
    t = C.c_void_p()
    ctx._check(ctx.lib.tvm_lde_table_begin(ctx.handle, 1, n, COLS, h, dom.c(), ev.c(), C.byref(t)), "tvm_lde_table_begin")
    mt._table = t.value
    ctx._check(ctx.lib.tvm_lde_table_add_columns(ctx.handle, t, coeffs.ptr, 0, COLS, mt.d_randomizers.ptr, h, dom.c(), ev.c()), "tvm_lde_table_add_columns")
    ctx._check(ctx.lib.tvm_lde_table_end(ctx.handle, t), "tvm_lde_table_end")
    table = mt.low_degree_extended_table()
    mt.clear_cache()
    coeffs.free()
    assert (table == want).all() and (table < np.uint64(P)).all()


@pytest.mark.gpu
def test_prove_fib_at_2p10_rows_still_hashes_to_the_pinned_digest(orc):
    from oracle.vm import workload
    from tests import test_proof_snapshot as snap
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.proof_stream import Proof
    from triton_vm_amd.prover import Claim

    with open(os.path.join(os.path.dirname(__file__), "golden", "combination_route_proof_digest.json")) as f:
        want = json.load(f)["fib:10:fri"]
    e = workload.execution("fib", 10)
    claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
    ctx = Context(device=0)
    try:
        proof = native_host.prove_execution(ctx, native_host.load_host_library(), e["aet"], e["padded_height"], claim,
                                            snap.prover_seed(want["seed_u64"]), ldt="fri")
        assert proof.size == want["proof_words"] and [int(w) for w in Proof(proof).digest(ctx.lib)] == want["digest"]
    finally:
        ctx.close()
