"""tvm_check_constraints -- the AIR on the trace itself (triton_constraints_evaluate_to_zero, stark.rs:2849-3016) -- against the
oracle's restatement of it (vm_fixture.constraint_violations, orc.air_constraint_values), and the C++ host's checked proving
(TVMH_OPTION_CHECK_TRACE) and tvmh_check_execution."""
import os

import numpy as np
import pytest

from triton_vm_amd import native_host
from triton_vm_amd.capi import CONSTRAINT_SECTIONS

SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))


def _applicable(row, n):
    return [(name, a, b) for name, a, b in CONSTRAINT_SECTIONS
            if name == "cons" or (name == "init" and row == 0) or (name == "tran" and row < n - 1) or (name == "term" and row == n - 1)]


def _oracle_report(orc, main, aux, ch, rows):
    """[(row, section, index)] of the applicable non-zero constraints of `rows`, ascending"""
    n = main.shape[1]
    mr, ar = np.ascontiguousarray(main.T), np.ascontiguousarray(aux.transpose(1, 0, 2))
    out = []
    for r in sorted(rows):
        v = orc.air_constraint_values(mr[r], mr[(r + 1) % n], ar[r], ar[(r + 1) % n], ch)
        out += [(r, name, i) for name, a, b in _applicable(r, n) for i in range(a, b) if v[i].any()]
    return out


def _check(ctx, main, aux, ch, seed=SEED_A, capacity=4096):
    n = main.shape[1]
    dm, da = ctx.to_device(main), ctx.to_device(aux)
    try:
        return ctx.check_constraints(dm, da, n, ch.reshape(-1), seed=seed, capacity=capacity)
    finally:
        dm.free()
        da.free()


def _corrupt(rng, main, aux, cells):
    """cells: (table, column, row) -> copies of the tables with those cells replaced by random canonical words"""
    main, aux = main.copy(), aux.copy()
    for table, col, row in cells:
        if table == "main":
            main[col, row] = int(rng.integers(1, 1 << 63))
        else:
            aux[col, row] = rng.integers(1, 1 << 63, 3, dtype=np.uint64)
    return main, aux


@pytest.fixture(scope="module")
def tables():
    from tests import vm_fixture as vf

    return {which: vf.valid_tables(which) for which in ("tiny", "every")}


@pytest.mark.parametrize("which", ["tiny", "every"])
def test_valid_tables_have_no_failing_row(ctx, tables, which):
    main, aux, ch, _ = tables[which]
    assert _check(ctx, main, aux, ch) == (0, [])
    ctx.air_check_chunk_rows(16)   # many chunks: every chunk boundary's successor row
    try:
        assert _check(ctx, main, aux, ch, seed=None) == (0, [])
    finally:
        ctx.air_check_chunk_rows(0)


@pytest.mark.parametrize("chunk", [0, 64])
def test_corrupted_cells_are_reported_by_row_section_and_index(ctx, orc, tables, chunk):
    """main and aux cells at row 0, row n-1 and either side of a chunk boundary (chunk = 64 rows): the (row, section) set is the oracle's
    constraint_violations, the indices of every row the non-zero applicable entries of orc.air_constraint_values"""
    from tests import vm_fixture as vf

    main, aux, ch, _ = tables["tiny"]
    n = main.shape[1]
    rng = np.random.default_rng(7 + chunk)
    cells = [("main", 12, 0), ("aux", 5, 0), ("main", 200, 63), ("aux", 30, 64), ("main", 3, 127), ("aux", 60, 128), ("main", 40, n - 1),
             ("aux", 2, n - 1), ("main", 150, n // 2 + 5)]
    bad_main, bad_aux = _corrupt(rng, main, aux, cells)
    ctx.air_check_chunk_rows(chunk)
    try:
        failing, report = _check(ctx, bad_main, bad_aux, ch)
    finally:
        ctx.air_check_chunk_rows(0)
    want_sections = vf.constraint_violations(bad_main, bad_aux, ch)
    assert sorted({(r, s) for r, s, _ in report}) == sorted(want_sections)
    rows = sorted({r for r, _ in want_sections})
    assert failing == len(rows)
    assert report == _oracle_report(orc, bad_main, bad_aux, ch, rows)
    # the lowest rows first, ascending by row, then by index
    assert report == sorted(report, key=lambda e: (e[0], e[2]))
    assert rows[0] == 0 and rows[-1] == n - 1


def test_failing_row_count_is_exact_and_the_capacity_keeps_the_lowest_rows(ctx, orc, tables):
    main, aux, ch, _ = tables["every"]
    n = main.shape[1]
    rng = np.random.default_rng(3)
    rows = sorted(rng.choice(n, 23, replace=False).tolist())
    bad_main, bad_aux = _corrupt(rng, main, aux, [("main" if k % 2 else "aux", int(rng.integers(0, 90)), r) for k, r in enumerate(rows)])
    from tests import vm_fixture as vf

    want_rows = sorted({r for r, _ in vf.constraint_violations(bad_main, bad_aux, ch)})
    want = _oracle_report(orc, bad_main, bad_aux, ch, want_rows)
    ctx.air_check_chunk_rows(32)
    try:
        full = _check(ctx, bad_main, bad_aux, ch)
        assert full == (len(want_rows), want)
        # a small capacity: the first entries of the full report -- the lowest rows, ascending
        for capacity in (1, 5, 17):
            assert _check(ctx, bad_main, bad_aux, ch, capacity=capacity) == (len(want_rows), want[:capacity])
        # another seed for the screen's weights: the same report
        assert _check(ctx, bad_main, bad_aux, ch, seed=SEED_B) == full
    finally:
        ctx.air_check_chunk_rows(0)


def test_random_tables_fail_on_every_row(ctx, orc):
    rng = np.random.default_rng(11)
    n = 64
    main, aux, ch = orc.random_elements(rng, (379, n)), orc.random_elements(rng, (91, n, 3)), orc.random_elements(rng, (63, 3))
    failing, report = _check(ctx, main, aux, ch, capacity=1 << 16)
    assert failing == n
    assert report == _oracle_report(orc, main, aux, ch, range(n))
    failing2, first = _check(ctx, main, aux, ch, seed=SEED_B, capacity=10)
    assert failing2 == n and first == report[:10]


def test_check_constraints_rejects_bad_arguments(ctx, tables):
    from triton_vm_amd.capi import TritonHipError

    main, aux, ch, _ = tables["tiny"]
    dm, da = ctx.to_device(main), ctx.to_device(aux)
    with pytest.raises(TritonHipError):
        ctx.check_constraints(dm, da, main.shape[1] - 1, ch.reshape(-1))   # not a power of two
    with pytest.raises(TritonHipError):
        ctx.air_check_chunk_rows(100)   # not a power of two


def _host_library(ctx):
    backend = ctx.lib._name
    if ctx.kind == "emu":
        return native_host.load_host_library(backend, os.path.join(os.path.dirname(backend), "libtriton_host_emu.so"))
    return native_host.load_host_library(backend)


def test_check_execution_of_the_snapshot_program(ctx, orc):
    """tvmh_check_execution: the device's fill, pad and extend of a real execution pass the AIR; a wrong public output in the claim
    fails on the last row only, in terminal constraints -- those the host evaluation of that row pair finds"""
    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays

    lib = _host_library(ctx)
    program, aet, public_input, output = vf.run("tiny")
    claim = snap.claim_of(orc, program, public_input, output)
    arrays, n = aet_arrays(orc, aet), aet.padded_height()
    assert native_host.check_execution(ctx, lib, arrays, n, claim, SEED_A) == (0, [])
    claim.output = np.append(claim.output, np.uint64(12345))   # an output the program does not write
    failing, report = native_host.check_execution(ctx, lib, arrays, n, claim, SEED_A)
    assert failing == 1 and report and {(r, s) for r, s, _ in report} == {(n - 1, "term")}


def test_sharded_prover_refuses_the_check_option(ctx, orc):
    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays

    lib = _host_library(ctx)
    program, aet, public_input, output = vf.run("tiny")
    with native_host.host_option(lib, native_host.OPTION_CHECK_TRACE, 1):
        with pytest.raises(native_host.NativeHostError) as e:
            native_host.prove_execution_sharded(ctx, lib, None, aet_arrays(orc, aet), aet.padded_height(),
                                                snap.claim_of(orc, program, public_input, output), snap.prover_seed(snap.SEED_U64),
                                                jit_passes=1)
        assert e.value.status == 4
    assert lib.tvmh_get_option(native_host.OPTION_CHECK_TRACE) == 0


def test_checked_proof_of_a_valid_trace_is_the_default_proof(ctx, orc):
    from tests import test_proof_snapshot as snap
    from tests import vm_fixture as vf
    from tests.test_fill import aet_arrays
    from triton_vm_amd.proof_stream import Proof

    lib = _host_library(ctx)
    program, aet, public_input, output = vf.run("tiny")
    with native_host.host_option(lib, native_host.OPTION_CHECK_TRACE, 1):
        words = native_host.prove_execution(ctx, lib, aet_arrays(orc, aet), aet.padded_height(),
                                            snap.claim_of(orc, program, public_input, output), snap.prover_seed(snap.SEED_U64))
    assert Proof(words).digest(ctx.lib) == snap.SNAPSHOT


# ---- GPU: the headline trace ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fib20():
    from oracle.vm import workload

    return workload.execution("fib", 20)


def _claim(e, output=None):
    from triton_vm_amd.prover import Claim

    return Claim(e["program_digest"], e["public_input"], e["public_output"] if output is None else output)


def _wrong_output(e):
    out = np.array(e["public_output"], np.uint64).copy()
    out[0] = (int(out[0]) + 12345) % ((1 << 64) - (1 << 32) + 1)
    return out


@pytest.mark.gpu
def test_fib_2p20_trace_from_the_device_passes_and_a_wrong_output_fails_in_terminal_constraints(orc, fib20):
    from triton_vm_amd import Context

    ctx = Context(device=0)
    try:
        lib = native_host.load_host_library()
        n = fib20["padded_height"]
        assert native_host.check_execution(ctx, lib, fib20["aet"], n, _claim(fib20), SEED_A) == (0, [])
        failing, report = native_host.check_execution(ctx, lib, fib20["aet"], n, _claim(fib20, _wrong_output(fib20)), SEED_A)
        assert failing == 1 and report
        assert {r for r, _, _ in report} == {n - 1} and {s for _, s, _ in report} == {"term"}
        # the indices are the applicable non-zero constraints of the host evaluation of that row pair: the device trace of the same
        # seed, downloaded row by row, through the oracle's AIR
        assert all(581 <= i < 604 for _, _, i in report)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_checked_proving_falls_back_to_the_exact_proof_on_an_invalid_trace(fib20):
    from triton_vm_amd import Context
    from tests import test_proof_snapshot as snap

    ctx = Context(device=0)
    lib = native_host.load_host_library()
    saved = {o: lib.tvmh_get_option(o) for o in (native_host.OPTION_EXACT_AIR, native_host.OPTION_CHECK_TRACE)}
    seed = snap.prover_seed(snap.SEED_U64)
    n = fib20["padded_height"]

    def prove(claim, exact=0, check=0):
        lib.tvmh_set_option(native_host.OPTION_EXACT_AIR, exact)
        lib.tvmh_set_option(native_host.OPTION_CHECK_TRACE, check)
        return native_host.prove_execution(ctx, lib, fib20["aet"], n, claim, seed, ldt="fri")

    try:
        wrong = _claim(fib20, _wrong_output(fib20))
        checked, exact, default = prove(wrong, check=1), prove(wrong, exact=1), prove(wrong)
        assert checked.size == exact.size and (checked == exact).all()
        assert default.size != exact.size or not (default == exact).all()
        right = _claim(fib20)
        assert (prove(right, check=1) == prove(right)).all()
    finally:
        for o, v in saved.items():
            lib.tvmh_set_option(o, v)
        ctx.close()
