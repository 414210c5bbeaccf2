#!/usr/bin/env python3
"""What checking the AIR on the trace costs (tvm_check_constraints): the check alone at 2^20 and 2^22 rows, and the
proof of prove_fib at 2^20 rows (C++ host, FRI) in its three modes -- default (valid-trace AIR, unchecked), checked
(TVMH_OPTION_CHECK_TRACE) and exact (TVMH_OPTION_EXACT_AIR) -- by same-box alternation: round after round, one proof of each mode,
so that a drift of the box hits the three alike.  Host wall time; medians.
Usage: python tools/constraint_check_time.py [rounds=7] [check_logs=20,22]  -> a text report, and one JSON line at the end"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(rounds="7", check_logs="20,22"):
    import numpy as np
    import torch  # noqa: F401  (first: the ROCm runtime torch ships)

    from oracle.vm import workload
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.master_table import aet_to_device
    from triton_vm_amd.proof_stream import Claim

    rounds = int(rounds)
    result = {"check_ms": {}, "proof_ms": {}}
    ctx = Context(device=0)
    # 1. the check alone on synthetic traces (random words: every row fails the screen; capacity 0 lists none, so this is the device
    #    screen and the count -- what a valid trace costs, the compaction aside)
    ch = np.arange(63 * 3, dtype=np.uint64) + 1
    for log in (int(v) for v in str(check_logs).split(",") if v):
        n = 1 << log
        main, aux = ctx.synthetic(379 * n, 1), ctx.synthetic(91 * n * 3, 2)
        times = []
        for k in range(rounds + 1):
            ctx.sync()
            t0 = time.perf_counter()
            failing, _ = ctx.check_constraints(main, aux, n, ch, capacity=0)
            times.append((time.perf_counter() - t0) * 1e3)
            assert failing == n
        result["check_ms"][f"2^{log}"] = statistics.median(times[1:])
        print(f"tvm_check_constraints 2^{log} rows: median {statistics.median(times[1:]):.2f} ms  (runs: {' '.join(f'{t:.2f}' for t in times[1:])})",
              flush=True)
        main.free()
        aux.free()
    ctx.trim()
    # 2. the proofs of prove_fib at 2^20 rows, the three modes alternating
    e = workload.execution("fib", 20)
    claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
    lib = native_host.load_host_library()
    aet = aet_to_device(ctx, e["aet"])
    seed = bytes(range(32))
    modes = {"default": (0, 0), "checked": (0, 1), "exact": (1, 0)}
    saved = {o: lib.tvmh_get_option(o) for o in (native_host.OPTION_EXACT_AIR, native_host.OPTION_CHECK_TRACE)}
    times, proofs = {m: [] for m in modes}, {}
    try:
        for r in range(rounds + 1):
            for m, (exact, check) in modes.items():
                lib.tvmh_set_option(native_host.OPTION_EXACT_AIR, exact)
                lib.tvmh_set_option(native_host.OPTION_CHECK_TRACE, check)
                ctx.sync()
                t0 = time.perf_counter()
                words = native_host.prove_execution(ctx, lib, aet, e["padded_height"], claim, seed, ldt="fri")
                times[m].append((time.perf_counter() - t0) * 1e3)
                proofs.setdefault(m, words)
    finally:
        for o, v in saved.items():
            lib.tvmh_set_option(o, v)
    same = all(p.size == proofs["default"].size and (p == proofs["default"]).all() for p in proofs.values())
    for m in modes:
        result["proof_ms"][m] = statistics.median(times[m][1:])
        print(f"prove_fib 2^20 rows, {m:8s}: median {result['proof_ms'][m]:.1f} ms  (runs: {' '.join(f'{t:.1f}' for t in times[m][1:])})",
              flush=True)
    print(f"the three modes give the same proof of this valid trace: {same}")
    result["same_proof"] = bool(same)
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main(*sys.argv[1:])
