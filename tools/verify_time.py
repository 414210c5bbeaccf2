#!/usr/bin/env python3
"""What verifying a proof costs: prove_fib at 2^16 and 2^20 rows, FRI and STIR -- proved once (C++ host), then the same proof verified
by (i) the native verifier (native_host.verify: triton_vm::Verifier, per-query work on the device) and (ii) the Python product
verifier (triton_vm_amd.verifier.Verifier), in this process on this box.  Host wall time; one warm-up, then the median of `runs`
runs (the Python verifier: `python_runs`, it takes seconds to minutes).  Prints the native verifier's split by stage.
Usage: python tools/verify_time.py [runs=5] [logs=16,20] [python_runs=5] [out=profiles/r09_verify_time.txt]

Batch mode -- python tools/verify_time.py batch [logs=16,20] [out=profiles/verify_batch_time.txt] -- compares, for the same proofs, a loop
of K tvmh_verify calls with ONE tvmh_verify_batch of K jobs (native_host.verify_batch_verdicts): K = 1, 16 and 64 copies of each proof,
and one mixed batch (every proof once: FRI and STIR, the heights given).  After a warm-up of both, the two alternate five times in this
process; per-proof wall time of every run, its range, and the batch's stage split.  The project's reading: the batch is faster only where
its slowest run is below the loop's fastest."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(runs="5", logs="16,20", python_runs="5", out=os.path.join(ROOT, "profiles", "r09_verify_time.txt")):
    import torch  # noqa: F401  (first: the ROCm runtime torch ships)

    from oracle.vm import workload
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.master_table import aet_to_device
    from triton_vm_amd.proof_stream import Claim
    from triton_vm_amd.verifier import Verifier

    runs, python_runs = int(runs), int(python_runs)
    lines, result = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)
        with open(out, "w") as f:   # (rewritten as it grows: a run that is cut short leaves what it measured)
            f.write("\n".join(lines) + "\n")

    ctx = Context(device=0)
    lib = native_host.load_host_library()
    seed = bytes(range(32))
    for log in (int(v) for v in str(logs).split(",") if v):
        e = workload.execution("fib", log)
        claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
        aet = aet_to_device(ctx, e["aet"])
        for ldt in ("fri", "stir"):
            words = native_host.prove_execution(ctx, lib, aet, e["padded_height"], claim, seed, ldt=ldt)
            native_ms, stages = [], []
            for _ in range(runs + 1):
                t0 = time.perf_counter()
                rc, verdict, name, native_indices, split = native_host.verify_verdict(ctx, lib, claim, words, ldt=ldt)
                native_ms.append((time.perf_counter() - t0) * 1e3)
                stages.append(split)
                assert rc == 0 and verdict == 0, (rc, verdict, name)
            python_ms, python_indices = [], None
            for _ in range(python_runs + 1):
                t0 = time.perf_counter()
                python_indices = Verifier(ctx, ldt=ldt).verify(claim, words)
                python_ms.append((time.perf_counter() - t0) * 1e3)
            n, p = statistics.median(native_ms[1:]), statistics.median(python_ms[1:])
            same = native_indices == python_indices
            key = f"2^{log} {ldt}"
            result[key] = {"native_ms": n, "python_ms": p, "ratio": p / n, "same_indices": same, "proof_words": int(words.size)}
            say(f"prove_fib {key:10s} ({words.size} proof words): native {n:8.2f} ms | Python {p:10.1f} ms | x{p / n:7.1f} | both accept, "
                f"indices equal: {same}")
            say(f"    native runs: {' '.join(f'{t:.2f}' for t in native_ms[1:])}   Python runs: {' '.join(f'{t:.0f}' for t in python_ms[1:])}")
            say("    native split (median ms): " + ", ".join(
                f"{stage} {statistics.median(s[stage] for s in stages[1:]):.2f}" for stage in native_host.VERIFY_STAGES))
        ctx.trim()
    ctx.close()
    say(json.dumps(result))


def batch_main(logs="16,20", out=os.path.join(ROOT, "profiles", "verify_batch_time.txt"), rounds="5"):
    import torch  # noqa: F401  (first: the ROCm runtime torch ships)

    from oracle.vm import workload
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.master_table import aet_to_device
    from triton_vm_amd.proof_stream import Claim

    rounds = int(rounds)
    lines, result = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)
        with open(out, "w") as f:   # (rewritten as it grows: a run that is cut short leaves what it measured)
            f.write("\n".join(lines) + "\n")

    ctx = Context(device=0)
    lib = native_host.load_host_library()
    seed = bytes(range(32))
    proofs = {}
    for log in (int(v) for v in str(logs).split(",") if v):
        e = workload.execution("fib", log)
        claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
        aet = aet_to_device(ctx, e["aet"])
        for ldt in ("fri", "stir"):
            proofs[f"2^{log} {ldt}"] = (claim, native_host.prove_execution(ctx, lib, aet, e["padded_height"], claim, seed, ldt=ldt), ldt)
        del aet
        ctx.trim()

    def loop(jobs):
        t0 = time.perf_counter()
        for claim, words, _, _, ldt in jobs:
            rc, verdict, name, _, _ = native_host.verify_verdict(ctx, lib, claim, words, ldt=ldt)
            assert rc == 0 and verdict == 0, (rc, verdict, name)
        return (time.perf_counter() - t0) * 1e3 / len(jobs)

    def batch(jobs):
        t0 = time.perf_counter()
        rc, error, verdicts, _, _, stages = native_host.verify_batch_verdicts(ctx, lib, jobs)
        ms = (time.perf_counter() - t0) * 1e3 / len(jobs)
        assert rc == 0 and not any(verdicts), (rc, error, verdicts)
        return ms, stages

    def compare(key, jobs):
        loop(jobs), batch(jobs)   # the warm-up of both
        loop_ms, batch_ms, stages = [], [], []
        for _ in range(rounds):
            loop_ms.append(loop(jobs))
            ms, split = batch(jobs)
            batch_ms.append(ms)
            stages.append(split)
        faster = max(batch_ms) < min(loop_ms)
        slower = min(batch_ms) > max(loop_ms)
        reading = "batch faster" if faster else "batch slower" if slower else "no difference beyond the runs' spread"
        result[key] = {"jobs": len(jobs), "loop_ms_per_proof": loop_ms, "batch_ms_per_proof": batch_ms, "reading": reading}
        say(f"{key:22s} K={len(jobs):3d}: loop {min(loop_ms):7.3f}..{max(loop_ms):7.3f} ms/proof | batch {min(batch_ms):7.3f}..{max(batch_ms):7.3f} "
            f"ms/proof | {reading}" + (f" (x{min(loop_ms) / max(batch_ms):.2f} at the least)" if faster else ""))
        say(f"    loop runs: {' '.join(f'{t:.3f}' for t in loop_ms)}   batch runs: {' '.join(f'{t:.3f}' for t in batch_ms)}")
        say("    batch split (median ms per proof): " + ", ".join(
            f"{stage} {statistics.median(s[stage] for s in stages) / len(jobs):.3f}" for stage in native_host.VERIFY_STAGES))

    say(f"tvmh_verify in a loop against one tvmh_verify_batch, host wall time per proof, {rounds} alternating runs after a warm-up of both")
    for key, (claim, words, ldt) in proofs.items():
        for k in (1, 16, 64):
            compare(f"prove_fib {key}", [native_host.verify_job(claim, words, ldt=ldt)] * k)
    compare("mixed: " + ", ".join(proofs), [native_host.verify_job(claim, words, ldt=ldt) for claim, words, ldt in proofs.values()])
    ctx.close()
    say(json.dumps(result))


if __name__ == "__main__":
    if sys.argv[1:2] == ["batch"]:
        batch_main(*sys.argv[2:])
    else:
        main(*sys.argv[1:])
