#!/usr/bin/env python3
"""What TVMH_OPTION_DEVICE_MIDDLE buys: prove_fib with FRI at 2^10 .. 2^20 rows through the C++ host (native_host.prove_execution), the
same execution trace proved with the option off and on, alternated `rounds` times in this process on this box, the proofs compared
every time.  Host wall time per proof: per round the median of `runs` proofs after one warm-up; then one proof each way under
TVMH_OPTION_TRACE = 1 (the stream drained at every stage boundary) for the stages from the quotient's Merkle tree to DEEP.
The yardstick is option off in the same process and alternation; the bar for turning the option on is DESIGN.md 4.5's: on not slower
than off beyond the off runs' own spread at every height.
Usage: python tools/device_middle_time.py [rounds=3] [runs=5] [logs=10,12,14,16,20] [out=profiles/device_middle_time.txt]"""
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def traced(call):
    """call() with the process's stderr (the C++ host's trace lines) captured -> (result, {stage: ms})"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            result = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return result, {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[tvmh\]\s+(.*?)\s+([0-9.]+) ms", text)}


def main(rounds="3", runs="5", logs="10,12,14,16,20", out=os.path.join(ROOT, "profiles", "device_middle_time.txt")):
    import torch  # noqa: F401  (first: the ROCm runtime torch ships)

    from oracle.vm import workload
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.master_table import aet_to_device
    from triton_vm_amd.proof_stream import Claim

    rounds, runs = int(rounds), int(runs)
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
        prove = lambda: native_host.prove_execution(ctx, lib, aet, e["padded_height"], claim, seed, ldt="fri")

        def timed(option):
            with native_host.host_option(lib, native_host.OPTION_DEVICE_MIDDLE, option):
                taken = lib.tvmh_device_middle_proofs()
                ms = []
                for _ in range(runs + 1):
                    t0 = time.perf_counter()
                    words = prove()
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert lib.tvmh_device_middle_proofs() - taken == (runs + 1 if option else 0)
            return statistics.median(ms[1:]), ms[1:], words

        off, on, same = [], [], True
        for _ in range(rounds):
            m_off, all_off, w_off = timed(0)
            m_on, all_on, w_on = timed(1)
            same = same and w_off.size == w_on.size and bool((w_off == w_on).all())
            off.append((m_off, all_off))
            on.append((m_on, all_on))
        stages = {}
        for option in (0, 1):
            with native_host.host_option(lib, native_host.OPTION_DEVICE_MIDDLE, option), native_host.host_option(lib, native_host.OPTION_TRACE, 1):
                stages[option] = traced(prove)[1]
        spread = (min(min(a) for _, a in off), max(max(a) for _, a in off))
        names = ("quotient Merkle", "out-of-domain rows", "linear combination", "DEEP", "out-of-domain rows to DEEP")
        result[f"2^{log}"] = {"off_ms": [m for m, _ in off], "on_ms": [m for m, _ in on], "off_min_max_ms": spread, "same_proof": same,
                              "stages_off_ms": {k: stages[0].get(k) for k in names[:4]},
                              "stages_on_ms": {k: stages[1].get(k) for k in (names[0], names[4])}}
        say(f"prove_fib 2^{log} FRI: option off {' '.join(f'{m:.3f}' for m, _ in off)} ms | on {' '.join(f'{m:.3f}' for m, _ in on)} ms per proof "
            f"(median of {runs}, per round) | off runs span {spread[0]:.3f} .. {spread[1]:.3f} ms | same proof words: {same}")
        nan = float("nan")
        say(f"    stages, option off (stream drained per stage): out-of-domain rows {stages[0].get(names[1], nan):.3f} ms, linear combination "
            f"{stages[0].get(names[2], nan):.3f} ms; with quotient Merkle {stages[0].get(names[0], nan):.3f} and DEEP {stages[0].get(names[3], nan):.3f} "
            f"the stretch is {sum(stages[0].get(k, nan) for k in names[:4]):.3f} ms")
        say(f"    stages, option on  (stream drained per stage): out-of-domain rows to DEEP {stages[1].get(names[4], nan):.3f} ms; with quotient Merkle "
            f"{stages[1].get(names[0], nan):.3f} the stretch is {stages[1].get(names[0], nan) + stages[1].get(names[4], nan):.3f} ms")
        ctx.trim()
    ctx.close()
    say(json.dumps(result))


if __name__ == "__main__":
    main(*sys.argv[1:])
