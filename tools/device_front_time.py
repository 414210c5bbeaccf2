#!/usr/bin/env python3
"""What the transcript on the device buys from the main root to the trace openings: prove_fib with FRI at 2^10 .. 2^20 rows through the
C++ host (native_host.prove_execution), the same execution trace proved with every option off and with TVMH_OPTION_DEVICE_FRONT +
TVMH_OPTION_DEVICE_MIDDLE + TVMH_OPTION_DEVICE_TAIL on, alternated `rounds` times in this process on this box, the proofs compared
every time.  Host wall time per proof: per round the median of `runs` proofs after one warm-up.  Then (pieces != 0) the options one by
one -- off, FRONT, MIDDLE, TAIL, FRONT + MIDDLE -- alternated the same way, so that the file says which piece costs or buys what.
The yardstick is option off in the same process and alternation; the bar for turning the options on is DESIGN.md 4.5's: on not slower
than off beyond the off runs' own spread at every height.
Usage: python tools/device_front_time.py [rounds=3] [runs=5] [logs=10,12,14,16,20] [out=profiles/device_front_time.txt] [pieces=1]"""
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(rounds="3", runs="5", logs="10,12,14,16,20", out=os.path.join(ROOT, "profiles", "device_front_time.txt"), pieces="1"):
    import torch  # noqa: F401  (first: the ROCm runtime torch ships)

    from oracle.vm import workload
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.master_table import aet_to_device
    from triton_vm_amd.proof_stream import Claim

    rounds, runs = int(rounds), int(runs)
    lines, result = [], {}
    options = (native_host.OPTION_DEVICE_FRONT, native_host.OPTION_DEVICE_MIDDLE, native_host.OPTION_DEVICE_TAIL)

    def say(text):
        print(text, flush=True)
        lines.append(text)
        with open(out, "w") as f:   # (rewritten as it grows: a run that is cut short leaves what it measured)
            f.write("\n".join(lines) + "\n")

    ctx = Context(device=0)
    lib = native_host.load_host_library()
    counters = (lib.tvmh_device_front_proofs, lib.tvmh_device_middle_proofs, lib.tvmh_device_tail_proofs)
    seed = bytes(range(32))
    for log in (int(v) for v in str(logs).split(",") if v):
        e = workload.execution("fib", log)
        claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
        aet = aet_to_device(ctx, e["aet"])
        prove = lambda: native_host.prove_execution(ctx, lib, aet, e["padded_height"], claim, seed, ldt="fri")

        def timed(value, which=options):
            """`which` of the three options at `value` -> (median ms, every run's ms, the proof); the counters must say who ran"""
            with contextlib.ExitStack() as stack:
                for o in which:
                    stack.enter_context(native_host.host_option(lib, o, value))
                taken = [count() for count in counters]
                ms = []
                for _ in range(runs + 1):
                    t0 = time.perf_counter()
                    words = prove()
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert [count() - t for count, t in zip(counters, taken)] == [runs + 1 if value and o in which else 0 for o in options]
            return statistics.median(ms[1:]), ms[1:], words

        off, on, same = [], [], True
        for _ in range(rounds):
            m_off, all_off, w_off = timed(0)
            m_on, all_on, w_on = timed(1)
            same = same and w_off.size == w_on.size and bool((w_off == w_on).all())
            off.append((m_off, all_off))
            on.append((m_on, all_on))
        spread = (min(min(a) for _, a in off), max(max(a) for _, a in off))
        result[f"2^{log}"] = {"off_ms": [m for m, _ in off], "on_ms": [m for m, _ in on], "off_min_max_ms": spread, "same_proof": same}
        say(f"prove_fib 2^{log} FRI: options off {' '.join(f'{m:.3f}' for m, _ in off)} ms | FRONT + MIDDLE + TAIL on "
            f"{' '.join(f'{m:.3f}' for m, _ in on)} ms per proof (median of {runs}, per round) | off runs span {spread[0]:.3f} .. {spread[1]:.3f} ms | "
            f"same proof words: {same}")
        if int(pieces):
            front, middle, tail = options
            settings = (("off", ()), ("FRONT", (front,)), ("MIDDLE", (middle,)), ("TAIL", (tail,)), ("FRONT + MIDDLE", (front, middle)))
            one_by_one = {name: [] for name, _ in settings}
            for _ in range(rounds):
                for name, which in settings:
                    m, _, w = timed(1, which)
                    assert w.size == w_off.size and bool((w == w_off).all()), name
                    one_by_one[name].append(m)
            result[f"2^{log}"]["one_by_one_ms"] = one_by_one
            say("    one by one, same alternation: " + " | ".join(f"{name} {' '.join(f'{m:.3f}' for m in ms)}" for name, ms in one_by_one.items()) + " ms")
        ctx.trim()
    ctx.close()
    say(json.dumps(result))


if __name__ == "__main__":
    main(*sys.argv[1:])
