#!/usr/bin/env python3
"""What a stretch of the transcript on the device buys (TVMH_OPTION_DEVICE_FRONT, _MIDDLE, _TAIL, _STIR; each default off): prove_fib
through the C++ host (native_host.prove_execution), the same execution trace proved with the stage's options off and on, alternated
`rounds` times in this process on this box, the proofs compared every time and the counters checked.  Host wall time per proof: per
round the median of `runs` proofs after one warm-up.  Then, by stage (STAGES below):
  front   FRONT + MIDDLE + TAIL against all off, FRI; pieces != 0: the options one by one -- off, FRONT, MIDDLE, TAIL, FRONT + MIDDLE --
          alternated the same way, so that the file says which piece costs or buys what
  middle  MIDDLE, FRI; one proof each way under TVMH_OPTION_TRACE = 1 (the stream drained at every stage boundary) for the stages from
          the quotient's Merkle tree to DEEP
  tail    TAIL, FRI; the same for the FRI and opening stages
  stir    STIR, with STIR forced below 2^16 rows (the reference picks FRI there); the same for the STIR stage
The yardstick is option off in the same process and alternation; the bar for turning an option on is DESIGN.md 4.5's: on not slower
than off beyond the off runs' own spread at every height.
Usage: python tools/device_transcript_time.py stage=front|middle|tail|stir [rounds=3] [runs=5] [logs=10,12,14,16,20] [out=profiles/device_<stage>_time.txt] [pieces=1]
(the arguments after the stage by name or in this order; stir's default logs: 10,12,14,16,18,20)"""
import contextlib
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAN = float("nan")
MIDDLE_OFF = ("quotient Merkle", "out-of-domain rows", "linear combination", "DEEP")
MIDDLE_ON = ("quotient Merkle", "out-of-domain rows to DEEP")
TAIL = ("FRI", "open trace leafs")


def middle_lines(off, on):
    return [f"    stages, option off (stream drained per stage): out-of-domain rows {off['out-of-domain rows']:.3f} ms, linear combination "
            f"{off['linear combination']:.3f} ms; with quotient Merkle {off['quotient Merkle']:.3f} and DEEP {off['DEEP']:.3f} "
            f"the stretch is {sum(off.values()):.3f} ms",
            f"    stages, option on  (stream drained per stage): out-of-domain rows to DEEP {on['out-of-domain rows to DEEP']:.3f} ms; with quotient Merkle "
            f"{on['quotient Merkle']:.3f} the stretch is {sum(on.values()):.3f} ms"]


def tail_lines(off, on):
    return [f"    stages, option {name} (stream drained per stage): FRI {s['FRI']:.3f} ms, open trace leafs {s['open trace leafs']:.3f} ms"
            for name, s in (("off", off), ("on ", on))]


def stir_lines(off, on):
    return [f"    STIR stage (stream drained per stage): option off {off['STIR']:.3f} ms, on {on['STIR']:.3f} ms"]


# per stage: its options (native_host.OPTION_DEVICE_<name>; each has the counter tvmh_device_<name>_proofs), the low-degree test it
# proves with, its default logs, how its first line names off and on, the TVMH_OPTION_TRACE stages it reports with the options off / on,
# their keys in the JSON line (one key: the single stage's value, not a dict), the lines that report them, and the settings of `pieces`
STAGES = {
    "front": dict(options=("FRONT", "MIDDLE", "TAIL"), ldt="fri", logs="10,12,14,16,20", off="options off", on="FRONT + MIDDLE + TAIL on",
                  traced=None, pieces=(("off", ()), ("FRONT", ("FRONT",)), ("MIDDLE", ("MIDDLE",)), ("TAIL", ("TAIL",)),
                                       ("FRONT + MIDDLE", ("FRONT", "MIDDLE")))),
    "middle": dict(options=("MIDDLE",), ldt="fri", logs="10,12,14,16,20", off="option off", on="on",
                   traced=(MIDDLE_OFF, MIDDLE_ON, ("stages_off_ms", "stages_on_ms"), middle_lines)),
    "tail": dict(options=("TAIL",), ldt="fri", logs="10,12,14,16,20", off="option off", on="on",
                 traced=(TAIL, TAIL, ("stages_off_ms", "stages_on_ms"), tail_lines)),
    "stir": dict(options=("STIR",), ldt="stir", logs="10,12,14,16,18,20", off="option off", on="on",
                 traced=(("STIR",), ("STIR",), ("stir_stage_off_ms", "stir_stage_on_ms"), stir_lines)),
}


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


def main(stage, rounds="3", runs="5", logs=None, out=None, pieces="1"):
    import torch  # noqa: F401  (first: the ROCm runtime torch ships)

    from oracle.vm import workload
    from triton_vm_amd import Context, native_host
    from triton_vm_amd.master_table import aet_to_device
    from triton_vm_amd.proof_stream import Claim

    s = STAGES[stage]
    rounds, runs = int(rounds), int(runs)
    out = out or os.path.join(ROOT, "profiles", f"device_{stage}_time.txt")
    lines, result = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)
        with open(out, "w") as f:   # (rewritten as it grows: a run that is cut short leaves what it measured)
            f.write("\n".join(lines) + "\n")

    ctx = Context(device=0)
    lib = native_host.load_host_library()
    option = {name: getattr(native_host, "OPTION_DEVICE_" + name) for name in s["options"]}
    counters = [getattr(lib, f"tvmh_device_{name.lower()}_proofs") for name in s["options"]]
    seed = bytes(range(32))
    for log in (int(v) for v in str(logs or s["logs"]).split(",") if v):
        e = workload.execution("fib", log)
        claim = Claim(e["program_digest"], e["public_input"], e["public_output"])
        aet = aet_to_device(ctx, e["aet"])
        prove = lambda: native_host.prove_execution(ctx, lib, aet, e["padded_height"], claim, seed, ldt=s["ldt"])

        def timed(value, which=s["options"]):
            """`which` of the stage's options at `value` -> (median ms, every run's ms, the proof); the counters must say who ran"""
            with contextlib.ExitStack() as stack:
                for name in which:
                    stack.enter_context(native_host.host_option(lib, option[name], value))
                taken = [count() for count in counters]
                ms = []
                for _ in range(runs + 1):
                    t0 = time.perf_counter()
                    words = prove()
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert [count() - t for count, t in zip(counters, taken)] == [runs + 1 if value and name in which else 0 for name in s["options"]]
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
        say(f"prove_fib 2^{log} {s['ldt'].upper()}: {s['off']} {' '.join(f'{m:.3f}' for m, _ in off)} ms | {s['on']} "
            f"{' '.join(f'{m:.3f}' for m, _ in on)} ms per proof (median of {runs}, per round) | off runs span {spread[0]:.3f} .. {spread[1]:.3f} ms | "
            f"same proof words: {same}")
        if s["traced"]:
            stages = []
            for value, names, key in zip((0, 1), s["traced"][:2], s["traced"][2]):
                with contextlib.ExitStack() as stack:
                    for o in (*option.values(), native_host.OPTION_TRACE):
                        stack.enter_context(native_host.host_option(lib, o, 1 if o == native_host.OPTION_TRACE else value))
                    seen = traced(prove)[1]
                result[f"2^{log}"][key] = {k: seen.get(k) for k in names} if len(names) > 1 else seen.get(names[0])
                stages.append({k: seen.get(k, NAN) for k in names})
            for line in s["traced"][3](*stages):
                say(line)
        if int(pieces) and s.get("pieces"):
            one_by_one = {name: [] for name, _ in s["pieces"]}
            for _ in range(rounds):
                for name, which in s["pieces"]:
                    m, _, w = timed(1, which)
                    assert w.size == w_off.size and bool((w == w_off).all()), name
                    one_by_one[name].append(m)
            result[f"2^{log}"]["one_by_one_ms"] = one_by_one
            say("    one by one, same alternation: " + " | ".join(f"{name} {' '.join(f'{m:.3f}' for m in ms)}" for name, ms in one_by_one.items()) + " ms")
        ctx.trim()
    ctx.close()
    say(json.dumps(result))


if __name__ == "__main__":
    named = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    main(named.pop("stage"), *(a for a in sys.argv[1:] if "=" not in a), **named)
