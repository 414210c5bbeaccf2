"""bench.py's plain run and --dump-outputs on CPU (tests/bench_on_emulation.py: the fiber emulation of the kernel sources instead of
the GPU): the line holds the headline and none of what --full adds, and the dump is the proof the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_prints_the_headline_and_dumps_the_last_proof(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "bench_on_emulation.py"), "--steps", "2", "--warmup", "0", "--data", "synthetic",
           "--log2-rows", "3", "--trace-randomizers", "3", "--queries", "2", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config"} <= set(rec)
    assert rec["steps"] == 2 and rec["warmup"] == 0 and rec["higher_is_better"] is True
    assert rec["value"] == pytest.approx(8 * 652 / (rec["ms_per_step"] * 1e-3), rel=1e-3)   # 2^3 rows x 652 words per timed step
    assert not {"roofline", "roofline_valu", "stage_ms", "verified", "valid_trace_mode", "cpu_baseline"} & set(rec)

    halves = np.load(dump / "proof_words.npy")
    assert halves.dtype == np.float64 and halves.ndim == 2 and halves.shape[1] == 2 and len(halves) > 0
    assert (halves >= 0).all() and (halves < 2.0 ** 32).all() and (halves == np.floor(halves)).all()
    words = halves[:, 0].astype(np.uint64) | (halves[:, 1].astype(np.uint64) << np.uint64(32))
    from tests.emu_fixture import emu_context
    from triton_vm_amd.proof_stream import Proof

    ctx = emu_context()
    try:
        assert Proof(words).padded_height(ctx.lib) == 8
    finally:
        ctx.close()
