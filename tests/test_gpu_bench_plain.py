"""bench.py's plain run (no --full): ONE JSON line with the contract's keys and nothing measured beside the headline, `--steps` timed steps,
and `--dump-outputs DIR`: the last timed step's SADs as float32 .npy files, identical from run to run and equal to the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H, BORDER, FRAMES, SR = 1920, 1080, 160, 4, 64


def plain_run(out_dir):
    env = dict(os.environ, AOMHIP_BENCH_RAMP_S="0.02")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames-per-gpu", str(FRAMES),
                        "--dump-outputs", str(out_dir)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON line"
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path, oracle, hip):
    d = plain_run(tmp_path / "a")
    assert d["metric"] == "SAD-candidates/s" and d["unit"] == "candidates/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["workload"] == "sad16x16_modeA_1080p_8bit" and d["config"]["ring_frame_pairs_per_gpu"] == FRAMES
    n = (W // 16) * (H // 16)
    assert d["config"]["candidates_per_step"] == 5 * n * FRAMES
    # candidates/s and ms per step describe the same timed steps
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / d["config"]["candidates_per_step"] - 1) < 1e-3
    for k in ("roofline", "cpu_baseline", "others", "txq", "strong_scaling_search", "full_record"):
        assert k not in d, k   # measured with --full only

    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert set(a) == {"sad_single.npy", "sad_x4d.npy"}
    assert a["sad_single.npy"].shape == (FRAMES, n) and a["sad_x4d.npy"].shape == (FRAMES, n, 4)
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20

    # the same arguments -> the same inputs -> the same outputs
    plain_run(tmp_path / "b")
    for f, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f)), f

    # what the oracle computes on the ring's inputs (benchlib/sad.py SadModeA, seed 1): first and last slot
    synth = hip.synth
    cands, groups = synth.mode_a_worklist(W, H, 16, seed=1, search=SR)
    rng = np.random.default_rng(1)
    allg = np.tile(groups, (FRAMES, 1))
    allg["rx"] = allg["sx"][..., None] + rng.integers(-SR, SR + 1, (FRAMES, n, 4), dtype=np.int16)
    allg["ry"] = allg["sy"][..., None] + rng.integers(-SR, SR + 1, (FRAMES, n, 4), dtype=np.int16)
    for slot in (0, FRAMES - 1):
        sb = oracle.extend_plane(synth.lcg_frame(W, H, 2 * slot, 0, 8), BORDER)
        rb = oracle.extend_plane(synth.lcg_frame(W, H, 2 * slot + 1, 0, 8), BORDER)
        assert np.array_equal(a["sad_single.npy"][slot], oracle.sad_batch(sb, rb, BORDER, 16, 16, cands, bd=8, threads=4).astype(np.float32))
        assert np.array_equal(a["sad_x4d.npy"][slot], oracle.sad_x4d_batch(sb, rb, BORDER, 16, 16, allg[slot], bd=8, threads=4).astype(np.float32))
