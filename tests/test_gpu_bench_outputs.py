"""A plain bench.py run times its steps and nothing else (the profile pass and
the CPU baseline belong to --full), keeps the result line's fields, and with
--dump-outputs writes the last timed step's disparity map: bit for bit what a
handle computes from the same synthetic pair."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from stereo_matching_amd import SGM, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_last_map(tmp_path):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] == bench.METRIC and rec["unit"] == "Mpixel-disparities/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == 3 and rec["warmup"] == 1
    cfg = bench.CONFIGS["k128"]
    h, w, D = cfg["h"], cfg["w"], cfg["D"]
    # value and ms_per_step describe the same timed region (both are rounded in the line)
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(h * w * D / (rec["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert abs(rec["rank_timed_s"]["max"] * 1e3 / 3 - rec["ms_per_step"]) < 1e-3 * rec["ms_per_step"] + 1e-3
    # only the warm-up and the timed steps ran
    assert rec["frames_verified"] == ["warmup", "timed"]
    assert rec["roofline"] is None and rec["kernels"] == {} and rec["cpu_baseline"] is None

    assert sorted(os.listdir(out)) == ["disparity.npy"]
    got = np.load(out / "disparity.npy")
    assert got.dtype == np.float32 and got.shape == (h, w)
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    with SGM(h, w, 1, D, views=cfg["views"]) as sgm:
        sgm.process(left, right)
        sgm.check()
        want = sgm.get_lr_disp().copy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
