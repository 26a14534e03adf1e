"""The launch ledger of the volume frames: sgm_aggregate_device, the frames of
SAD / SSD handles and filter_volume.

As tests/test_gpu_launch_ledger.py does for the census schedules: with
profiling on, one frame (or one filter_volume call) leaves {class: (launches,
elements per launch)} in get_profile(), compared exactly with a recorded table.
Every case runs at 20 x 40, D = 32, scale 1, the smallest shape every launch
here accepts: a ledger counts launches, so nothing larger is needed.

The table was recorded from the library as it was before volume_frame and
frame_maps came to share their frame tail (`python
tests/test_gpu_volume_ledger.py` prints it).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from stereo_matching_amd import SGM

pytestmark = pytest.mark.gpu

SWITCHES = ("SGM_BAND_ROWS", "SGM_SLANT", "SGM_VSTRIP", "SGM_P4_HPAIR", "SGM_CONFIDENCE")
H, W, D = 20, 40, 32

# name: (entry, constructor keywords, (horizontal, vertical) filter or None for the handle's default,
# cost kind, weighted)
CASES = {
    "aggregate_v1": ("aggregate", {"views": 1}, None, None, False),
    "aggregate_v2_h": ("aggregate", {}, (True, False), None, False),
    "aggregate_v2_v": ("aggregate", {}, (False, True), None, False),
    "aggregate_v2_hv": ("aggregate", {}, (True, True), None, False),
    "aggregate_v1_paths4_hv": ("aggregate", {"views": 1, "paths": 4}, (True, True), None, False),
    "sad_v1": ("frame", {"views": 1}, None, "sad", False),
    "sad_v2_v": ("frame", {}, (False, True), "sad", False),
    "ssd_v2_weighted": ("frame", {}, None, "ssd", True),
    "filter_volume_v": ("filter_volume", {"views": 1}, (False, True), None, False),
}

LEDGERS = {
    "aggregate_v1": {
        "vol_import": (1, 25600.0),
        "pair_fwd_L3": (1, 25600.0),
        "stage_a": (1, 25600.0),
        "stage_b": (1, 25600.0),
        "sweep_L8_acc": (1, 25600.0),
        "pair_bwd_L4_final": (1, 25600.0),
    },
    "aggregate_v2_h": {
        "vol_import": (1, 51200.0),
        "vol_hfilter": (1, 51200.0),
        "pair_fwd_L3": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    },
    "aggregate_v2_v": {
        "vol_import": (1, 51200.0),
        "vfwd": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    },
    "aggregate_v2_hv": {
        "vol_import": (1, 51200.0),
        "vol_hfilter": (1, 51200.0),
        "vfwd": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    },
    "aggregate_v1_paths4_hv": {
        "vol_import": (1, 25600.0),
        "vol_hfilter": (1, 25600.0),
        "vfwd": (1, 25600.0),
        "hpair4_fwd": (1, 25600.0),
        "hpair4_bwd": (1, 25600.0),
        "final4": (1, 25600.0),
    },
    "sad_v1": {
        "window_cost": (1, 25600.0),
        "pair_fwd_L3": (1, 25600.0),
        "stage_a": (1, 25600.0),
        "stage_b": (1, 25600.0),
        "sweep_L8_acc": (1, 25600.0),
        "pair_bwd_L4_final": (1, 25600.0),
    },
    "sad_v2_v": {
        "window_cost": (1, 25600.0),
        "vol_import": (1, 25600.0),
        "vfwd": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    },
    "ssd_v2_weighted": {
        "window_cost_weighted": (1, 25600.0),
        "vol_import": (1, 25600.0),
        "pair_fwd_L3": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    },
    "filter_volume_v": {
        "vol_copy": (1, 25600.0),
        "vfwd": (1, 25600.0),
    },
}


def _ledger(name):
    """One frame, or one filter_volume call, of case `name`."""
    import torch
    entry, kw, filt, kind, weighted = CASES[name]
    rng = np.random.default_rng(5)
    with SGM(H, W, 1, D, **kw) as s:
        if kind:
            s.set_cost(kind)
        if weighted:
            s.set_weighted(True)
        if filt and entry != "filter_volume":
            s.set_volume_filter(*filt)
        s.set_profiling(True)
        if entry == "frame":
            left, right = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
            s.process(left, right)
        else:
            cost = torch.from_numpy(rng.integers(0, 64, (H, W, D)).astype(np.float32)).to(f"cuda:{s.device}")
            if entry == "aggregate":
                s.aggregate(cost)
            else:
                s.filter_volume(cost, *filt)
            torch.cuda.synchronize()
        prof = s.get_profile()
    return {k: (v[0], v[2]) for k, v in prof.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_volume_ledger(name, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    got = _ledger(name)
    print(name, got)
    assert got == LEDGERS[name]


if __name__ == "__main__":
    for k in SWITCHES:
        os.environ.pop(k, None)
    print("LEDGERS = {")
    for name in CASES:
        print(f'    "{name}": {{')
        for k, v in _ledger(name).items():
            print(f'        "{k}": {v!r},')
        print("    },")
    print("}")
