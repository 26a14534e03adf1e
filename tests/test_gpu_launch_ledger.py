"""The launch ledger of every frame schedule.

With profiling on, one frame leaves {class: (launches, elements per launch)} in
get_profile(): which launches a schedule makes, how often, and how much each
covers.  The elements are computed on the host, so the ledgers are compared
exactly.  One case per branch of the schedule (sgm_frame.hip: cost_stage,
run_frame, the aggregations, bm_frame, finish_frame), each at the smallest
shape that reaches it.  The bit-exact tests pin what the launches compute;
this one pins which launches run.

The table was recorded from the library as it was before the schedules moved
out of the C-ABI file, sgm_capi.hip (`python tests/test_gpu_launch_ledger.py` prints it);
slant_v1_cost_h and per_view_v2 from the library as it was before the one- and
two-view launchers became one per role.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import rectify_recipe
from stereo_matching_amd import BM, SGM, synthetic

pytestmark = pytest.mark.gpu

SWITCHES = ("SGM_BAND_ROWS", "SGM_SLANT", "SGM_VSTRIP", "SGM_P4_HPAIR", "SGM_CONFIDENCE")


def _maps_37x53(s):
    s.set_rectify(37, 53, *rectify_recipe.maps(s.h, s.w, 37, 53, 0), *rectify_recipe.maps(s.h, s.w, 37, 53, 1))


def _size_and_bgr8(s):
    s.set_input_size(37, 53)
    s.set_input_format("bgr8")


# name: (h, w, D, constructor keywords, (left mask, right mask), environment[, setter applied after
# construction: the frame then takes random images of the shape the handle asks for])
CASES = {
    "joint": (96, 260, 128, {}, (False, False), {}),
    "bands": (96, 260, 128, {}, (False, False), {"SGM_BAND_ROWS": "32"}),
    "one_view": (96, 260, 128, {"views": 1}, (False, False), {}),
    "one_view_bands": (96, 260, 128, {"views": 1}, (False, False), {"SGM_BAND_ROWS": "32"}),
    "slant_strips": (80, 240, 256, {}, (True, True), {"SGM_SLANT": "1"}),
    "slant_cost_h": (80, 240, 256, {}, (True, True), {"SGM_SLANT": "1", "SGM_VSTRIP": "0"}),
    # one view: the same vfwd_l3 launch with one view
    "slant_v1_cost_h": (80, 240, 256, {"views": 1}, (False, False), {"SGM_SLANT": "1", "SGM_VSTRIP": "0"}),
    "left_mask": (100, 300, 64, {}, (True, False), {}),
    "paths4_v1_one_launch": (96, 260, 128, {"paths": 4, "views": 1}, (False, False), {"SGM_P4_HPAIR": "0"}),
    "paths4_v1_split": (96, 260, 128, {"paths": 4, "views": 1}, (False, False), {"SGM_P4_HPAIR": "1"}),
    "paths4_v2_one_launch": (96, 260, 128, {"paths": 4}, (False, False), {"SGM_P4_HPAIR": "0"}),
    "paths4_v2_split": (96, 260, 128, {"paths": 4}, (False, False), {"SGM_P4_HPAIR": "1"}),
    "bm": (96, 260, 64, {"bm": True}, (False, False), {}),
    "post_lk": (96, 260, 128, {"post_filter": True, "lk_refine": True}, (False, False), {}),
    # 277 MB per volume: the smallest shape above the Infinity Cache, where
    # SGM_BAND_ROWS=0 runs whole-volume passes and both views' finals at once
    "whole_final2": (512, 1056, 128, {}, (False, False), {"SGM_BAND_ROWS": "0"}),
    # 135.2 MB per volume: the smallest shape whose volumes fit the Infinity Cache one at a time
    # but not together, where two views run whole-volume passes view after view
    "per_view_v2": (264, 500, 256, {}, (False, False), {}),
    # the input slot (sgm_frame.hip input_slot): one launch in front of the one_view frame, whichever
    # stages are set
    "input_size": (96, 260, 128, {"views": 1}, (False, False), {}, lambda s: s.set_input_size(37, 53)),
    "input_maps": (96, 260, 128, {"views": 1}, (False, False), {}, _maps_37x53),
    "input_bgr8": (96, 260, 128, {"views": 1}, (False, False), {}, lambda s: s.set_input_format("bgr8")),
    "input_size_bgr8": (96, 260, 128, {"views": 1}, (False, False), {}, _size_and_bgr8),
}

# the adaptive median fill's launch count depends on the map
DATA_DEPENDENT = ("post_median",)

LEDGERS = {
    "joint": {
        "census": (1, 49920.0),
        "cost_h": (1, 6389760.0),
        "vfwd": (1, 6389760.0),
        "stage_a": (1, 6389760.0),
        "stage_b": (1, 6389760.0),
        "sweep_L8_acc": (1, 6389760.0),
        "pair_bwd_L4_final": (1, 6389760.0),
        "lr": (1, 24960.0),
    },
    "bands": {
        "census": (1, 49920.0),
        "cost_h": (1, 6389760.0),
        "vfwd": (6, 1064960.0),
        "stage_a_d": (6, 1064960.0),
        "stage_a_h": (1, 6389760.0),
        "stage_b_d2": (6, 1064960.0),
        "sweep_L8_acc": (6, 1064960.0),
        "pair_bwd_L4_final": (6, 1064960.0),
        "lr": (1, 24960.0),
    },
    "one_view": {
        "census": (1, 49920.0),
        "cost_h": (1, 3194880.0),
        "vfwd": (1, 3194880.0),
        "stage_a": (1, 3194880.0),
        "stage_b": (1, 3194880.0),
        "sweep_L8_acc": (1, 3194880.0),
        "pair_bwd_L4_final": (1, 3194880.0),
    },
    "one_view_bands": {
        "census": (1, 49920.0),
        "cost_h": (1, 3194880.0),
        "vfwd": (3, 1064960.0),
        "stage_a_d": (3, 1064960.0),
        "stage_a_h": (1, 3194880.0),
        "stage_b_d2": (3, 1064960.0),
        "sweep_L8_acc": (3, 1064960.0),
        "pair_bwd_L4_final": (3, 1064960.0),
    },
    "slant_strips": {
        "census": (1, 38400.0),
        "cost_ck": (1, 9830400.0),
        "sky_words": (2, 19200.0),
        "vstrip": (1, 9830400.0),
        "slant_down": (1, 9830400.0),
        "stage_a_h": (1, 9830400.0),
        "slant_down_hpair": (1, 9830400.0),
        "slant_up": (1, 9830400.0),
        "lr": (1, 19200.0),
    },
    "slant_cost_h": {
        "census": (1, 38400.0),
        "cost_h": (1, 9830400.0),
        "vfwd_l3": (1, 9830400.0),
        "slant_down": (1, 9830400.0),
        "stage_a_h": (1, 9830400.0),
        "slant_down_hpair": (1, 9830400.0),
        "slant_up": (1, 9830400.0),
        "lr": (1, 19200.0),
    },
    "slant_v1_cost_h": {
        "census": (1, 38400.0),
        "cost_h": (1, 4915200.0),
        "vfwd_l3": (1, 4915200.0),
        "slant_down": (1, 4915200.0),
        "stage_a_h": (1, 4915200.0),
        "slant_down_hpair": (1, 4915200.0),
        "slant_up": (1, 4915200.0),
    },
    "left_mask": {
        "census": (1, 60000.0),
        "cost_h": (2, 1920000.0),
        "vfwd": (2, 1920000.0),
        "stage_a": (1, 3840000.0),
        "stage_b": (1, 3840000.0),
        "sweep_L8_acc": (1, 3840000.0),
        "pair_bwd_L4_final": (1, 3840000.0),
        "lr": (1, 30000.0),
    },
    "paths4_v1_one_launch": {
        "census": (1, 49920.0),
        "cost_h": (1, 3194880.0),
        "vfwd": (1, 3194880.0),
        "hpair4": (1, 3194880.0),
        "final4": (1, 3194880.0),
    },
    "paths4_v1_split": {
        "census": (1, 49920.0),
        "cost_h": (1, 3194880.0),
        "vfwd": (1, 3194880.0),
        "hpair4_fwd": (1, 3194880.0),
        "hpair4_bwd": (1, 3194880.0),
        "final4": (1, 3194880.0),
    },
    "paths4_v2_one_launch": {
        "census": (1, 49920.0),
        "cost_h": (1, 6389760.0),
        "vfwd": (1, 6389760.0),
        "hpair4": (1, 6389760.0),
        "final4": (1, 6389760.0),
        "lr": (1, 24960.0),
    },
    "paths4_v2_split": {
        "census": (1, 49920.0),
        "cost_h": (1, 6389760.0),
        "vfwd": (1, 6389760.0),
        "hpair4_fwd": (1, 6389760.0),
        "hpair4_bwd": (1, 6389760.0),
        "final4": (1, 6389760.0),
        "lr": (1, 24960.0),
    },
    "bm": {
        "census": (1, 49920.0),
        "cost_h": (1, 1597440.0),
        "vfwd": (1, 1597440.0),
        "bm_wta": (1, 1597440.0),
        "post_prep": (1, 24960.0),
        "post_cc_local": (2, 24960.0),
        "post_cc_merge": (2, 24960.0),
        "post_cc_count": (2, 24960.0),
        "post_cc_apply": (2, 24960.0),
    },
    "post_lk": {
        "census": (1, 49920.0),
        "cost_h": (1, 6389760.0),
        "vfwd": (1, 6389760.0),
        "stage_a": (1, 6389760.0),
        "stage_b": (1, 6389760.0),
        "sweep_L8_acc": (1, 6389760.0),
        "pair_bwd_L4_final": (1, 6389760.0),
        "lr": (1, 24960.0),
        "post_prep": (1, 24960.0),
        "post_cc_local": (2, 24960.0),
        "post_cc_merge": (2, 24960.0),
        "post_cc_count": (2, 24960.0),
        "post_cc_apply": (2, 24960.0),
        "lk_refine": (1, 24960.0),
    },
    "whole_final2": {
        "census": (1, 1081344.0),
        "cost_h": (1, 138412032.0),
        "vfwd": (1, 138412032.0),
        "stage_a": (2, 69206016.0),
        "stage_b": (2, 69206016.0),
        "sweep_L8_acc": (2, 69206016.0),
        "pair_bwd_L4_final": (1, 138412032.0),
        "lr": (1, 540672.0),
    },
    "per_view_v2": {
        "census": (1, 264000.0),
        "cost_h": (1, 67584000.0),
        "vfwd": (1, 67584000.0),
        "stage_a": (2, 33792000.0),
        "stage_b": (2, 33792000.0),
        "sweep_L8_acc": (2, 33792000.0),
        "pair_bwd_L4_final": (2, 33792000.0),
        "lr": (1, 132000.0),
    },
}
# the one_view ledger plus exactly one entry, 2 x 96 x 260 elements: both images in one launch
for _name, _cls in (("input_size", "resize"), ("input_maps", "rectify"), ("input_bgr8", "gray"),
                    ("input_size_bgr8", "resize")):
    LEDGERS[_name] = dict(LEDGERS["one_view"], **{_cls: (1, 49920.0)})


def _ledger(name):
    """One frame of case `name` under the environment as it is now."""
    h, w, D, kw, (sky_l, sky_r), _, *setter = CASES[name]
    kw = dict(kw)
    left, right = synthetic.stereo_pair(h, w, D, pair_index=5, kind="road")
    mask = synthetic.sky_mask(h, w)
    with (BM(h, w, 1, D) if kw.pop("bm", False) else SGM(h, w, 1, D, **kw)) as s:
        if setter:
            setter[0](s)
            shape = (s.in_h, s.in_w) if s.in_ch == 1 else (s.in_h, s.in_w, s.in_ch)
            left, right = np.random.default_rng(5).integers(0, 256, (2,) + shape, dtype=np.uint8)
        s.set_profiling(True)
        s.process(left, right, mask if sky_l else None, mask if sky_r else None)
        prof = s.get_profile()
    return {k: (v[0], v[2]) for k, v in prof.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_ledger(name, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[name][5].items():
        monkeypatch.setenv(k, v)
    got = _ledger(name)
    print(name, got)
    if "post_median" in got:
        # 3 fill launches, then 2 more for every further round of the
        # component kernels (post_filter's pf_iters)
        assert got["post_median"][0] == 3 + 2 * (got["post_cc_local"][0] - 1)
    assert {k: v for k, v in got.items() if k not in DATA_DEPENDENT} == LEDGERS[name]


if __name__ == "__main__":
    for k in SWITCHES:
        os.environ.pop(k, None)
    print("LEDGERS = {")
    for name, case in CASES.items():
        os.environ.update(case[5])
        led = _ledger(name)
        for k in case[5]:
            del os.environ[k]
        print(f'    "{name}": {{')
        for k, v in led.items():
            if k not in DATA_DEPENDENT:
                print(f'        "{k}": {v!r},')
        print("    },")
    print("}")
