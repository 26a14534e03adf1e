"""The cost stage's launch variants that no small frame reaches: which kernel
launch_cost_h picks depends on whether a padded census row, W + 2 * (D / scale
+ 16) words, fits 64 KiB of LDS at 16 bytes per word (17 with a sky mask):

  * both rows staged (one row per block at these widths);
  * D >= 64 past that: the uniform-operand kernel (8 or 9 bytes per word);
  * D < 64 past that: cost_h_global_kernel, one view slot per launch, so a
    two-view frame's joint cost_h and vfwd launches are refused.

Each side of each switch, both views, with and without a mask, the raw DSI
(filters = 0) and the horizontal filter (filters = 1), bit-exact against the
oracle through the stage API; then whole frames at the fallback width.  Rows
are few (H = 5 or 6): the switches depend on the width alone.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from support import f32_bits as bits
from stereo_matching_amd import SGM

pytestmark = pytest.mark.gpu

# D, scale, working-grid rows and columns, sky mask, the launch it reaches
CASES = [
    (64, 1, 5, 3936, False, "stride 4096: staged"),
    (64, 1, 5, 3937, False, "stride 4097: uniform operand"),
    (64, 1, 6, 3695, True, "stride 3855, masked: staged"),
    (64, 1, 6, 3696, True, "stride 3856, masked: uniform operand"),
    (32, 1, 6, 4000, False, "stride 4096: staged"),
    (32, 1, 6, 4001, False, "stride 4097: global"),
    (32, 1, 5, 4001, True, "masked: global"),
    (32, 2, 5, 4033, False, "scale 2, stride 4097: global, window 2"),
    (32, 2, 5, 4033, True, "scale 2, masked: global, window 2"),
]
IDS = [f"D{D}-s{s}-{H}x{W}{'-sky' if sky else ''}" for D, s, H, W, sky, _ in CASES]


@pytest.mark.parametrize("D,s,H,W,sky,what", CASES, ids=IDS)
def test_cost_h_variants(D, s, H, W, sky, what):
    rng = np.random.default_rng(D + W)
    nbits = 62 if s == 1 else 14  # the census words of the 7x9 and the 3x5 window
    ctl, ctr = rng.integers(0, 1 << nbits, (2, H, W), dtype=np.uint64)
    # 255 marks sky; every other value is ground
    mask = np.where(rng.random((H, W)) < 0.3, 255, rng.integers(0, 255, (H, W))).astype(np.uint8) if sky else None
    with SGM(H * s, W * s, s, D) as sgm:
        for view in (0, 1):
            raw = oracle.dsi(ctl, ctr, D, s, view, mask)
            got = sgm.stage_cost(ctl, ctr, view, mask, filters=0)
            assert np.array_equal(bits(got), bits(raw)), f"dsi v{view}: {what}"
            got = sgm.stage_cost(ctl, ctr, view, mask, filters=1)
            assert np.array_equal(bits(got), bits(oracle.hfilter(raw, 5 // s))), f"hfilter v{view}: {what}"


# Whole frames where rows are too wide for the staged kernel: the views' cost_h
# and vfwd launches run one by one (slot 1, then slot 0).
FRAME = dict(h=6, w=4001, D=32)


@pytest.fixture(scope="module")
def frame():
    h, w, D = FRAME["h"], FRAME["w"], FRAME["D"]
    left, right = np.random.default_rng(7).integers(0, 256, (2, h, w), dtype=np.uint8)
    return left, right, oracle.process(left, right, D)


def test_fallback_frame_two_views(frame):
    left, right, ref = frame
    h, w, D = FRAME["h"], FRAME["w"], FRAME["D"]
    with SGM(h, w, 1, D) as sgm:
        sgm.set_profiling(True)
        sgm.process(left, right)
        prof = sgm.get_profile()
        assert np.array_equal(sgm.get_raw_disp().astype(np.int64), ref["disp"].astype(np.int64))
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(ref["lr"]))
    one_view = float(h * w * D)
    assert (prof["cost_h"][0], prof["cost_h"][2]) == (2, one_view)
    assert (prof["vfwd"][0], prof["vfwd"][2]) == (2, one_view)


def test_fallback_frame_right_view_handle(frame):
    left, right, ref = frame
    h, w, D = FRAME["h"], FRAME["w"], FRAME["D"]
    with SGM(h, w, 1, D, views=1, view="right") as sgm:
        sgm.process(left, right)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(ref["sub_beta"]))
        assert np.array_equal(sgm.get_raw_disp().astype(np.int64), ref["disp_beta"].astype(np.int64))
