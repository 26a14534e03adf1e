"""The strip pass of the slanted schedule (sgm_vstrip.hip):
checkpoints of the horizontal IIR at every strip edge (launch_cost_ck; a strip
has sgm_vstrip_cols() = NC columns, 16 as built), then one pass that runs the horizontal IIR across each
strip from its checkpoint, the vertical IIR and the L3 forward pass, writing
C and the L3 volume.  It replaces cost_h + vfwd_l3 on slanted frames
(SGM_VSTRIP=0 restores those), so the maps must be bit-identical to the
oracle and to the two-pass path -- at the strip edges where the horizontal
filter's boundary columns meet the strips.  EDGE_CASES takes its widths from
the library's strip width, W = NC * k + r: a last strip of one column, W-1
(r = 1), starting at W-2 (r = 2; both raw columns only), at W-3 (r = 3: its
first column is the last filtered one, restored from a checkpoint with no update
after it), at W-4 (r = 4: one update) and one column short of full (r = NC-1),
and whole strips only (r = 0); unmasked frames take cost_ck_body, masked ones
cost_h_body<..., CK>.  CASES holds fixed widths: the 3-row and 5-column minimum
frame, widths around 24 and wider frames, each D, one and two views, sky masks
(staged as one word per pixel), and scale 2, where the strip pass does not
apply and the two-pass path runs.  The right-view handle runs both."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
from stereo_matching_amd import SGM, _capi, synthetic

pytestmark = pytest.mark.gpu

CASES = [
    # h, w, s, D, views, sky
    # (the comments: the last strip at 16 columns per strip)
    (3, 5, 1, 32, 2, False),      # the minimum frame, one partial strip
    (4, 23, 1, 64, 2, False),     # strip 1 starts at W-7
    (5, 24, 1, 64, 1, False),     # strip 1 starts at W-8
    (7, 25, 1, 128, 2, False),    # strip 1 starts at W-9
    (9, 26, 1, 128, 2, False),    # strip 1 starts at W-10
    (10, 27, 1, 256, 2, False),   # strip 1 starts at W-11
    (11, 28, 1, 256, 1, False),   # strip 1 starts at W-12
    (33, 300, 1, 32, 2, False),
    (20, 70, 1, 64, 2, True),     # sky masks
    (40, 97, 1, 64, 2, True),
    (64, 200, 1, 256, 2, True),
    (50, 241, 1, 128, 1, False),
    (40, 100, 2, 64, 2, True),    # scale 2: the two-pass path
]


# W = NC * k + r around the library's strip width NC, as (k, r); the width itself is worked out
# when the test runs (importing this file must not load the library).  Rows 3 .. 12, D over 64, 128,
# 256, one and two views; r = 3 and r = 4 also under a sky mask (rows >= 6: synthetic.sky_mask marks
# H / 6).
EDGE_CASES = [
    # h, (k, r), s, D, views, sky      the last strip
    (3, (1, 0), 1, 64, 2, False),      # r = 0: whole strips only
    (4, (1, 1), 1, 128, 1, False),     # r = 1: column W-1 (raw)
    (5, (1, 2), 1, 256, 2, False),     # r = 2: starts at W-2 (raw)
    (6, (1, 3), 1, 64, 2, False),      # r = 3: starts at W-3 (checkpoint, no update)
    (7, (1, 3), 1, 128, 1, True),
    (8, (1, 4), 1, 256, 2, False),     # r = 4: starts at W-4 (one update)
    (9, (1, 4), 1, 64, 2, True),
    (10, (2, -1), 1, 128, 2, False),   # W = 2 NC - 1 (k = 1, r = NC-1): one column short of two strips
    (11, (2, 3), 1, 256, 1, False),    # k = 2, r = 3
    (12, (2, 3), 1, 128, 2, True),
    (12, (2, 4), 1, 64, 1, False),     # k = 2, r = 4
]


def _id(c):
    w = c[1] if isinstance(c[1], int) else "%dNC%+d" % c[1]
    return f"{c[0]}x{w}_s{c[2]}_D{c[3]}_V{c[4]}{'_sky' if c[5] else ''}"


def _sized(c):
    """The case with its width as a number of columns."""
    if isinstance(c[1], int):
        return c
    nc = _capi.lib().sgm_vstrip_cols()
    assert nc >= 8
    return (c[0], nc * c[1][0] + c[1][1], *c[2:])


def _run(c, env, view="left"):
    h, w, s, D, views, use_sky = c
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        left, right = synthetic.stereo_pair(h, w, D, pair_index=7, kind="road")
        H, W = h // s, w // s
        sky = synthetic.sky_mask(H, W) if use_sky else None
        with SGM(h, w, s, D, views=views, view=view) as sgm:
            sgm.set_profiling(True)
            sgm.process(left, right, sky, sky)
            prof = sgm.get_profile()
            return sgm.get_lr_disp().copy(), sgm.get_raw_disp().copy(), prof, (left, right, sky)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("c", CASES + EDGE_CASES, ids=_id)
def test_strips_vs_oracle_and_two_pass(c):
    c = _sized(c)
    h, w, s, D, views, _ = c
    m, raw, prof, (left, right, sky) = _run(c, {"SGM_SLANT": "1"})
    strips = s == 1
    assert ("vstrip" in prof) == strips and ("vfwd_l3" in prof) == (not strips), sorted(prof)
    ref = oracle.process(left, right, D, scale=s, sky_l=sky, sky_r=sky, views=views)
    want = ref["lr"] if views == 2 else ref["sub"]
    assert np.array_equal(raw.astype(np.int64), ref["disp"].astype(np.int64)), "WTA"
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32)), "map"
    m2, raw2, prof2, _ = _run(c, {"SGM_SLANT": "1", "SGM_VSTRIP": "0"})
    assert "vstrip" not in prof2 and "vfwd_l3" in prof2, sorted(prof2)
    assert np.array_equal(m.view(np.uint32), m2.view(np.uint32))
    assert np.array_equal(raw, raw2)


@pytest.mark.parametrize("c", [(30, 130, 1, 128, 1, True), (12, 49, 1, 256, 1, False),
                               (9, (2, 3), 1, 64, 1, False)],
                         ids=["130_D128_sky", "49_D256", "2NC+3_D64"])
def test_right_view_handle(c):
    # a right-view handle runs the right-view DSI in slot 0 (dsi0 = 1)
    c = _sized(c)
    h, w, s, D, _, _ = c
    m, raw, prof, (left, right, sky) = _run(c, {"SGM_SLANT": "1"}, view="right")
    assert "vstrip" in prof, sorted(prof)
    ref = oracle.process(left, right, D, scale=s, sky_l=sky, sky_r=sky, views=2, final=False)
    assert np.array_equal(raw.astype(np.int64), ref["disp_beta"].astype(np.int64)), "WTA"
    assert np.array_equal(m.view(np.uint32), ref["sub_beta"].view(np.uint32)), "map"
    m2, raw2, _, _ = _run(c, {"SGM_SLANT": "1", "SGM_VSTRIP": "0"}, view="right")
    assert np.array_equal(m.view(np.uint32), m2.view(np.uint32))
    assert np.array_equal(raw, raw2)
