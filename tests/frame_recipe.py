"""One composed CPU reference for a frame under any settings a handle takes:
frame(left, right, settings, sky_l, sky_r) -> every map the handle can report,
and refusal(settings) -> why the library refuses them, or None.

No arithmetic of its own: frame() routes the settings record to the recipes that
already pin each feature (tests/window_recipe.py for census, SAD / SSD and BM
frames with a window, weights, a minimum disparity and 4 or 8 paths;
tests/ct_cost_recipe.py for the CT volume; tests/volume_recipe.py and
tests/volume_filter_recipe.py from a volume on; tests/fill_recipe.py;
tests/reproject_recipe.py) and hands every one of them the handle's P1, P2,
uniqueness ratio and LR threshold and each view its own sky mask.
tests/test_frame_recipe_cpu.py ties it to oracle.process, to each recipe on its
own and to tests/pyref.py's independent loops.

What frame() does decide is the order of a frame's last stages, a restatement of
sgm_frame.hip's finish_frame and run_frame that only the GPU comparison checks:
the LR check (two views), post_filter where params.post_filter is set, the
hole filling where fill is set, then the reprojection of that last map.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import ct_cost_recipe
import fill_recipe
import oracle
import reproject_recipe
import volume_filter_recipe
import volume_recipe
import weighted_recipe
import window_recipe

COSTS = ("census", "sad", "ssd", "ct")
FILLS = ("off", "background", "interpolate")
VIEWS = ("two", "left", "right")


@dataclasses.dataclass(frozen=True)
class Settings:
    """What a handle is created with and set to.  views: "two", or one view "left" / "right";
    window: (win_h, win_w) as sgm_set_window takes it, None: the reference's (7, 9);
    volume_filter: (horizontal, vertical); reproject: Q (16 values) or None; sky_detect: the
    handle makes its own masks (params.sky_detect)."""
    solver: str = "sgm"
    D: int = 64
    s: int = 1
    blur: bool = True
    views: str = "two"
    paths: int = 8
    min_disp: int = 0
    cost: str = "census"
    window: tuple | None = None
    weighted: bool = False
    volume_filter: tuple = (False, False)
    p1: int = 10
    p2: int = 100
    uniqueness: float = 0.7
    lr_max_diff: float = 1.0
    post_filter: bool = False
    confidence: bool = False
    fill: str = "off"
    reproject: tuple | None = None
    sky_detect: bool = False

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


def refusal(st, sky=False):
    """Why sgm_create or a setter refuses these settings (the rule's name), or None.  sky: the
    frame is handed sky masks.  Each rule is the library's own check:
    sgm_plan.h valid_params (create), sgm_create.hip's setters, sgm_fill.hip sgm_set_fill,
    sgm_capi.hip's frame check (masks with a window cost); DESIGN.md 5h, 5o-5t."""
    if st.solver not in ("sgm", "bm") or st.cost not in COSTS or st.fill not in FILLS or st.views not in VIEWS:
        return "unknown value"
    if st.s not in (1, 2) or st.D not in (32, 64, 128, 256) or st.paths not in (4, 8):
        return "create: scale, max_disp or paths"
    if st.p1 < 0 or st.p2 < 0:
        return "create: negative penalty"
    if not st.uniqueness > 0.0:  # (valid_params' bound 8 (p2 + 999999) / FLT_MAX is ~1e-31)
        return "create: uniqueness"
    if st.views == "right" and (st.solver != "sgm" or st.post_filter):
        return "create: a right-view handle is a one-view SGM handle without post_filter"
    # sgm_set_window: window_refusal; a weighted handle: weighted_refusal (odd effective sides)
    if st.window is not None or st.weighted:
        why = weighted_recipe.refusal(st.window or window_recipe.DEFAULT, st.s)
        if why == "odd":
            if st.weighted:
                return "weighted: odd effective window sides"
        elif why:
            return "window: " + why
    if st.min_disp < 0 or st.min_disp % st.s or st.D + st.min_disp + 1 > 65535:
        return "min_disp: >= 0, a multiple of the scale, D + m + 1 in 16 bits"
    if st.solver == "bm":
        if st.min_disp:
            return "bm: no min_disp"
        if st.cost != "census":
            return "bm: no cost kind"
        if st.fill == "interpolate":
            return "bm: no interpolate"
        if st.confidence:
            return "bm: no confidence"
        if any(st.volume_filter):
            return "bm: no volume filter"
        if st.views != "left":
            return "bm: one view, the left"
    if st.fill == "interpolate" and st.views != "two":
        return "interpolate: two views"
    if st.views == "right" and (st.cost != "census" or any(st.volume_filter) or st.fill != "off"
                                or st.reproject is not None):
        return "right view: no cost kind, volume filter, fill or reprojection"
    if st.cost != "census" and st.sky_detect:
        return "sky_detect: no cost kind"
    if st.cost != "census" and sky:
        return "sky masks: no cost kind"
    return None


def _views(left, right, st, sky_l, sky_r):
    """The views' maps by the recipe the settings belong to (keys as oracle.process, "ratio"s too)."""
    kw = dict(P1=st.p1, P2=st.p2, uniq=st.uniqueness, lr_dis=st.lr_max_diff)
    window = st.window or window_recipe.DEFAULT
    if st.cost == "ct":
        C = ct_cost_recipe.volume(left, right, st.D, st.s, st.min_disp, window, st.weighted)
        fbits = (1 if st.volume_filter[0] else 0) | (2 if st.volume_filter[1] else 0)
        if fbits:
            return volume_filter_recipe.recipe(C, st.min_disp, st.s, st.paths, fbits, **kw)
        return volume_recipe.recipe(C, st.min_disp, st.s, st.paths, **kw)
    # (census frames filter as ever: sgm_set_volume_filter is for volume frames)
    return window_recipe.recipe(left, right, st.D, window, st.s, None, st.paths, st.min_disp, st.blur,
                                1 if st.views == "left" and st.cost == "census" else 2, st.cost, st.solver,
                                st.weighted, st.volume_filter if st.cost != "census" else (False, False),
                                sky_l=sky_l, sky_r=sky_r, ratio=True, **kw)


def frame(left, right, settings, sky_l=None, sky_r=None):
    """The maps a handle with `settings` reports after process(left, right, sky_l, sky_r), in true
    disparity: "disp" (raw WTA), "sub", "ratio" -- of the handle's one view, or of the left view
    with "sub_beta", "ratio_beta" and "lr" beside them on a two-view handle --, "map" (what
    process() returns: the LR or sub-pixel map, post-filtered where post_filter is set),
    "final" (post_filter of the LR / sub-pixel map: get_disp() of an unfilled handle; not on a
    right-view handle), "filled" and "fill_mask" (fill set: "map" filled), "xyz" and "depth"
    (reproject set: of the frame's last map)."""
    st = settings
    why = refusal(st, sky_l is not None or sky_r is not None)
    assert why is None, why
    if st.sky_detect:
        sky_l, sky_r = oracle.sky_detect(left, st.s), oracle.sky_detect(right, st.s)
    Dm = st.D + st.min_disp
    v = _views(left, right, st, sky_l, sky_r)
    out = {}
    if st.solver == "bm":
        out["disp"] = v["disp"]
        base = None
        out["final"] = out["map"] = v["final"]     # (BM::process always ends in post_filter)
    elif st.views == "right":
        out["disp"], out["sub"], out["ratio"] = v["disp_beta"], v["sub_beta"], v["ratio_beta"]
        base = out["sub"]
    elif st.views == "left":
        out["disp"], out["sub"], out["ratio"] = v["disp"], v["sub"], v["ratio"]
        base = out["sub"]
    else:
        for k in ("disp", "sub", "ratio", "sub_beta", "ratio_beta", "lr"):
            out[k] = v[k]
        base = out["lr"]
    if not st.confidence:
        out = {k: a for k, a in out.items() if not k.startswith("ratio")}
    if base is not None:
        if st.views != "right":
            out["final"] = oracle.post_filter(base, Dm, st.s)
        out["map"] = out["final"] if st.post_filter else base
    last = out["map"]
    if st.fill != "off":
        out["filled"], out["fill_mask"] = fill_recipe.fill(last, st.D, st.min_disp, st.s, out.get("sub_beta"),
                                                           st.fill, st.lr_max_diff)
        last = out["filled"]
    if st.reproject is not None:
        r = reproject_recipe.reproject(last, st.reproject, Dm + 1, st.s)
        out["xyz"], out["depth"] = r["xyz"], r["depth"]
    return out
