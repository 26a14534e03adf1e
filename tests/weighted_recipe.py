"""Weighted windows (sgm_set_weighted), in numpy: the reference's
cost functions with WEIGHTED_COST on, restated literally.

  weights(e_h, e_w)      Solver::Solver's Gaussian table (Solver.cpp:29-45)
  refusal(window, s)     the rule of sgm_set_weighted / sgm_set_window on a weighted handle
  census(img, e_h, e_w)  CT_pts (cost.cpp:99-129): taps of weight < 0.5 skipped
  window_volume(...)     Solver::build_dsi over SAD / SSD (cost.cpp:4-59): the taps in the
                         reference's order (rows outer, columns inner), cost = cost + AD * w in
                         fp32 (numpy multiplies, rounds, then adds: no FMA), two fp32 divisions
  recipe(...)            whole frames, composed from the oracle's stages as
                         tests/window_recipe.py composes them

and the case lists of the tests and of tests/golden/make_ref_weighted_golden.py,
which writes the fixtures under tests/golden/weighted/ with the reference's own
compiled functions; tests/test_weighted_cpu.py pins everything here to them.
The images and shapes are tests/window_cases.py's.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np

import oracle
import volume_filter_recipe
import volume_recipe
import window_cases as cases
import window_recipe as wr
from min_disp_recipe import shift_tables
from paths4_recipe import aggregate, assert_bits_equal, cost_volume  # noqa: F401
from window_cases import effective, wid, working  # noqa: F401

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted")

# ------------------------------------------------------------------- cases
# windows as sgm_set_window takes them, by scale; every effective side odd
CENSUS_SHAPES = [(3, 5), (16, 64), (17, 65), (33, 130)]
CENSUS_WINDOWS = {1: [(7, 9), (9, 7), (7, 7), (5, 9), (5, 5), (1, 9)], 2: [(14, 18), (10, 18)]}
# bits the disc keeps, by effective window (5 x 9 has 44 bits and loses its four corners)
KEPT_BITS = {(7, 9): 50, (9, 7): 50, (7, 7): 44, (5, 9): 40, (9, 5): 40, (5, 5): 24, (3, 3): 8, (1, 9): 8}
COST_WINDOWS = {1: CENSUS_WINDOWS[1] + [(3, 3)], 2: CENSUS_WINDOWS[2]}
COST_SHAPES = ("3x5", "10x20", "24x33", "20x70")
# The fixtures pin the recipe, which the GPU tests then compare with over every case: every
# window on the three smaller shapes, the widest windows on the largest.
COST_FIXTURES = (
    [(name, 1, win) for name in ("3x5", "10x20", "24x33") for win in COST_WINDOWS[1]]
    + [("20x70", 1, (7, 9))]
    + [("24x33", 2, (14, 18)), ("24x33", 2, (10, 18)), ("20x70", 2, (14, 18))]
)
# (accepted?, window, scale): the refusal rule
RULE = [
    (True, (7, 9), 1), (True, (9, 7), 1), (True, (3, 3), 1), (True, (1, 9), 1), (True, (9, 1), 1),
    (True, (14, 18), 2), (True, (15, 19), 2), (True, (10, 18), 2), (True, (2, 6), 2),
    (False, (7, 9), 2),    # 3 x 4: the default at scale 2
    (False, (5, 6), 1),    # an even width
    (False, (10, 12), 2),  # 5 x 6
    (False, (6, 5), 1), (False, (8, 8), 1), (False, (12, 10), 2),
    (False, (9, 9), 1),    # 80 census bits, weighted or not
    (False, (1, 1), 1), (False, (11, 3), 1), (False, (0, 3), 1), (False, (18, 18), 2),
]


def census_fixture(shape, s):
    return os.path.join(GOLDEN_DIR, f"ref_weighted_ct_{shape[0]}x{shape[1]}_s{s}.npz")


def cost_fixture(name, s, window):
    return os.path.join(GOLDEN_DIR, f"ref_weighted_ad_{name}_s{s}_{wid(window)}.npz")


WEIGHTS_FIXTURE = os.path.join(GOLDEN_DIR, "ref_weighted_weights.npz")


def weight_windows():
    """Every effective window a fixture or a test uses."""
    out = []
    for s, wins in COST_WINDOWS.items():
        for w in wins:
            if effective(w, s) not in out:
                out.append(effective(w, s))
    return out


@functools.lru_cache(maxsize=None)
def ref_census(shape, s, window):
    with np.load(census_fixture(shape, s)) as z:
        out = z["l_" + wid(window)], z["r_" + wid(window)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_cost(name, s, window, kind):
    with np.load(cost_fixture(name, s, window)) as z:
        v = z[kind]
    v.setflags(write=False)
    return v


# ------------------------------------------------------------------ recipe
def refusal(window, s):
    """Why sgm_set_weighted (or sgm_set_window on a weighted handle) refuses, or None:
    window_refusal's rules, then both effective sides odd."""
    if s not in (1, 2):
        return "scale"
    e_h, e_w = effective(window, s)
    if not (1 <= e_h <= 9 and 1 <= e_w <= 9):
        return "1..9"
    if e_h // 2 == 0 and e_w // 2 == 0:
        return "centre"
    if (2 * (e_h // 2) + 1) * (2 * (e_w // 2) + 1) - 1 > 64:
        return "64 bits"
    if e_h % 2 == 0 or e_w % 2 == 0:
        return "odd"
    return None


@functools.lru_cache(maxsize=None)
def weights(e_h, e_w):
    """weight[i * win_w + j] = exp((pow(i - win_h / 2, 2) + pow(j - win_w / 2, 2)) / -25.0),
    a double stored into a float."""
    w = np.empty((e_h, e_w), np.float32)
    for i in range(e_h):
        for j in range(e_w):
            w[i, j] = np.float32(math.exp((float((i - e_h // 2) ** 2) + float((j - e_w // 2) ** 2)) / -25.0))
    w.setflags(write=False)
    return w


def kept(e_h, e_w, weighted=True):
    """The taps CT_pts keeps, (e_h, e_w) bool: not the centre, and weight >= 0.5 when weighted."""
    k = np.ones((e_h, e_w), bool)
    if weighted:
        k = ~(weights(e_h, e_w) < 0.5)
    k = k.copy()
    k[e_h // 2, e_w // 2] = False
    return k


def census(img, e_h, e_w, weighted=True):
    """CT_pts over a working-grid image with WEIGHTED_COST as given: the loops of cost.cpp:107-122;
    a skipped tap shifts nothing."""
    assert e_h % 2 == 1 and e_w % 2 == 1
    H, W = img.shape
    hh, hw = e_h // 2, e_w // 2
    keep = kept(e_h, e_w, weighted)
    out = np.zeros((H, W), np.uint64)
    rows, cols = np.arange(H), np.arange(W)
    for i in range(-hh, hh + 1):
        y = np.minimum(np.maximum(rows + i, 0), H - 1)
        for j in range(-hw, hw + 1):
            if not keep[i + hh, j + hw]:
                continue
            x = np.minimum(np.maximum(cols + j, 0), W - 1)
            out = (out << np.uint64(1)) | (img[y][:, x] > img).astype(np.uint64)
    return out


def frame_census(img, window, s, blur=True, bm_rows=False, weighted=True):
    """The table a frame of a weighted handle builds of a full-size image (window_recipe's, masked)."""
    if bm_rows:
        h, w = img.shape
        g = np.ascontiguousarray(img[:h // s, :(w // s) * s:s])
    else:
        g = working(img, s)
    return census(oracle.blur(g) if blur else g, *effective(window, s), weighted=weighted)


def window_volume(L, R, D, kind, e_h, e_w, s=1, min_disp=0, weighted=True):
    """Solver::build_dsi over SAD or SSD on working-grid images, tap by tap in the reference's
    order for every (row, column, d) at once: cost starts at 0.0f, each tap adds
    (float)AD * weight (weighted) or AD (not), each a float32 operation of its own; then
    cost / e_h / e_w."""
    assert e_h % 2 == 1 and e_w % 2 == 1
    rows, cols = L.shape
    hh, hw = e_h // 2, e_w // 2
    w = weights(e_h, e_w)
    Li, Ri = L.astype(np.int32), R.astype(np.int32)
    shift = (np.arange(D)[None, :] + min_disp) // s           # disp / scale
    yy, xx = np.arange(rows), np.arange(cols)
    cost = np.zeros((rows, cols, D), np.float32)
    for i in range(-hh, hh + 1):
        y = np.minimum(np.maximum(yy + i, 0), rows - 1)
        for j in range(-hw, hw + 1):
            x_l = np.minimum(np.maximum(xx + j, 0), cols - 1)  # (cols,)
            x_r = np.maximum(x_l[:, None] - shift, 0)          # (cols, D)
            diff = Li[y][:, x_l][:, :, None] - Ri[y][:, x_r]   # (rows, cols, D)
            ad = (np.abs(diff) if kind == "sad" else diff * diff).astype(np.float32)
            if weighted:
                ad = ad * w[i + hh, j + hw]                    # float32 * float32, rounded
            cost = cost + ad                                   # float32 + float32, rounded
    assert cost.dtype == np.float32
    return ((cost / np.float32(e_h)) / np.float32(e_w)).astype(np.float32)


def volume(left, right, D, kind, window, s=1, min_disp=0, weighted=True):
    """The left cost volume of two full-size grey images, as a weighted frame or window_cost builds it."""
    return window_volume(working(left, s), working(right, s), D, kind, *effective(window, s), s, min_disp,
                         weighted)


def recipe(left, right, D, window=(7, 9), s=1, paths=8, m=0, blur=True, views=2, cost="census", solver="sgm",
           filters=(False, False)):
    """The maps of a frame on a weighted handle, oracle.process's keys (window_recipe.recipe with
    the masked tables or the weighted volume in the place of its own)."""
    if cost != "census":
        C = volume(left, right, D, cost, window, s, m)
        if any(filters):
            return volume_filter_recipe.recipe(C, m, s, paths, (1 if filters[0] else 0) | (2 if filters[1] else 0))
        return volume_recipe.recipe(C, m, s, paths)
    if solver == "bm":
        ctl, ctr = (frame_census(x, window, s, blur, bm_rows=True) for x in (left, right))
        d = wr.bm_wta(cost_volume(ctl, ctr, D, s, 0, None))
        return {"disp": d, "final": oracle.post_filter(d.astype(np.float32), D, s)}
    ctl, ctr = frame_census(left, window, s, blur), frame_census(right, window, s, blur)
    ctl_s, ctr_s = shift_tables(ctl, ctr, m // s)
    out = {}
    vols = [cost_volume(ctl, ctr_s, D, s, 0, None)]
    if views == 2:
        vols.append(cost_volume(ctl_s, ctr, D, s, 1, None))
    for C, sfx in zip(vols, ("", "_beta")):
        S = aggregate(C, paths)
        d = oracle.wta(S)
        out["disp" + sfx] = d + m
        out["sub" + sfx] = (oracle.subpixel(d, S) + np.float32(m)).astype(np.float32)
    if views == 2:
        out["lr"] = oracle.lr_check(out["sub"], out["sub_beta"], D + m, s)
        out["final"] = oracle.post_filter(out["lr"], D + m, s)
    else:
        out["final"] = oracle.post_filter(out["sub"], D + m, s)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
