"""The matching window as a setting (sgm_set_window), in numpy:
CT_pts (cost.cpp:99-129) and SAD / SSD (cost.cpp:4-59) restated for a window
(e_h, e_w) = (win_h // s, win_w // s), and whole frames composed from the
oracle's stages on those tables, as tests/min_disp_recipe.py composes them.
tests/test_window_cpu.py pins the restatements to fixtures written by the
reference's own compiled functions, and to oracle.census and
tests/window_cost_recipe.py at the default (7, 9).

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

import oracle
import volume_filter_recipe
import volume_recipe
import weighted_recipe
import window_cost_recipe as wc
from min_disp_recipe import shift_tables
from confidence_recipe import ratio_of
from paths4_recipe import aggregate, assert_bits_equal, bits, cost_volume, masks  # noqa: F401
from window_cases import effective, working  # noqa: F401

DEFAULT = (7, 9)


def census(img, e_h, e_w, weighted=False):
    """CT_pts over a working-grid image (cost.cpp:107-122): rows -e_h/2 .. e_h/2, columns
    -e_w/2 .. e_w/2 in row-major order, the centre skipped, value = (value << 1) |
    (neighbour > centre) in a 64-bit word, coordinates clamped to the image.  weighted:
    WEIGHTED_COST on, the taps of weight < 0.5 skipped too; a skipped tap shifts nothing."""
    H, W = img.shape
    hh, hw = e_h // 2, e_w // 2
    assert (2 * hh + 1) * (2 * hw + 1) - 1 <= 64
    assert not weighted or (e_h % 2 == 1 and e_w % 2 == 1)
    keep = weighted_recipe.kept(2 * hh + 1, 2 * hw + 1, weighted)
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


def frame_census(img, window, s, blur=True, bm_rows=False, weighted=False):
    """The table a frame builds of a full-size image: decimated (BM: the columns only,
    BM.cpp:24-25), blurred, then CT_pts over the window at this scale (weighted: masked)."""
    if bm_rows:
        h, w = img.shape
        g = np.ascontiguousarray(img[:h // s, :(w // s) * s:s])
    else:
        g = working(img, s)
    return census(oracle.blur(g) if blur else g, *effective(window, s), weighted)


def window_volume(L, R, D, kind, e_h, e_w, s=1, min_disp=0):
    """Solver::build_dsi over SAD or SSD with the window (e_h, e_w) on working-grid images, by
    integer sums (tests/window_cost_recipe.py's separable form): the divisors are e_h and e_w."""
    rows, cols = L.shape
    hh, hw = e_h // 2, e_w // 2
    Li, Ri = L.astype(np.int64), R.astype(np.int64)
    x = np.arange(cols)[:, None]
    xr = np.maximum(x - (np.arange(D)[None, :] + min_disp) // s, 0)
    ad = np.abs(Li[:, :, None] - Ri[:, xr])
    if kind == "ssd":
        ad = ad * ad
    yi = np.clip(np.arange(rows)[:, None] + np.arange(-hh, hh + 1)[None, :], 0, rows - 1)
    col = ad[yi].sum(axis=1)
    xi = np.clip(np.arange(cols)[:, None] + np.arange(-hw, hw + 1)[None, :], 0, cols - 1)
    tot = col[:, xi].sum(axis=2)
    assert tot.max(initial=0) <= 63 * 255 * 255
    return ((tot.astype(np.float32) / np.float32(e_h)) / np.float32(e_w)).astype(np.float32)


def window_volume_literal(L, R, D, kind, e_h, e_w, s=1, min_disp=0):
    """The same volume by the reference's loops (window_cost_recipe.window_cost, line by line)."""
    rows, cols = L.shape
    cost = np.empty((rows, cols, D), np.float32)
    for i in range(rows):
        for j in range(cols):
            for d in range(D):
                cost[i, j, d] = wc.window_cost(L, R, j, i, d + min_disp, e_h, e_w, s, kind)
    return cost


def volume(left, right, D, kind, window, s=1, min_disp=0):
    """The left cost volume of two full-size grey images, as a frame or window_cost builds it."""
    return window_volume(working(left, s), working(right, s), D, kind, *effective(window, s), s, min_disp)


def bm_wta(cost, uniq=0.7):
    """BM's winner-take-all on the filtered cost (BM.cpp:53-85): the second minimum's index is
    declared once outside the pixel loops and so survives from pixel to pixel."""
    H, W, D = cost.shape
    invalid = D + 1
    disp = np.empty((H, W), np.int32)
    sec_d = invalid
    big = np.float32(np.finfo(np.float32).max)
    for i in range(H):
        for j in range(W):
            c = cost[i, j]
            min_d = int(np.argmin(c))  # the first of equal minima, as `<` keeps it
            min_c = c[min_d]
            if not min_c < big:
                min_d = invalid
                min_c = big
            rest = np.where(c != min_c, c, big)
            sec_c = big
            if (rest < big).any():
                sec_d = int(np.argmin(rest))
                sec_c = rest[sec_d]
            with np.errstate(all="ignore"):
                reject = np.float32(min_c) / np.float32(sec_c) > np.float32(uniq) and abs(min_d - sec_d) > 2
            disp[i, j] = invalid if reject else min_d
    return disp


def recipe(left, right, D, window=DEFAULT, s=1, sky=None, paths=8, m=0, blur=True, views=2, cost="census",
           solver="sgm", weighted=False, filters=(False, False), P1=10, P2=100, uniq=0.7, lr_dis=1.0,
           sky_l=None, sky_r=None, ratio=False):
    """The maps of a frame on a handle with sgm_set_window(window): oracle.process's keys, in
    true disparity (min_disp m).  cost "sad" | "ssd": the window cost volume through
    tests/volume_recipe.py, with `filters` (horizontal, vertical) through
    tests/volume_filter_recipe.py (5q).  solver "bm": "disp" (BM's raw winner-take-all) and
    "final" (its post_filter) only.  weighted: sgm_set_weighted's masked tables or weighted
    volume (tests/weighted_recipe.py) in the place of the plain ones.  The sky mask `sky`
    serves both views unless sky_l / sky_r give a view its own; ratio: census frames also
    return "ratio" / "ratio_beta", the confidence quotient (the volume recipes always do)."""
    sky_l, sky_r = masks(sky, sky_l, sky_r)
    if cost != "census":
        C = (weighted_recipe.volume if weighted else volume)(left, right, D, cost, window, s, m)
        if any(filters):
            return volume_filter_recipe.recipe(C, m, s, paths, (1 if filters[0] else 0) | (2 if filters[1] else 0),
                                               P1, P2, uniq, lr_dis)
        return volume_recipe.recipe(C, m, s, paths, P1, P2, uniq, lr_dis)
    if solver == "bm":
        ctl, ctr = (frame_census(x, window, s, blur, True, weighted) for x in (left, right))
        d = bm_wta(cost_volume(ctl, ctr, D, s, 0, sky_l), uniq)
        return {"disp": d, "final": oracle.post_filter(d.astype(np.float32), D, s)}
    ctl, ctr = (frame_census(x, window, s, blur, False, weighted) for x in (left, right))
    ctl_s, ctr_s = shift_tables(ctl, ctr, m // s)
    out = {}
    vols = [cost_volume(ctl, ctr_s, D, s, 0, sky_l)]
    if views == 2:
        vols.append(cost_volume(ctl_s, ctr, D, s, 1, sky_r))
    for C, sfx in zip(vols, ("", "_beta")):
        S = aggregate(C, paths, P1, P2)
        d = oracle.wta(S, uniq)
        if ratio:
            out["ratio" + sfx] = ratio_of(S)
        out["disp" + sfx] = d + m
        out["sub" + sfx] = (oracle.subpixel(d, S) + np.float32(m)).astype(np.float32)
    if views == 2:
        out["lr"] = oracle.lr_check(out["sub"], out["sub_beta"], D + m, s, lr_dis)
        out["final"] = oracle.post_filter(out["lr"], D + m, s)
    else:
        out["final"] = oracle.post_filter(out["sub"], D + m, s)
    return out
