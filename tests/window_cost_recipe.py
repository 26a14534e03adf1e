"""The reference's SAD / SSD window costs as a cost volume, in
numpy: a literal restatement of SAD, SSD (cost.cpp:4-59) and Solver::build_dsi
(Solver.cpp:96-117) in the reference's loop order, with np.float32 accumulation
and two np.float32 divisions, and the separable integer form the kernel's
arithmetic follows.  tests/test_window_cost_cpu.py checks that the two agree bit
for bit and pins the literal form to fixtures written by the reference's own
compiled functions.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

from paths4_recipe import bits  # noqa: F401
from volume_recipe import derive_right  # noqa: F401  (the right view's volume of a left one)

KINDS = ("sad", "ssd")
WIN_H, WIN_W = 7, 9  # inc/Solver.h


def working(img, scale):
    """The working-grid image the census and the window costs read: every
    scale-th row and column of the full-size one (SGM.cpp:47-48)."""
    h, w = img.shape
    return np.ascontiguousarray(img[:(h // scale) * scale:scale, :(w // scale) * scale:scale])


def window_cost(img_l, img_r, x, y, disp, win_h, win_w, scale, kind):
    """SAD / SSD(img_l, img_r, Point(x, y), disp, win_h, win_w, weight, scale)
    with WEIGHTED_COST = 0, line by line (cost.cpp:4-30, :33-59)."""
    rows, cols = img_l.shape
    cost = np.float32(0)
    for i in range(-(win_h // 2), win_h // 2 + 1):
        yy = max(y + i, 0)
        yy = min(yy, rows - 1)
        for j in range(-(win_w // 2), win_w // 2 + 1):
            x_l = max(x + j, 0)
            x_l = min(x_l, cols - 1)
            x_r = max(x_l - disp // scale, 0)
            diff = int(img_l[yy, x_l]) - int(img_r[yy, x_r])
            cost = np.float32(cost + np.float32(abs(diff) if kind == "sad" else diff * diff))
    return np.float32(np.float32(cost / np.float32(win_h)) / np.float32(win_w))


def build_dsi(L, R, D, kind, scale=1, min_disp=0):
    """Solver::build_dsi over SAD or SSD on working-grid images L, R: (rows,
    cols, D) float32, index d standing for disparity min_disp + d."""
    rows, cols = L.shape
    win_h, win_w = WIN_H // scale, WIN_W // scale
    cost = np.empty((rows, cols, D), np.float32)
    for i in range(rows):
        for j in range(cols):
            for d in range(D):
                cost[i, j, d] = window_cost(L, R, j, i, d + min_disp, win_h, win_w, scale, kind)
    return cost


def build_dsi_separable(L, R, D, kind, scale=1, min_disp=0):
    """The same volume by integer sums: AD at clamped coordinates, summed over
    the window's rows, then over its columns, then the two divisions."""
    rows, cols = L.shape
    win_h, win_w = WIN_H // scale, WIN_W // scale
    hh, hw = win_h // 2, win_w // 2
    Li, Ri = L.astype(np.int64), R.astype(np.int64)
    x = np.arange(cols)[:, None]
    xr = np.maximum(x - (np.arange(D)[None, :] + min_disp) // scale, 0)  # (cols, D)
    ad = np.abs(Li[:, :, None] - Ri[:, xr])                             # (rows, cols, D)
    if kind == "ssd":
        ad = ad * ad
    yi = np.clip(np.arange(rows)[:, None] + np.arange(-hh, hh + 1)[None, :], 0, rows - 1)
    col = ad[yi].sum(axis=1)                                             # (rows, cols, D)
    xi = np.clip(np.arange(cols)[:, None] + np.arange(-hw, hw + 1)[None, :], 0, cols - 1)
    tot = col[:, xi].sum(axis=2)
    assert tot.max(initial=0) <= 63 * 255 * 255
    return ((tot.astype(np.float32) / np.float32(win_h)) / np.float32(win_w)).astype(np.float32)


def volume(left, right, D, kind, scale=1, min_disp=0):
    """The left cost volume of two full-size grey images, as a frame builds it."""
    return build_dsi_separable(working(left, scale), working(right, scale), D, kind, scale, min_disp)


