"""The reference's CT cost as a cost volume (SGM_COST_CT), in
numpy: a literal restatement of CT (cost.cpp:62-96), of hamming_cost
(cost.cpp:132-144) and of Solver::build_dsi's loop (Solver.cpp:96-117) in the
reference's order, with its two 64-bit words; and the vectorised form the GPU
tests compare with (a count of differing kept taps).  tests/test_ct_cost_cpu.py
checks that the two agree bit for bit and pins the literal form to fixtures
written by the reference's own compiled CT (tests/golden/make_ref_ct_golden.py).

CT is called with `scale` passed, as the SAD / SSD recipe calls its functions:
the taps shift by disp / scale, the right centre by disp itself (cost.cpp:69).

The cases are the window-cost tests' pairs (window_cost_cases.py) on the default
window, and window_cases.py's pairs under a set window, weighted or not.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools
import os

import numpy as np

import weighted_recipe as wt
import window_cases
import window_cost_cases
from window_cost_recipe import WIN_H, WIN_W, bits, derive_right, working  # noqa: F401

GOLDEN_DIR = os.path.join(window_cases.GOLDEN, "ct")
M64 = (1 << 64) - 1

# name: (source, pair's name, D, scale, min_disp, window as sgm_set_window takes it or None, weighted)
# source "cost": window_cost_cases.inputs(name); "window": window_cases.cost_pair(name, scale)
CASES = {
    "min_3x5_D32": ("cost", "min_3x5_D32", 32, 1, 0, None, False),            # the window is larger than the image
    "s2_6x10_D32": ("cost", "s2_6x10_D32", 32, 2, 0, None, False),            # scale 2: centre by disp, taps by disp / 2
    "odd_s2_51x99_D32": ("cost", "odd_s2_51x99_D32", 32, 2, 0, None, False),
    "edge_24x33_D32": ("cost", "edge_24x33_D32", 32, 1, 0, None, False),      # W = D + 1
    "m16_s2_20x66_D32": ("cost", "m16_s2_20x66_D32", 32, 2, 16, None, False),  # min_disp at scale 2
    "narrow_24x33_D64": ("window", "24x33", 64, 1, 0, None, False),           # W < D: most taps skipped, centre clamped
    "win_9x7": ("window", "24x33", 32, 1, 0, (9, 7), False),
    "win_5x9": ("window", "24x33", 32, 1, 0, (5, 9), False),
    "win_3x3": ("window", "24x33", 32, 1, 0, (3, 3), False),
    "win_1x9": ("window", "24x33", 32, 1, 0, (1, 9), False),
    "weighted_7x9": ("window", "24x33", 32, 1, 0, (7, 9), True),
    "weighted_5x5": ("window", "24x33", 32, 1, 0, (5, 5), True),
    "weighted_s2_14x18": ("window", "20x70", 32, 2, 0, (14, 18), True),
    # GPU only (no fixture: the vectorised form, which the cases above pin)
    "narrow_20x40_D128": ("cost", "narrow_20x40_D128", 128, 1, 0, None, False),
    "road_48x170_D64": ("cost", "road_48x170_D64", 64, 1, 0, None, False),
    "wide_36x300_D256": ("cost", "wide_36x300_D256", 256, 1, 0, None, False),
    "m16_48x170_D64": ("cost", "m16_48x170_D64", 64, 1, 16, None, False),
}
GOLDEN = [k for k in CASES if k not in ("narrow_20x40_D128", "road_48x170_D64", "wide_36x300_D256",
                                        "m16_48x170_D64")]


def inputs(name):
    """The case's full-size pair."""
    source, pair, _, scale, _, _, _ = CASES[name]
    return window_cost_cases.inputs(pair) if source == "cost" else window_cases.cost_pair(pair, scale)


def effective(name):
    """(e_h, e_w): the window CT is called with, win / scale."""
    _, _, _, scale, _, window, _ = CASES[name]
    return window_cases.effective(window or (WIN_H, WIN_W), scale)


def fixture(name):
    return os.path.join(GOLDEN_DIR, f"ref_ct_{name}.npz")


# ------------------------------------------------------------------ literal
def hamming_cost(ct_l, ct_r):
    not_the_same = ct_l ^ ct_r
    cnt = 0
    while not_the_same:
        cnt += not_the_same & 1
        not_the_same >>= 1
    return cnt


def ct(img_l, img_r, rows, cols, x, y, disp, win_h, win_w, weight, scale):
    """CT(img_l, img_r, Point(x, y), disp, win_h, win_w, weight, scale), line by line; the
    images as lists of rows, weight the flat table or None (WEIGHTED_COST = 0)."""
    ct_l = ct_r = 0
    ctr_pixel_l = img_l[y][x]
    ctr_pixel_r = img_r[y][max(x - disp, 0)]
    for i in range(-(win_h // 2), win_h // 2 + 1):
        yy = max(y + i, 0)
        yy = min(yy, rows - 1)
        ptr_l, ptr_r = img_l[yy], img_r[yy]
        for j in range(-(win_w // 2), win_w // 2 + 1):
            if i == 0 and j == 0:
                continue
            if weight is not None and weight[(i + win_h // 2) * win_w + (j + win_w // 2)] < 0.5:
                continue
            x_l = max(x + j, 0)
            x_l = min(x_l, cols - 1)
            x_r = x_l - disp // scale
            if x_r < 0:
                continue
            ct_l = ((ct_l | (ptr_l[x_l] > ctr_pixel_l)) << 1) & M64
            ct_r = ((ct_r | (ptr_r[x_r] > ctr_pixel_r)) << 1) & M64
    return hamming_cost(ct_l, ct_r)


def build_dsi(L, R, D, e_h, e_w, scale=1, min_disp=0, weighted=False):
    """Solver::build_dsi over CT on working-grid images: (rows, cols, D) float32, index d
    standing for disparity min_disp + d."""
    rows, cols = L.shape
    weight = [float(w) for w in wt.weights(e_h, e_w).ravel()] if weighted else None
    img_l, img_r = L.tolist(), R.tolist()
    cost = np.empty((rows, cols, D), np.float32)
    for i in range(rows):
        for j in range(cols):
            for d in range(D):
                cost[i, j, d] = ct(img_l, img_r, rows, cols, j, i, d + min_disp, e_h, e_w, weight, scale)
    return cost


# --------------------------------------------------------------- vectorised
def kept(e_h, e_w, weighted=False):
    """The taps CT keeps, (2 hh + 1, 2 hw + 1) bool: not the centre; weighted: weight >= 0.5."""
    hh, hw = e_h // 2, e_w // 2
    k = np.ones((2 * hh + 1, 2 * hw + 1), bool)
    if weighted:
        assert e_h % 2 == 1 and e_w % 2 == 1
        k = ~(wt.weights(e_h, e_w) < 0.5)
    k[hh, hw] = False
    return k


def build_dsi_vec(L, R, D, e_h, e_w, scale=1, min_disp=0, weighted=False):
    """The same volume tap by tap for every (row, column, d) at once: the count of kept,
    unskipped taps at which the two census bits differ."""
    rows, cols = L.shape
    hh, hw = e_h // 2, e_w // 2
    keep = kept(e_h, e_w, weighted)
    assert keep.sum() <= 62  # no bit leaves the reference's words
    disp = np.arange(D) + min_disp
    k = disp // scale
    yy, xx = np.arange(rows), np.arange(cols)
    cl = L                                                   # (rows, cols)
    cr = R[:, np.maximum(xx[:, None] - disp[None, :], 0)]    # (rows, cols, D): disp, not k
    cost = np.zeros((rows, cols, D), np.int32)
    for a in range(-hh, hh + 1):
        y = np.clip(yy + a, 0, rows - 1)
        for b in range(-hw, hw + 1):
            if not keep[a + hh, b + hw]:
                continue
            x_l = np.clip(xx + b, 0, cols - 1)               # (cols,)
            x_r = x_l[:, None] - k[None, :]                  # (cols, D)
            bit_l = L[y][:, x_l] > cl                        # (rows, cols)
            bit_r = R[y][:, np.maximum(x_r, 0)] > cr         # (rows, cols, D)
            cost += (bit_l[:, :, None] != bit_r) & (x_r >= 0)[None]
    return cost.astype(np.float32)


def volume(left, right, D, scale=1, min_disp=0, window=None, weighted=False):
    """The left CT volume of two full-size grey images, as a frame or window_cost builds it."""
    e_h, e_w = window_cases.effective(window or (WIN_H, WIN_W), scale)
    return build_dsi_vec(working(left, scale), working(right, scale), D, e_h, e_w, scale, min_disp, weighted)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The case's left volume by the vectorised form (computed once, shared, read-only)."""
    _, _, D, scale, m, window, weighted = CASES[name]
    left, right = inputs(name)
    v = volume(left, right, D, scale, m, window, weighted)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's compiled CT over the case (the fixture), as float32; read-only."""
    with np.load(fixture(name)) as z:
        v = z["ct"].astype(np.float32)
    v.setflags(write=False)
    return v


# ----------------------------------------------------------------- identity
def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(*x.shape, 8), axis=-1).sum(axis=-1)


def table_region(cols, D, e_w, min_disp=0):
    """(cols, D) bool: where, at scale 1, no tap is skipped or clamped in x, so that CT equals
    the Hamming distance of two census tables: hw <= j <= cols - 1 - hw and j - disp >= hw."""
    hw = e_w // 2
    j = np.arange(cols)[:, None]
    disp = np.arange(D)[None, :] + min_disp
    return (j >= hw) & (j <= cols - 1 - hw) & (j - disp >= hw)
