"""Weighted windows (sgm_set_weighted), in numpy: the reference's
cost functions with WEIGHTED_COST on, restated literally.

  weights(e_h, e_w)      Solver::Solver's Gaussian table (Solver.cpp:29-45)
  refusal(window, s)     the rule of sgm_set_weighted / sgm_set_window on a weighted handle
  kept(e_h, e_w)         the taps CT_pts (cost.cpp:99-129) keeps: weight >= 0.5
  window_volume(...)     Solver::build_dsi over SAD / SSD (cost.cpp:4-59): the taps in the
                         reference's order (rows outer, columns inner), cost = cost + AD * w in
                         fp32 (numpy multiplies, rounds, then adds: no FMA), two fp32 divisions

(the masked census and whole frames are tests/window_recipe.py's census, frame_census and
recipe with weighted=True) and the case lists of the tests and of tests/golden/make_ref_weighted_golden.py,
which writes the fixtures under tests/golden/weighted/ with the reference's own
compiled functions; tests/test_weighted_cpu.py pins everything here to them.
The images, the shapes and the fixture loaders (family="weighted") are
tests/window_cases.py's.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np

from window_cases import GOLDEN, effective, working

GOLDEN_DIR = os.path.join(GOLDEN, "weighted")

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


WEIGHTS_FIXTURE = os.path.join(GOLDEN_DIR, "ref_weighted_weights.npz")


def weight_windows():
    """Every effective window a fixture or a test uses."""
    out = []
    for s, wins in COST_WINDOWS.items():
        for w in wins:
            if effective(w, s) not in out:
                out.append(effective(w, s))
    return out


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
