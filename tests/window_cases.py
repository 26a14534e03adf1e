"""The seeded images and the case lists of the matching-window tests (DESIGN.md
5p): shared by the CPU tests, the GPU tests and
tests/golden/make_ref_window_golden.py.

A window is written as sgm_set_window takes it, (win_h, win_w) before the
division by the scale; the reference's functions see (win_h // s, win_w // s).

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools
import os

import numpy as np

# (directories of their own: tests/test_reference_parity.py bounds the files of tests/golden itself)
# family "window": the plain windows' fixtures; "weighted": tests/weighted_recipe.py's
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_DIR = os.path.join(GOLDEN, "window")

# ------------------------------------------------------------------ census
# working-grid shapes around the census kernel's 64 x 16 tile (four waves of four rows)
CENSUS_SHAPES = [(3, 5), (16, 64), (17, 65), (20, 70), (33, 130)]
# by scale: 3x3 (8 bits), 5x7 (34 bits: two in the high word), 9x7 and 7x9 (62 bits), HH = 0,
# HW = 0, an even width; at scale 2 (9, 9) -> 4 x 4 -> 5 x 5 taps and the default (7, 9) -> 3 x 4
CENSUS_WINDOWS = {
    1: [(3, 3), (5, 5), (5, 7), (7, 7), (9, 7), (7, 9), (1, 9), (9, 1), (3, 8)],
    2: [(9, 9), (7, 9)],
}

# ------------------------------------------------------------ window costs
# working-grid shapes: smaller than any window, the largest sums, two column tiles, W = 33
COST_SHAPES = {"3x5": (3, 5, "noise"), "10x20": (10, 20, "extreme"), "20x70": (20, 70, "noise"),
               "24x33": (24, 33, "noise")}
COST_WINDOWS = {
    1: [(3, 3), (5, 5), (9, 7), (5, 6), (1, 9)],
    2: [(10, 12)],  # -> 5 x 6
}
COST_S2_SHAPES = ("20x70", "24x33")
COST_D = (32, 64)
COST_MIN_DISP = (0, 16)
# a fixture holds disparities 0 .. COST_DMAX - 1; a case (D, m) is its slice [m, m + D): SAD and
# SSD take the disparity itself, so index d of a handle with min_disp m is disparity m + d
COST_DMAX = max(COST_D) + max(COST_MIN_DISP)
KINDS = ("sad", "ssd")


def effective(window, s):
    return window[0] // s, window[1] // s


def wid(window):
    return f"{window[0]}x{window[1]}"


def image(h, w, seed):
    """Noise on a grid of 32 grey levels: neighbours equal to the centre are common, so the
    census's strict `>` is exercised."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 32, (h, w)) * 8 + rng.integers(0, 2, (h, w)) * 7).astype(np.uint8)


def full_pair(rows, cols, s, seed, kind="noise"):
    """A full-size pair whose working grid is rows x cols at scale s."""
    h, w = rows * s, cols * s
    if kind == "extreme":
        return np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    return image(h, w, seed), image(h, w, seed + 1000)


def working(img, s):
    h, w = img.shape
    return np.ascontiguousarray(img[:(h // s) * s:s, :(w // s) * s:s])


def census_pair(shape, s):
    rows, cols = shape
    return full_pair(rows, cols, s, 100 * rows + cols + s)


def cost_pair(name, s):
    rows, cols, kind = COST_SHAPES[name]
    return full_pair(rows, cols, s, 7 * rows + cols + s, kind)


def census_cases():
    return [(shape, s, win) for s in (1, 2) for shape in CENSUS_SHAPES for win in CENSUS_WINDOWS[s]]


def cost_fixture_cases():
    out = [(name, 1, win) for name in COST_SHAPES for win in COST_WINDOWS[1]]
    return out + [(name, 2, win) for name in COST_S2_SHAPES for win in COST_WINDOWS[2]]


def census_fixture(shape, s, family="window"):
    return os.path.join(GOLDEN, family, f"ref_{family}_ct_{shape[0]}x{shape[1]}_s{s}.npz")


def cost_fixture(name, s, window, family="window"):
    return os.path.join(GOLDEN, family, f"ref_{family}_ad_{name}_s{s}_{wid(window)}.npz")


@functools.lru_cache(maxsize=None)
def ref_census(shape, s, window, family="window"):
    """(table of the left image, of the right image) by the reference's CT_pts; read-only."""
    with np.load(census_fixture(shape, s, family)) as z:
        out = z["l_" + wid(window)], z["r_" + wid(window)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_cost(name, s, window, kind, family="window"):
    """The reference's SAD or SSD volume over disparities 0 .. COST_DMAX - 1; read-only."""
    with np.load(cost_fixture(name, s, window, family)) as z:
        v = z[kind]
    v.setflags(write=False)
    return v
