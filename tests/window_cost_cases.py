"""The seeded image pairs of the window-cost tests: shared by the
CPU tests, the GPU tests and tests/golden/make_ref_window_cost_golden.py.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools

import numpy as np

import window_cost_recipe as wc
from stereo_matching_amd import synthetic

# name: (h, w, D, scale, min_disp, image kind, pair index); h, w the full-size images'
CASES = {
    "min_3x5_D32": (3, 5, 32, 1, 0, "noise", 0),            # the window is larger than the image
    "s2_6x10_D32": (6, 10, 32, 2, 0, "noise", 1),           # 3 x 5 taps, divisors 3 and 4
    "odd_s2_51x99_D32": (51, 99, 32, 2, 0, "road", 2),      # odd sizes at scale 2
    "edge_24x33_D32": (24, 33, 32, 1, 0, "noise", 3),       # W = D + 1
    "narrow_20x40_D128": (20, 40, 128, 1, 0, "road", 4),    # W < D: max(., 0) over most of the volume
    "road_48x170_D64": (48, 170, 64, 1, 0, "road", 5),      # crosses column-tile edges
    "wide_36x300_D256": (36, 300, 256, 1, 0, "road", 6),    # the widest disparity range
    "m16_48x170_D64": (48, 170, 64, 1, 16, "road", 5),      # min_disp = 16 on the same pair
    "m16_s2_20x66_D32": (20, 66, 32, 2, 16, "noise", 7),    # min_disp at scale 2
    "extreme_10x20_D32": (10, 20, 32, 1, 0, "extreme", 0),  # all 255 against all 0: the largest sums
}
# the cases small enough for a full volume of both kinds in a committed fixture
GOLDEN = {k: CASES[k][:5] for k in ("min_3x5_D32", "s2_6x10_D32", "odd_s2_51x99_D32", "edge_24x33_D32",
                                    "m16_s2_20x66_D32", "extreme_10x20_D32")}


def pair(h, w, D, kind, index):
    if kind == "extreme":
        return np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    return synthetic.stereo_pair(h, w, D, pair_index=index, kind=kind)


def inputs(name):
    h, w, D, _, _, kind, index = CASES[name]
    return pair(h, w, D, kind, index)


@functools.lru_cache(maxsize=None)
def expected(name, kind):
    """The case's left volume by the recipe (computed once, shared, read-only)."""
    h, w, D, scale, m, _, _ = CASES[name]
    left, right = inputs(name)
    v = wc.volume(left, right, D, kind, scale, m)
    v.setflags(write=False)
    return v
