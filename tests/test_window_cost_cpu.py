"""The window-cost recipe on the CPU (tests/window_cost_recipe.py, DESIGN.md
5o): the literal restatement of SAD / SSD / build_dsi agrees bit for bit with
its separable integer form, and both with the fixtures that the reference's own
compiled SAD and SSD wrote (tests/golden/make_ref_window_cost_golden.py)."""
from __future__ import annotations

import os

import numpy as np
import pytest

import window_cost_cases as cases
import window_cost_recipe as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (the literal form runs 63 Python steps per element: the smallest cases)
LITERAL = ["min_3x5_D32", "s2_6x10_D32", "extreme_10x20_D32", "m16_s2_20x66_D32"]


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", LITERAL)
def test_literal_and_separable_forms_agree(name, kind):
    h, w, D, scale, m, _, _ = cases.CASES[name]
    left, right = cases.inputs(name)
    L, R = wc.working(left, scale), wc.working(right, scale)
    lit = wc.build_dsi(L, R, D, kind, scale, m)
    assert lit.shape == (h // scale, w // scale, D) and lit.dtype == np.float32
    assert np.array_equal(wc.bits(lit), wc.bits(cases.expected(name, kind)))


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", sorted(cases.GOLDEN))
def test_recipe_equals_the_references_own_functions(name, kind):
    ref = np.load(os.path.join(GOLDEN, f"ref_window_cost_{name}.npz"))[kind]
    assert np.array_equal(wc.bits(ref), wc.bits(cases.expected(name, kind)))


def test_the_extreme_pair_reaches_the_largest_cost():
    assert (cases.expected("extreme_10x20_D32", "ssd") == np.float32(65025)).all()
    assert (cases.expected("extreme_10x20_D32", "sad") == np.float32(255)).all()


def test_scale_two_divides_fifteen_taps_by_three_and_four():
    # a constant difference of 1: 15 taps / 3 / 4, not 1
    L, R = np.full((4, 6), 9, np.uint8), np.full((4, 6), 8, np.uint8)
    v = wc.build_dsi_separable(L, R, 32, "sad", 2)
    assert (v == np.float32(np.float32(15) / np.float32(3)) / np.float32(4)).all()
    assert np.array_equal(wc.bits(v), wc.bits(wc.build_dsi(L, R, 32, "sad", 2)))


def test_two_divisions_are_not_one():
    # sums whose two-step quotient differs from sum / 63 exist, so the order is part of the definition
    x = np.arange(0, 63 * 255 + 1, dtype=np.float32)
    assert (wc.bits(x / np.float32(7) / np.float32(9)) != wc.bits(x / np.float32(63))).any()
