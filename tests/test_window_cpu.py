"""The matching-window recipe (tests/window_recipe.py) on the CPU:
equal to every fixture the reference's own compiled CT_pts, SAD and SSD wrote
(tests/golden/make_ref_window_golden.py), and at the default (7, 9) equal to
oracle.census, tests/window_cost_recipe.py and oracle.process."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
import window_cases as cases
import window_cost_recipe as wc
import window_recipe as wr
from stereo_matching_amd import synthetic


def test_every_fixture_is_committed_and_small():
    paths = {cases.census_fixture(shape, s) for shape, s, _ in cases.census_cases()}
    paths |= {cases.cost_fixture(*c) for c in cases.cost_fixture_cases()}
    for p in sorted(paths):
        assert os.path.getsize(p) < 1 << 20, p


@pytest.mark.parametrize("shape,s,window", cases.census_cases(),
                         ids=[f"{a[0]}x{a[1]}_s{s}_{cases.wid(w)}" for a, s, w in cases.census_cases()])
def test_census_recipe_equals_the_reference(shape, s, window):
    left, right = cases.census_pair(shape, s)
    want_l, want_r = cases.ref_census(shape, s, window)
    e_h, e_w = cases.effective(window, s)
    assert np.array_equal(wr.census(cases.working(left, s), e_h, e_w), want_l)
    assert np.array_equal(wr.census(cases.working(right, s), e_h, e_w), want_r)
    # (what the GPU tests hand in: the frame's table of the full-size image, not blurred)
    assert np.array_equal(wr.frame_census(left, window, s, blur=False), want_l)


def test_the_bit_counts():
    # 3x3 fills 8 bits, 5x7 34 (two above bit 31), 7x9 and 9x7 62: all-brighter neighbours set them all
    big = np.full((12, 12), 9, np.uint8)
    big[6, 6] = 0
    for (e_h, e_w), nbits in (((3, 3), 8), ((5, 7), 34), ((7, 9), 62), ((9, 7), 62), ((3, 8), 26), ((1, 9), 8)):
        assert int(wr.census(big, e_h, e_w)[6, 6]) == (1 << nbits) - 1


@pytest.mark.parametrize("name,s,window", cases.cost_fixture_cases(),
                         ids=[f"{n}_s{s}_{cases.wid(w)}" for n, s, w in cases.cost_fixture_cases()])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_cost_recipe_equals_the_reference(name, s, window, kind):
    left, right = cases.cost_pair(name, s)
    want = cases.ref_cost(name, s, window, kind)
    e_h, e_w = cases.effective(window, s)
    got = wr.window_volume(cases.working(left, s), cases.working(right, s), cases.COST_DMAX, kind, e_h, e_w, s)
    assert np.array_equal(wc.bits(got), wc.bits(want))
    # a handle's (D, min_disp) is a slice of it
    for D in cases.COST_D:
        for m in cases.COST_MIN_DISP:
            v = wr.volume(left, right, D, kind, window, s, m)
            assert np.array_equal(wc.bits(v), wc.bits(want[:, :, m:m + D])), (D, m)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_integer_sums_equal_the_literal_loops(kind):
    left, right = cases.cost_pair("3x5", 1)
    for e_h, e_w in ((5, 6), (1, 9), (9, 7)):
        assert np.array_equal(wc.bits(wr.window_volume(left, right, 8, kind, e_h, e_w)),
                              wc.bits(wr.window_volume_literal(left, right, 8, kind, e_h, e_w)))


@pytest.mark.parametrize("s", [1, 2])
def test_the_default_window_is_todays(s):
    left, right = synthetic.stereo_pair(20 * s, 70 * s, 32, pair_index=4, kind="road")
    g = cases.working(left, s)
    assert np.array_equal(wr.census(g, 7 // s, 9 // s), oracle.census(g, s))
    assert np.array_equal(wr.frame_census(left, (7, 9), s), oracle.census(oracle.blur(g), s))
    for kind in cases.KINDS:
        assert np.array_equal(wc.bits(wr.volume(left, right, 32, kind, (7, 9), s, 2 * s)),
                              wc.bits(wc.volume(left, right, 32, kind, s, 2 * s)))


@pytest.mark.parametrize("s", [1, 2])
def test_the_default_frame_is_the_oracles(s):
    h, w, D = 24 * s, 80 * s, 32
    left, right = synthetic.stereo_pair(h, w, D, pair_index=1, kind="road")
    want = oracle.process(left, right, D, s)
    got = wr.recipe(left, right, D, (7, 9), s)
    for k in want:
        wr.assert_bits_equal(got[k], want[k], k)
    bm = wr.recipe(left, right, D, (7, 9), s, solver="bm")
    wr.assert_bits_equal(bm["disp"], oracle.bm_process(left, right, D, s), "bm")


def test_a_window_changes_the_frame():
    h, w, D = 24, 80, 32
    left, right = synthetic.stereo_pair(h, w, D, pair_index=1, kind="road")
    a, b = wr.recipe(left, right, D, (7, 9)), wr.recipe(left, right, D, (5, 5))
    assert not np.array_equal(a["sub"], b["sub"])
