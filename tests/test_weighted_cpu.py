"""Weighted windows on the CPU (sgm_set_weighted): the recipe of
tests/weighted_recipe.py against the fixtures the reference's own compiled
CT_pts, SAD and SSD wrote with WEIGHTED_COST on (tests/golden/weighted/), bit for
bit over every element; against the unweighted recipes with weighting off; the
kept-bit counts; the weight table; the refusal rule."""
from __future__ import annotations

import numpy as np
import pytest

import weighted_recipe as wt
import window_cases as cases
import window_cost_recipe as wc
import window_recipe as wr


def census_id(c):
    shape, s, win = c
    return f"{shape[0]}x{shape[1]}_s{s}_{cases.wid(win)}"


CENSUS_CASES = [(shape, s, win) for s in (1, 2) for shape in wt.CENSUS_SHAPES for win in wt.CENSUS_WINDOWS[s]]


@pytest.mark.parametrize("case", CENSUS_CASES, ids=census_id)
def test_masked_census_equals_the_reference(case):
    shape, s, win = case
    left, right = cases.census_pair(shape, s)
    for img, want in zip((left, right), cases.ref_census(shape, s, win, "weighted")):
        assert np.array_equal(wr.census(cases.working(img, s), *cases.effective(win, s), weighted=True), want)


@pytest.mark.parametrize("case", wt.COST_FIXTURES, ids=lambda c: f"{c[0]}_s{c[1]}_{cases.wid(c[2])}")
@pytest.mark.parametrize("kind", cases.KINDS)
def test_weighted_volume_equals_the_reference(case, kind):
    name, s, win = case
    left, right = cases.cost_pair(name, s)
    got = wt.volume(left, right, cases.COST_DMAX, kind, win, s)
    want = cases.ref_cost(name, s, win, kind, "weighted")
    assert got.dtype == np.float32 and np.array_equal(wr.bits(got), wr.bits(want))


def test_a_min_disp_case_is_a_slice_of_the_fixture():
    left, right = cases.cost_pair("24x33", 2)
    got = wt.volume(left, right, 64, "sad", (14, 18), 2, min_disp=16)
    want = np.ascontiguousarray(cases.ref_cost("24x33", 2, (14, 18), "sad", "weighted")[:, :, 16:80])
    assert np.array_equal(wr.bits(got), wr.bits(want))


@pytest.mark.parametrize("win", wt.COST_WINDOWS[1], ids=cases.wid)
def test_weighting_off_is_the_unweighted_recipe(win):
    left, right = cases.cost_pair("24x33", 1)
    L, R = cases.working(left, 1), cases.working(right, 1)
    assert np.array_equal(wr.census(L, *win, weighted=False), wr.census(L, *win))
    for kind in cases.KINDS:
        got = wt.window_volume(L, R, 40, kind, *win, 1, 16, weighted=False)
        assert np.array_equal(wr.bits(got), wr.bits(wr.window_volume(L, R, 40, kind, *win, 1, 16)))


def test_weighting_off_is_the_literal_window_cost():
    left, right = cases.cost_pair("3x5", 1)
    for kind in cases.KINDS:
        got = wt.window_volume(left, right, 8, kind, 7, 9, 1, 0, weighted=False)
        assert np.array_equal(wr.bits(got), wr.bits(wc.build_dsi(left, right, 8, kind)))


def test_weighting_changes_the_widest_windows_and_only_those():
    left, _ = cases.census_pair((17, 65), 1)
    for win, bits in wt.KEPT_BITS.items():
        full = win[0] * win[1] - 1
        assert int(wt.kept(*win).sum()) == bits <= full
        same = np.array_equal(wr.census(left, *win, weighted=True), wr.census(left, *win, weighted=False))
        assert same == (bits == full), win
        # the disc of the issue, da^2 + db^2 <= 17
        a, b = np.meshgrid(np.arange(win[0]) - win[0] // 2, np.arange(win[1]) - win[1] // 2, indexing="ij")
        assert np.array_equal(wt.kept(*win), (a * a + b * b <= 17) & ((a != 0) | (b != 0)))
        # a masked word never carries more bits than it keeps
        assert int(wr.census(left, *win, weighted=True).max()) < 1 << bits


def test_weight_table_equals_the_recorded_one():
    with np.load(wt.WEIGHTS_FIXTURE) as z:
        assert sorted(z.files) == sorted(f"{a}x{b}" for a, b in wt.weight_windows())
        for e_h, e_w in wt.weight_windows():
            w = wt.weights(e_h, e_w)
            assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), z[f"{e_h}x{e_w}"].view(np.uint32))
            assert w[e_h // 2, e_w // 2] == 1.0 and (w > 0.36).all()  # exp(-25 / 25) at the farthest tap


@pytest.mark.parametrize("ok,window,s", wt.RULE, ids=lambda v: str(v).replace(" ", ""))
def test_refusal_rule(ok, window, s):
    assert (wt.refusal(window, s) is None) == ok
    if wr_accepts(window, s) and not ok:
        assert wt.refusal(window, s) == "odd"


def wr_accepts(window, s):
    e_h, e_w = cases.effective(window, s)
    return (1 <= e_h <= 9 and 1 <= e_w <= 9 and not (e_h // 2 == 0 and e_w // 2 == 0)
            and (2 * (e_h // 2) + 1) * (2 * (e_w // 2) + 1) - 1 <= 64)


def test_every_case_window_is_accepted():
    for s, wins in wt.COST_WINDOWS.items():
        for win in wins:
            assert wt.refusal(win, s) is None
