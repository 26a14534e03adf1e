"""The filtered-volume recipe (tests/volume_filter_recipe.py) against the oracle,
on the CPU: fed the raw census DSI of an image pair it is oracle.process, the
one-tap vertical window is not the identity, and the undershoot volume really
goes below zero."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import volume_filter_recipe as fr
import volume_recipe as vr


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.build()


@pytest.mark.parametrize("h,w,D,s", [(24, 80, 32, 1), (20, 40, 128, 1), (24, 80, 32, 2)])
def test_raw_census_dsi_through_the_recipe_is_process(h, w, D, s):
    left, right = vr.road_pair(h, w, D, s)
    ctl, ctr = vr.road_tables(h, w, D, s)
    raw = oracle.dsi(ctl, ctr, D, s, 0, None)
    ref = oracle.process(left, right, D, scale=s, views=1)
    disp, sub, _ = vr.view_maps(fr.filtered(raw, s), 0, 8)
    assert np.array_equal(fr.bits(sub), fr.bits(ref["sub"]))
    assert np.array_equal(disp, ref["disp"])
    assert np.array_equal(fr.bits(fr.recipe(raw, 0, s)["sub"]), fr.bits(ref["sub"]))


def test_window_one_is_not_the_identity():
    C = fr.mixed_volume(9, 12, 32)
    assert not np.array_equal(fr.bits(oracle.vfilter(C, 1)), fr.bits(C))
    assert not np.array_equal(fr.bits(oracle.hfilter(C, 1)), fr.bits(C))


def test_the_undershoot_volume_goes_below_zero():
    # (the 5-wide window: it subtracts outputs two steps old; the 2-wide one subtracts its own)
    C = fr.undershoot_volume(9, 40, 32)
    assert C.min() >= 0.0
    assert oracle.hfilter(C, 5).min() < 0.0
    assert fr.filtered(C, 1).min() < 0.0


def test_two_views_derive_then_filter_is_not_filter_then_derive():
    C = fr.frame_volume(12, 37, 32)
    a, b = fr.recipe(C), fr.caller_side(C)
    assert np.array_equal(fr.bits(a["sub"]), fr.bits(b["sub"]))  # the left view is the same
    assert not np.array_equal(fr.bits(a["sub_beta"]), fr.bits(b["sub_beta"]))
