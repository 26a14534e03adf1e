"""The CT cost (SGM_COST_CT) on the CPU: tests/ct_cost_recipe.py's
literal restatement of CT and build_dsi against the fixtures the reference's own
compiled CT wrote (tests/golden/ct/), the vectorised form against the literal
one, the identity with the Hamming distance of two unblurred census tables inside
its region (and not outside it), and the host side of the kernel
(csrc/sgm_window_cost_args.h) as a stand-alone program under sanitizers."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import ct_cost_recipe as ct
import window_recipe
import support
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def literal(name):
    _, _, D, scale, m, _, weighted = ct.CASES[name]
    left, right = ct.inputs(name)
    v = ct.build_dsi(ct.working(left, scale), ct.working(right, scale), D, *ct.effective(name), scale, m, weighted)
    v.setflags(write=False)
    return v


def test_the_cases_the_issue_names_have_fixtures():
    assert {"min_3x5_D32", "s2_6x10_D32", "odd_s2_51x99_D32", "edge_24x33_D32", "m16_s2_20x66_D32"} <= set(ct.GOLDEN)
    windows = {(ct.CASES[n][5], ct.CASES[n][6], ct.CASES[n][3]) for n in ct.GOLDEN}
    assert {((9, 7), False, 1), ((5, 9), False, 1), ((3, 3), False, 1), ((1, 9), False, 1), ((7, 9), True, 1),
            ((5, 5), True, 1), ((14, 18), True, 2)} <= windows
    for name in ct.GOLDEN:
        assert os.path.getsize(ct.fixture(name)) < 1 << 20
    # the W < D case: most taps skipped (the cost 0 of a pixel with every tap off the left edge
    # fills over half of the volume's elements with j < disp) and the centre clamped
    _, _, D, _, _, _, _ = ct.CASES["narrow_24x33_D64"]
    v = ct.reference("narrow_24x33_D64")
    assert v.shape[1] < D
    j, d = np.arange(v.shape[1])[:, None], np.arange(D)[None, :]
    assert (j < d).mean() > 0.5 and (v[:, (j + 4 < d)] == 0).all()


@pytest.mark.parametrize("name", ct.GOLDEN)
def test_literal_recipe_equals_the_reference(name):
    ref = ct.reference(name)
    got = literal(name)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(ct.bits(got), ct.bits(ref))
    assert ref.min() >= 0 and ref.max() <= 62 and ref.max() > 0


@pytest.mark.parametrize("name", ct.GOLDEN)
def test_vectorised_form_equals_the_literal(name):
    assert np.array_equal(ct.bits(ct.expected(name)), ct.bits(literal(name)))


def test_scale_2_centre_uses_the_disparity_itself():
    # with the centre column at disp / 2 instead (what a consistent reading would do) the
    # volume differs: the fixture pins cost.cpp:69 as it is written
    name = "m16_s2_20x66_D32"
    _, _, D, scale, m, _, _ = ct.CASES[name]
    left, right = ct.inputs(name)
    L, R = ct.working(left, scale), ct.working(right, scale)
    # CT with disp and scale 1 shifts the centre and the taps alike: feed it disp / 2
    consistent = np.stack([ct.build_dsi_vec(L, R, 1, *ct.effective(name), 1, (d + m) // scale)[:, :, 0]
                           for d in range(D)], axis=2)
    assert not np.array_equal(consistent, ct.reference(name))


@pytest.mark.parametrize("name", ["edge_24x33_D32", "narrow_24x33_D64", "win_5x9", "win_3x3", "weighted_7x9",
                                  "weighted_5x5"])
def test_identity_with_the_census_tables(name):
    """Scale 1, hw <= j <= cols - 1 - hw and j - disp >= hw: CT is the popcount of the XOR of the
    two CT_pts tables of the unblurred images (the oracle's: window_recipe.census); outside the
    region the census DSI is another volume."""
    _, _, D, scale, m, _, weighted = ct.CASES[name]
    assert scale == 1
    e_h, e_w = ct.effective(name)
    left, right = ct.inputs(name)
    tl, tr = (window_recipe.census(img, e_h, e_w, weighted) for img in (left, right))
    rows, cols = left.shape
    xr = np.maximum(np.arange(cols)[:, None] - (np.arange(D)[None, :] + m), 0)   # the census DSI's column
    ham = ct.popcount(tl[:, :, None] ^ tr[:, xr]).astype(np.float32)              # (rows, cols, D)
    v = ct.reference(name)
    region = ct.table_region(cols, D, e_w, m)
    assert region.any() and not region.all()
    assert np.array_equal(v[:, region], ham[:, region])
    assert (v[:, ~region] != ham[:, ~region]).any()


def test_kernel_arithmetic_runs_clean_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "ct_args_main.cpp"))
    r = support.run(exe, timeout=300)
    assert r.returncode == 0 and "ct args ok" in r.stdout, r.stdout + r.stderr


def test_the_names():
    assert _capi.COST_KINDS == {"census": 0, "sad": 1, "ssd": 2, "ct": 4}
    assert 3 not in _capi.COST_KINDS.values() and "mi" not in _capi.COST_KINDS
