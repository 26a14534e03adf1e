"""tests/frame_recipe.py earns its trust on the CPU, bit for bit: against
oracle.process at the defaults and with P1, P2, the uniqueness ratio and the LR
threshold moved; against each setting's own recipe with that setting alone on;
against tests/pyref.py's independent loops where the oracle has no switch (4
paths, min_disp, a sky mask per view).  And the quality of
tests/test_gpu_settings_fuzz.py's case list, so that a weak list fails here."""
from __future__ import annotations

import numpy as np
import pytest

import ct_cost_recipe
import fill_recipe
import frame_recipe
import min_disp_recipe
import oracle
import paths4_recipe
import pyref
import reproject_recipe
import test_gpu_settings_fuzz as fuzz
import volume_filter_recipe
import volume_recipe
import window_recipe
from frame_recipe import Settings, frame, refusal
from paths4_recipe import assert_bits_equal
from stereo_matching_amd import synthetic

H, W, D = 24, 70, 32


def pair(kind="road", h=H, w=W, d=D):
    return synthetic.stereo_pair(h, w, d, pair_index=7, kind=kind)


def same(got, want, keys):
    for k in keys:
        assert_bits_equal(got[k], want[k], k)


# (P1, P2, uniq, lr_dis): p2 < p1, p1 = 0, p1 = p2, and each ratio and threshold the fuzz draws
MOVED = [(10, 100, 0.7, 1.0), (25, 10, 0.5, 0.0), (0, 100, 1.0, 2.5), (10, 10, 0.7, 1.0), (0, 0, 0.9, 0.5),
         (3, 1, 1.0, 1.0)]


@pytest.mark.parametrize("P1,P2,uniq,lr", MOVED)
@pytest.mark.parametrize("s", [1, 2])
def test_equals_oracle_process(P1, P2, uniq, lr, s):
    left, right = pair("road", H * s, W * s)
    sky = synthetic.sky_mask(H, W)
    st = Settings(D=D, s=s, p1=P1, p2=P2, uniqueness=uniq, lr_max_diff=lr, confidence=True)
    ref = oracle.process(left, right, D, scale=s, sky_l=sky, sky_r=sky, P1=P1, P2=P2, uniq=uniq, lr_dis=lr)
    got = frame(left, right, st, sky, sky)
    same(got, ref, ("disp", "sub", "sub_beta", "lr", "final"))
    assert_bits_equal(got["map"], ref["lr"], "map")
    one = oracle.process(left, right, D, scale=s, P1=P1, P2=P2, uniq=uniq, lr_dis=lr, views=1)
    got = frame(left, right, st.replace(views="left"))
    same(got, one, ("disp", "sub"))
    got = frame(left, right, st.replace(views="right"), sky, sky)
    assert_bits_equal(got["disp"], ref["disp_beta"], "right disp")
    assert_bits_equal(got["sub"], ref["sub_beta"], "right sub")


def test_bm_equals_the_oracle():
    left, right = pair("noise")
    for uniq in (0.5, 0.7, 1.0):
        got = frame(left, right, Settings(solver="bm", D=D, views="left", uniqueness=uniq, post_filter=True))
        d = oracle.bm_process(left, right, D, uniq=uniq)
        assert_bits_equal(got["disp"], d, "bm")
        assert_bits_equal(got["map"], oracle.post_filter(d.astype(np.float32), D, 1), "bm final")


# one setting on, the rest at their defaults: the setting's own recipe
def test_paths4_alone():
    left, right = pair()
    same(frame(left, right, Settings(D=D, paths=4)), paths4_recipe.recipe(left, right, D, 1, None, 4),
         ("disp", "sub", "sub_beta", "lr", "final"))


def test_min_disp_alone():
    left, right = pair(d=2 * D)
    want = min_disp_recipe.recipe(left, right, D, 16)
    same(frame(left, right, Settings(D=D, min_disp=16, confidence=True)), want,
         ("disp", "sub", "sub_beta", "ratio", "ratio_beta", "lr", "final"))


@pytest.mark.parametrize("cost", ["sad", "ssd", "ct"])
@pytest.mark.parametrize("filters", [(False, False), (True, True)])
def test_cost_kind_alone(cost, filters):
    left, right = pair(h=12, w=40)
    if cost == "ct":
        C = ct_cost_recipe.volume(left, right, D)
    else:
        C = window_recipe.volume(left, right, D, cost, window_recipe.DEFAULT)
    want = volume_filter_recipe.recipe(C) if any(filters) else volume_recipe.recipe(C)
    got = frame(left, right, Settings(D=D, cost=cost, volume_filter=filters, confidence=True))
    same(got, want, ("disp", "sub", "sub_beta", "ratio", "ratio_beta", "lr", "final"))


@pytest.mark.parametrize("weighted", [False, True])
def test_window_alone(weighted):
    left, right = pair()
    want = window_recipe.recipe(left, right, D, (5, 5), weighted=weighted)
    same(frame(left, right, Settings(D=D, window=(5, 5), weighted=weighted)), want, ("disp", "sub", "lr", "final"))


def test_confidence_post_filter_fill_reproject_alone():
    left, right = pair()
    ref = oracle.process(left, right, D)
    import confidence_recipe
    S = confidence_recipe.view_volumes(left, right, D, 1, None, 8)
    got = frame(left, right, Settings(D=D, confidence=True))
    assert_bits_equal(got["ratio"], confidence_recipe.ratio_of(S[0]), "ratio")
    assert_bits_equal(got["ratio_beta"], confidence_recipe.ratio_of(S[1]), "ratio_beta")
    assert "ratio" not in frame(left, right, Settings(D=D))
    assert_bits_equal(frame(left, right, Settings(D=D, post_filter=True))["map"], ref["final"], "post_filter")
    q = fuzz.Q
    for post in (False, True):
        base = ref["final"] if post else ref["lr"]
        for mode in ("background", "interpolate"):
            want, mask = fill_recipe.fill(base, D, 0, 1, ref["sub_beta"], mode, 1.0)
            got = frame(left, right, Settings(D=D, post_filter=post, fill=mode, reproject=q))
            assert_bits_equal(got["filled"], want, "filled")
            assert np.array_equal(got["fill_mask"], mask)
            assert_bits_equal(got["xyz"], reproject_recipe.reproject(want, q, D + 1, 1)["xyz"], "xyz")
    got = frame(left, right, Settings(D=D, reproject=q))
    assert_bits_equal(got["depth"], reproject_recipe.reproject(ref["lr"], q, D + 1, 1)["depth"], "depth")


def test_fill_classifies_with_the_handles_threshold():
    left, right = pair("noise")
    ref = oracle.process(left, right, D, lr_dis=0.0)
    want, mask = fill_recipe.fill(ref["lr"], D, 0, 1, ref["sub_beta"], "interpolate", 0.0)
    got = frame(left, right, Settings(D=D, lr_max_diff=0.0, fill="interpolate"))
    assert np.array_equal(got["fill_mask"], mask)
    other = fill_recipe.fill(ref["lr"], D, 0, 1, ref["sub_beta"], "interpolate", 1.0)[1]
    assert not np.array_equal(mask, other)      # (the threshold decides pixels of this frame)


# ------------------------------------------------- pyref: independent loops
SMALL = (12, 40)
P = dict(P1=25, P2=10, uniq=0.5, lr=2.5)


def _pyref_frame(left, right, m, paths, sky_l=None, sky_r=None):
    """A frame from tests/pyref.py's functions alone, constants moved."""
    ctl, ctr = pyref.census(pyref.blur(left)), pyref.census(pyref.blur(right))
    Wd = ctl.shape[1]
    x = np.arange(Wd)
    ctl_s, ctr_s = ctl[:, np.minimum(x + m, Wd - 1)], ctr[:, np.maximum(x - m, 0)]
    subs = []
    for view, (a, b, sky) in enumerate(((ctl, ctr_s, sky_l), (ctl_s, ctr, sky_r))):
        C = pyref.vfilter(pyref.hfilter(pyref.dsi(a, b, D, 1, view, sky), 5), 3)
        L = [pyref.path(C, k, P["P1"], P["P2"])[0] for k in range(paths)]
        S = ((L[0] + L[1]) + L[2]) + L[3]
        if paths == 8:
            S = S + (((L[4] + L[5]) + L[6]) + L[7])
        d = pyref.wta(S, P["uniq"])
        subs.append((d + m, (pyref.subpixel(d, S) + np.float32(m)).astype(np.float32)))
    return subs[0][0], subs[0][1], subs[1][1], pyref.lr_check(subs[0][1], subs[1][1], D + m, 1, P["lr"])


@pytest.mark.parametrize("m,paths,sky", [(0, 4, False), (16, 8, False), (0, 8, True)],
                         ids=["paths4", "min_disp16", "sky_per_view"])
def test_moved_constants_against_pyref(m, paths, sky):
    left, right = pair("road", *SMALL, d=2 * D if m else D)
    sky_l = sky_r = None
    if sky:
        rng = np.random.default_rng(3)
        sky_l, sky_r = fuzz.blob_mask(rng, *SMALL), fuzz.blob_mask(rng, *SMALL)
        assert not np.array_equal(sky_l, sky_r)
    st = Settings(D=D, min_disp=m, paths=paths, p1=P["P1"], p2=P["P2"], uniqueness=P["uniq"], lr_max_diff=P["lr"])
    got = frame(left, right, st, sky_l, sky_r)
    disp, sub, sub_beta, lr = _pyref_frame(left, right, m, paths, sky_l, sky_r)
    assert_bits_equal(got["disp"], disp, "disp")
    assert_bits_equal(got["sub"], sub, "sub")
    assert_bits_equal(got["sub_beta"], sub_beta, "sub_beta")
    assert_bits_equal(got["lr"], lr, "lr")
    if sky:  # (the masks matter: the same frame with them swapped is another frame)
        swapped = frame(left, right, st, sky_r, sky_l)
        assert not np.array_equal(swapped["sub_beta"], got["sub_beta"])


# ------------------------------------------------------------ refusal rules
def test_refusal_rules():
    ok = Settings()
    assert refusal(ok) is None
    assert refusal(ok.replace(s=2, weighted=True)) == "weighted: odd effective window sides"
    assert refusal(ok.replace(s=2, window=(14, 18), weighted=True)) is None
    assert refusal(ok.replace(fill="interpolate", views="left")) == "interpolate: two views"
    bm = ok.replace(solver="bm", views="left")
    assert refusal(bm) is None
    assert refusal(bm.replace(min_disp=16)) == "bm: no min_disp"
    assert refusal(bm.replace(cost="sad")) == "bm: no cost kind"
    assert refusal(bm.replace(fill="interpolate")) == "bm: no interpolate"
    assert refusal(ok.replace(cost="ct", sky_detect=True)) == "sky_detect: no cost kind"
    assert refusal(ok.replace(cost="ct"), sky=True) == "sky masks: no cost kind"
    assert refusal(ok.replace(s=2, window=(18, 18))) == "window: 64 bits"
    assert refusal(ok.replace(s=2, window=(20, 18))) == "window: 1..9"
    assert refusal(ok.replace(s=2, window=(3, 3))) == "window: centre"
    assert refusal(ok.replace(s=2, min_disp=3)).startswith("min_disp")
    # every rule refusal() can return has its refused example on the GPU: a setter's (REFUSALS), or
    # sgm_create's (test_create_refusals); two are not the library's: a value no setter has a word
    # for, and BM's one view, which its constructor fixes
    import inspect
    import re
    rules = set(re.findall(r'return "([^"]+)"', inspect.getsource(refusal)))
    rules.discard("window: ")
    rules |= {"window: " + w for w in ("1..9", "centre", "64 bits")}      # (weighted_recipe.refusal's)
    assert "window: scale" not in rules
    create = {r for r in rules if r.startswith("create: ")}
    assert len(create) == 4 == len(fuzz.CREATE_REFUSALS)
    assert rules - create - {"unknown value", "bm: one view, the left"} == set(fuzz.REFUSALS)


# ------------------------------------------------- the quality of the cases
def test_case_list_quality():
    cases = fuzz.CASES
    # (the issue aimed at 40 to 56; every accepted pair, mixed maps and two thirds of the cases under
    # each forced schedule together take more: small frames, so the GPU file still runs in seconds)
    assert len(cases) == 206
    assert all(refusal(fuzz.settings(a), a["sky"] != "none") is None for a in cases)
    for name, values in fuzz.AXES.items():
        for v in values:
            assert sum(a[name] == v for a in cases) >= 2, (name, v)
    two = [a for a in cases if a["views"] == "two"]
    assert 3 * sum(a["sky"] == "differ" for a in two) >= len(two)
    assert 4 * sum(a["p2"] < a["p1"] or a["p1"] == 0 for a in cases) >= len(cases)
    assert any(a["p1"] == a["p2"] for a in cases)
    for cost in fuzz.AXES["cost"]:
        assert any(a["cost"] == cost and a["uniqueness"] <= 0.5 for a in cases), cost
        assert any(a["cost"] == cost and a["uniqueness"] == 1.0 for a in cases), cost
    sgm = [a for a in cases if fuzz.sgm_solver(a)]
    for name in fuzz.SCHEDULES:
        assert 3 * sum(fuzz.keeps(a, name) for a in sgm) >= 2 * len(sgm), name
    seen = set().union(*(fuzz.pairs_of(a) for a in cases))
    missing = sorted(fuzz.accepted_pairs() - seen, key=str)
    assert not missing, missing


@pytest.mark.parametrize("k", range(len(fuzz.CASES)), ids=fuzz.IDS)
def test_case_compares_a_map_with_valid_and_invalid_pixels(k):
    """The frame's map, as post_filter leaves it where it is set, holds valid and invalid pixels;
    a filled case compares that map filled, so its mask holds measured and inferred pixels."""
    a, want = fuzz.CASES[k], fuzz.expected(k)
    valid = fill_recipe.valid(want["map"].astype(np.float32), a["D"], a["min_disp"])
    assert valid.any() and not valid.all(), float(valid.mean())
    if a["fill"] != "off":
        assert (want["fill_mask"] == 0).any() and (want["fill_mask"] != 0).any()
