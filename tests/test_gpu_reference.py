"""GPU parity with the REFERENCE's own binaries, not through the oracle.

Every expected value here was written by hilbertw/stereo_matching's unmodified
src/{Solver,SGM,cost,BM}.cpp (tests/golden/ref_*.npz, ref_maps.npz,
ref_hashes.json; tests/golden/make_ref_golden.py).  The library is compared
with them as raw bits: whole frames (raw, LR-checked and post-filtered maps,
and the right view's raw and sub-pixel maps from a one-view right handle),
the stage entry points (census words, cost volumes, the eight path volumes,
aggregation + WTA + sub-pixel of both views, the LR check), BM, post_filter()
and colormap() on arbitrary maps, and one frame under SGM_SLANT=1 and
SGM_BAND_ROWS=16.  Volumes are checked by the D-vectors of the sampled pixels
(a failure names the pixel) and by sha256.  A stage is fed the reference's
census words, or the library's own volume once its sha256 has matched the
reference's.  Nothing here reads anything but tests/golden/.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from support import bits
from stereo_matching_amd import BM, SGM

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLDEN, "make_ref_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "ref_hashes.json")) as _fh:
    HASHES = json.load(_fh)["volumes"]
NAMES = list(gen.CASES)


def same_map(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype == np.float32:
        assert got.dtype == np.float32, (what, got.dtype)
        g, w = bits(got), bits(want)
    else:
        g, w = got.astype(np.int64), want.astype(np.int64)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)}/{g.size} differ, first at {tuple(bad[0])}: "
                           f"got {got[tuple(bad[0])]!r}, reference {want[tuple(bad[0])]!r}")


def same_volume(got, fx, name, key):
    got = np.ascontiguousarray(got, np.float32)
    H, W, D = got.shape
    idx, want = fx["sample_idx"], fx["smp_" + key]
    g = got.reshape(H * W, D)[idx]
    bad = np.argwhere(bits(g) != bits(want))
    if bad.size:
        p, d = bad[0]
        raise AssertionError(f"{name} {key}: {len(bad)} sampled entries differ, first at pixel "
                             f"({idx[p] // W}, {idx[p] % W}) d={d}: got {g[p, d]!r}, reference {want[p, d]!r}")
    assert hashlib.sha256(got.tobytes()).hexdigest() == HASHES[name][key], \
        f"{name} {key}: the sampled vectors agree but the volume's sha256 does not"


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    name = request.param
    fx = gen.load_case(name)
    m = fx["meta"]
    left, right, sky_l, sky_r = gen.inputs(m)
    sgm = SGM(m["h"], m["w"], m["scale"], m["D"], blur=m["blur"])
    c = dict(name=name, fx=fx, m=m, left=left, right=right, sky_l=sky_l, sky_r=sky_r, sgm=sgm)
    yield c
    sgm.close()


def _cost(case, view):
    """The library's filtered cost volume of one view, from the reference's
    census words; usable as the next stage's input once it equals the
    reference's (sha256)."""
    key = "vf_b" if view else "vf"
    if key not in case:
        fx = case["fx"]
        sky = case["sky_r"] if view else case["sky_l"]
        cost = case["sgm"].stage_cost(fx["ct_l"], fx["ct_r"], view, sky, filters=3)
        same_volume(cost, fx, case["name"], key)
        case[key] = cost
    return case[key]


def test_census(case):
    fx = case["fx"]
    same_map(case["sgm"].stage_census(case["left"]), fx["ct_l"], "census, left")
    same_map(case["sgm"].stage_census(case["right"]), fx["ct_r"], "census, right")


def test_cost_volumes(case):
    fx, sgm = case["fx"], case["sgm"]
    for view, sfx, sky in ((0, "", case["sky_l"]), (1, "_b", case["sky_r"])):
        same_volume(sgm.stage_cost(fx["ct_l"], fx["ct_r"], view, sky, filters=0), fx, case["name"], "dsi" + sfx)
        same_volume(sgm.stage_cost(fx["ct_l"], fx["ct_r"], view, sky, filters=1), fx, case["name"], "hf" + sfx)
        _cost(case, view)


@pytest.mark.parametrize("view", [0, 1], ids=["left", "right"])
def test_paths(case, view):
    cost = _cost(case, view)
    for k in range(8):
        L, _ = case["sgm"].stage_path(k, cost)
        same_volume(L, case["fx"], case["name"], f"L{k + 1}" + ("_b" if view else ""))


@pytest.mark.parametrize("view", [0, 1], ids=["left", "right"])
def test_aggregate_wta_subpixel(case, view):
    """stage_aggregate on the right view's cost gives the right view's raw map."""
    sfx = "_b" if view else ""
    d, f = case["sgm"].stage_aggregate(_cost(case, view))
    same_map(d, case["fx"]["disp" + sfx], "WTA" + sfx)
    same_map(f, case["fx"]["sub" + sfx], "sub-pixel" + sfx)


def test_lr_check(case):
    fx = case["fx"]
    same_map(case["sgm"].stage_lr(fx["sub"], fx["sub_b"]), fx["lr"], "LR check")


def _frame(m, fx, left, right, sky_l, sky_r, sgm=None, what=""):
    """A processed frame against the reference: the two-view handle's raw, LR
    and post-filtered maps, and the right view's raw and sub-pixel maps from
    a one-view handle (views=1, view="right": the frame path's right view,
    not the stage entry)."""
    own = sgm is None
    if own:
        sgm = SGM(m["h"], m["w"], m["scale"], m["D"], blur=m["blur"])
    try:
        sgm.process(left, right, sky_l, sky_r)
        same_map(sgm.get_raw_disp(), fx["disp"], "get_raw_disp" + what)
        same_map(sgm.get_lr_disp(), fx["lr"], "get_lr_disp" + what)
        same_map(sgm.get_disp(), fx["final"], "get_disp" + what)
    finally:
        if own:
            sgm.close()
    with SGM(m["h"], m["w"], m["scale"], m["D"], blur=m["blur"], views=1, view="right") as rgt:
        rgt.process(left, right, sky_l, sky_r)
        same_map(rgt.get_raw_disp(), fx["disp_b"], "right view's raw map" + what)
        same_map(rgt.get_lr_disp(), fx["sub_b"], "right view's sub-pixel map" + what)
    with SGM(m["h"], m["w"], m["scale"], m["D"], blur=m["blur"], views=1) as lft:
        lft.process(left, right, sky_l, sky_r)
        same_map(lft.get_raw_disp(), fx["disp"], "one-view left raw map" + what)
        same_map(lft.get_lr_disp(), fx["sub"], "left view's sub-pixel map" + what)


def test_full_process(case):
    _frame(case["m"], case["fx"], case["left"], case["right"], case["sky_l"], case["sky_r"],
           sgm=case["sgm"])


def test_bm(case):
    m = case["m"]
    with BM(m["h"], m["w"], m["scale"], m["D"], blur=m["blur"]) as bm:
        bm.process(case["left"], case["right"], case["sky_l"], case["sky_r"])
        same_map(bm.get_raw_disp(), case["fx"]["bm_disp"], "BM get_raw_disp")


@pytest.mark.parametrize("env", [{"SGM_SLANT": "1"}, {"SGM_BAND_ROWS": "16"}], ids=["slant", "bands16"])
def test_schedules(env, monkeypatch):
    name = "road_sky_48x170_D64"
    fx = gen.load_case(name)
    m = fx["meta"]
    left, right, sky_l, sky_r = gen.inputs(m)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _frame(m, fx, left, right, sky_l, sky_r, what=f" {env}")


MAP_KEYS = list(gen.map_inputs())


@pytest.fixture(scope="module")
def ref_maps():
    with np.load(os.path.join(GOLDEN, "ref_maps.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("key", MAP_KEYS)
def test_post_filter_and_colormap_on_maps(ref_maps, key):
    f, D, s = gen.map_inputs()[key]
    H, W = f.shape
    with SGM(H * s, W * s, s, D) as sgm:
        got = sgm.post_filter(f) if key.startswith("pf_") else sgm.colormap(f)
    same_map(got, ref_maps[key], key)
