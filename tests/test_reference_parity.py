"""The CPU oracle against what the REFERENCE's own code computed.

tests/golden/ref_*.npz, ref_maps.npz and ref_hashes.json were written by
hilbertw/stereo_matching's unmodified src/{Solver,SGM,cost,BM}.cpp, run
through oracle/ref/ref_driver.cpp (tests/golden/make_ref_golden.py).  Every
stage of oracle/sgm_oracle.c (and pyref.colormap) is compared with them as raw
bits: H x W maps in full, volumes by sha256 and by the D-vectors of up to 64
sampled pixels, so that a failure names the pixel.  Each stage is fed the
oracle's own output of the stage before it, so the first stage that differs
is the one that fails first.

These tests read tests/golden/ only.  The last one regenerates every fixture
when oracle/_ref/'s driver and the reference are there, and is skipped
otherwise.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import oracle
import pyref
from support import bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLDEN, "make_ref_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "ref_hashes.json")) as _fh:
    HASHES = json.load(_fh)
NAMES = list(gen.CASES)


@pytest.fixture(scope="module", autouse=True)
def few_threads():
    """The frames are tiny: on a many-core host the oracle's OpenMP regions
    cost more in thread start-up than in work."""
    before = oracle.max_threads()
    oracle.set_threads(min(before, 4))
    yield
    oracle.set_threads(before)


def same_map(got, want, what):
    """Integer maps by value (the reference's uchar against the oracle's
    int32), float maps as uint32."""
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
    """A volume against its sampled D-vectors (says where) and its sha256."""
    got = np.ascontiguousarray(got, np.float32)
    H, W, D = got.shape
    idx, want = fx["sample_idx"], fx["smp_" + key]
    g = got.reshape(H * W, D)[idx]
    bad = np.argwhere(bits(g) != bits(want))
    if bad.size:
        p, d = bad[0]
        raise AssertionError(f"{name} {key}: {len(bad)} sampled entries differ, first at pixel "
                             f"({idx[p] // W}, {idx[p] % W}) d={d}: got {g[p, d]!r}, reference {want[p, d]!r}")
    assert hashlib.sha256(got.tobytes()).hexdigest() == HASHES["volumes"][name][key], \
        f"{name} {key}: the sampled vectors agree but the volume's sha256 does not"


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    """The fixture, the regenerated inputs and the oracle's chain of stages."""
    name = request.param
    fx = gen.load_case(name)
    m = fx["meta"]
    left, right, sky_l, sky_r = gen.inputs(m)
    s, D = m["scale"], m["D"]
    H, W = m["h"] // s, m["w"] // s
    wl = np.ascontiguousarray(left[: H * s: s, : W * s: s])
    wr = np.ascontiguousarray(right[: H * s: s, : W * s: s])
    c = dict(name=name, fx=fx, m=m, left=left, right=right, sky_l=sky_l, sky_r=sky_r, wl=wl, wr=wr)
    bl, br = (oracle.blur(wl), oracle.blur(wr)) if m["blur"] else (wl, wr)
    c["ct_l"], c["ct_r"] = oracle.census(bl, s), oracle.census(br, s)
    for view, sfx, sky in ((0, "", sky_l), (1, "_b", sky_r)):
        c["dsi" + sfx] = oracle.dsi(c["ct_l"], c["ct_r"], D, s, view, sky)
        c["hf" + sfx] = oracle.hfilter(c["dsi" + sfx], 5 // s)
        c["vf" + sfx] = oracle.vfilter(c["hf" + sfx], 3 // s)
        Ls = [oracle.path(c["vf" + sfx], k)[0] for k in range(8)]
        for k in range(8):
            c[f"L{k + 1}{sfx}"] = Ls[k]
        c["S" + sfx] = oracle.aggregate(Ls)
        c["disp" + sfx] = oracle.wta(c["S" + sfx])
        c["sub" + sfx] = oracle.subpixel(c["disp" + sfx], c["S" + sfx])
    c["lr"] = oracle.lr_check(c["sub"], c["sub_b"], D, s)
    c["final"] = oracle.post_filter(c["lr"], D, s)
    return c


def test_working_images_and_census(case):
    fx = case["fx"]
    same_map(case["wl"], fx["img_l"], "working image, left")
    same_map(case["wr"], fx["img_r"], "working image, right")
    assert fx["ct_l"].dtype == np.uint64
    same_map(case["ct_l"], fx["ct_l"], "census, left")
    same_map(case["ct_r"], fx["ct_r"], "census, right")


@pytest.mark.parametrize("key", ["dsi", "hf", "vf", "dsi_b", "hf_b", "vf_b"])
def test_cost_volume(case, key):
    same_volume(case[key], case["fx"], case["name"], key)


@pytest.mark.parametrize("view", ["", "_b"], ids=["left", "right"])
@pytest.mark.parametrize("k", range(1, 9))
def test_path(case, k, view):
    same_volume(case[f"L{k}{view}"], case["fx"], case["name"], f"L{k}{view}")


@pytest.mark.parametrize("view", ["", "_b"], ids=["left", "right"])
def test_aggregate_wta_subpixel(case, view):
    fx = case["fx"]
    same_volume(case["S" + view], fx, case["name"], "S" + view)
    same_map(case["disp" + view], fx["disp" + view], "WTA " + (view or "left"))
    same_map(case["sub" + view], fx["sub" + view], "sub-pixel " + (view or "left"))


def test_subpixel_on_drawn_disparities(case):
    """compute_subpixel() on disparities that are not the minimum: quotients
    of either sign, 0/0 and x/0 included (Solver.cpp:586-594)."""
    m, fx = case["m"], case["fx"]
    H, W = fx["disp"].shape
    din = gen.subpixel_input(case["name"], H, W, m["D"]).astype(np.int32)
    same_map(oracle.subpixel(din, case["S_b"]), fx["subpixel"], "compute_subpixel")


def test_lr_check_and_post_filter(case):
    fx = case["fx"]
    same_map(case["lr"], fx["lr"], "LR check")
    same_map(case["final"], fx["final"], "post_filter")
    # each stage on the reference's own input as well, so that one stage's
    # fault cannot hide the next one's
    m = case["m"]
    same_map(oracle.lr_check(fx["sub"], fx["sub_b"], m["D"], m["scale"]), fx["lr"], "LR check (ref input)")
    same_map(oracle.post_filter(fx["lr"], m["D"], m["scale"]), fx["final"], "post_filter (ref input)")


@pytest.mark.parametrize("schedule", ["parity", "lean", "refplace"])
def test_process(case, schedule):
    m, fx = case["m"], case["fx"]
    out = oracle.process(case["left"], case["right"], m["D"], m["scale"], case["sky_l"], case["sky_r"],
                         blur=m["blur"], schedule=schedule)
    for key, ref in (("disp", "disp"), ("disp_beta", "disp_b"), ("sub", "sub"), ("sub_beta", "sub_b"),
                     ("lr", "lr"), ("final", "final")):
        same_map(out[key], fx[ref], f"process[{schedule}] {key}")


def test_bm_process(case):
    m, fx = case["m"], case["fx"]
    got = oracle.bm_process(case["left"], case["right"], m["D"], m["scale"], sky=case["sky_l"], blur=m["blur"])
    same_map(got, fx["bm_disp"], "BM::process disp")
    if m["scale"] > 1:   # BM's own decimation: rows not strided (BM.cpp:23-24)
        s = m["scale"]
        H, W = fx["disp"].shape
        for img, key in ((case["left"], "bm_ct_l"), (case["right"], "bm_ct_r")):
            w = np.ascontiguousarray(img[:H, : W * s: s])
            same_map(oracle.census(oracle.blur(w) if m["blur"] else w, s), fx[key], key)


MAP_KEYS = list(gen.map_inputs())


@pytest.fixture(scope="module")
def ref_maps():
    with np.load(os.path.join(GOLDEN, "ref_maps.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("key", MAP_KEYS)
def test_post_filter_and_colormap_on_maps(ref_maps, key):
    f, D, s = gen.map_inputs()[key]
    if key.startswith("pf_"):
        same_map(oracle.post_filter(f, D, s), ref_maps[key], key)
    else:
        same_map(pyref.colormap(f, D), ref_maps[key], key)


def test_fixture_set_conditions():
    """The conditions the issue of record sets on the fixture set, re-derived
    from the fixtures themselves (and compared with the recorded statistics).
    The one field not re-derived here is inf_subpixel: it needs the summed
    volume, which the fixtures hold only as samples, so the recorded count is
    passed through; the next test re-derives it from the oracle's S_b."""
    stats = {}
    for name in NAMES:
        fx = gen.load_case(name)
        st = gen.stats(dict(fx["meta"], inf_subpixel=HASHES["stats"][name]["inf_subpixel"]), fx)
        assert st == HASHES["stats"][name], name
        stats[name] = st
    gen.check_set(stats)
    sizes = [os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("ref_")]
    assert max(sizes) < 315188 and sum(sizes) < 1.5e6


def test_inf_subpixel_pixels_are_in_the_fixtures():
    """The recorded +inf -> D-1 count, re-derived from the oracle's S_b (which
    test_aggregate_wta_subpixel pins to the reference's by hash)."""
    total = 0
    for name in NAMES:
        if HASHES["stats"][name]["inf_subpixel"] == 0:
            continue
        fx = gen.load_case(name)
        m = fx["meta"]
        left, right, sl, sr = gen.inputs(m)
        D, s = m["D"], m["scale"]
        H, W = fx["disp"].shape
        wl, wr = left[: H * s: s, : W * s: s], right[: H * s: s, : W * s: s]
        ctl, ctr = (oracle.census(oracle.blur(w) if m["blur"] else np.ascontiguousarray(w), s) for w in (wl, wr))
        cost = oracle.vfilter(oracle.hfilter(oracle.dsi(ctl, ctr, D, s, 1, sr), 5 // s), 3 // s)
        S = oracle.aggregate([oracle.path(cost, k)[0] for k in range(8)])
        din = gen.subpixel_input(name, H, W, D)
        d = np.clip(din.astype(np.int64), 1, D - 2)
        c0, cm, cp = (np.take_along_axis(S, (d + o)[..., None], 2)[..., 0] for o in (0, -1, 1))
        with np.errstate(all="ignore"):
            q = (cm - cp) / (np.float32(2) * (cm + cp - np.float32(2) * c0))
        n = int(np.sum(np.isposinf(q) & (din >= 1) & (din <= D - 2) & (fx["subpixel"] == D - 1)))
        assert n == HASHES["stats"][name]["inf_subpixel"], name
        total += n
    assert total > 0


@pytest.mark.skipif(oracle.ref_driver() is None, reason="no reference build in oracle/_ref/")
def test_regenerated_fixtures_equal_committed():
    """Run the reference again: every array equals the committed fixture, and
    every stage before post_filter is the same with 1 and 8 OpenMP threads
    (speckle_filter_new races; everything before it is deterministic)."""
    for name in NAMES:
        fx = gen.load_case(name)
        meta, maps, vols = gen.run_case(oracle, name, threads=1)
        meta.pop("inf_subpixel")
        assert meta == fx["meta"], name
        H, W = maps["disp"].shape
        idx = gen.sample_pixels(name, H, W)
        assert np.array_equal(idx, fx["sample_idx"])
        for k, v in maps.items():
            assert v.dtype == fx[k].dtype and np.array_equal(bits(v), bits(fx[k])), (name, k)
        for k, v in vols.items():
            assert gen.sha(v) == HASHES["volumes"][name][k], (name, k)
            assert np.array_equal(bits(v.reshape(H * W, -1)[idx]), bits(fx["smp_" + k])), (name, k)
        _, maps8, vols8 = gen.run_case(oracle, name, threads=8)
        for k, v in maps8.items():
            if k != "final":
                assert np.array_equal(bits(v), bits(maps[k])), (name, k, "1 and 8 threads differ")
        for k, v in vols8.items():
            assert gen.sha(v) == HASHES["volumes"][name][k], (name, k, "1 and 8 threads differ")
    with np.load(os.path.join(GOLDEN, "ref_maps.npz")) as z:
        for k, v in gen.run_maps(oracle).items():
            assert np.array_equal(bits(v), bits(z[k])), k
