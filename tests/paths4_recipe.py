"""Expected maps of the 4-path aggregation mode (params.paths = 4), composed
from the oracle's stage functions.

The oracle has no 4-path switch (the reference's is a compile-time constant,
USE_8_PATH in inc/SGM.h:7), so the expectation follows SGM::process stage by
stage (SGM.cpp:32-826) with S = ((L1+L2)+L3)+L4 (SGM.cpp:387-388 with the
switch off) in numpy float32, in exactly that association order.  With
paths=8 the same recipe adds (((L5+L6)+L7)+L8) (SGM.cpp:389-390) and must
reproduce oracle.process bit for bit, which tests/test_paths4_cpu.py checks.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
from stereo_matching_amd import synthetic

# (h, w, D, scale, kind, sky)
SHAPES = [
    (3, 5, 32, 1, "noise", False),
    (19, 23, 64, 1, "road", False),
    (37, 75, 32, 1, "road", False),
    (48, 150, 64, 1, "noise", True),
    (50, 141, 128, 1, "road", True),
    (33, 270, 256, 1, "road", False),
    (96, 300, 64, 2, "road", True),
    (8, 17, 64, 1, "road", False),
    (9, 31, 32, 1, "road", False),
    (40, 16, 128, 1, "road", False),
]
IDS = [f"{h}x{w}_D{D}_s{s}_{k}{'_sky' if sk else ''}" for h, w, D, s, k, sk in SHAPES]


def make_inputs(h, w, D, s, kind, sky):
    left, right = synthetic.stereo_pair(h, w, D, pair_index=3, kind=kind)
    mask = synthetic.sky_mask(h // s, w // s) if sky else None
    return left, right, mask


def census(img, s):
    return oracle.census(oracle.blur(np.ascontiguousarray(img[::s, ::s])), s)


def cost_volume(ctl, ctr, D, s, view, sky):
    c = oracle.dsi(ctl, ctr, D, s, view, sky)
    return oracle.vfilter(oracle.hfilter(c, 5 // s), 3 // s)


def aggregate(cost, paths, P1=10, P2=100):
    """S of one view, float32, the reference's association order."""
    L = [oracle.path(cost, k, P1, P2)[0] for k in range(paths)]
    S = ((L[0] + L[1]) + L[2]) + L[3]
    if paths == 8:
        S = S + (((L[4] + L[5]) + L[6]) + L[7])
    assert S.dtype == np.float32
    return S


def view_maps(cost, paths, P1=10, P2=100, uniq=0.7):
    S = aggregate(cost, paths, P1, P2)
    disp = oracle.wta(S, uniq)
    return disp, oracle.subpixel(disp, S)


def masks(sky, sky_l=None, sky_r=None):
    """(left view's mask, right view's): `sky` serves both unless a view's own is given."""
    return (sky if sky_l is None else sky_l), (sky if sky_r is None else sky_r)


def recipe(left, right, D, s=1, sky=None, paths=4, P1=10, P2=100, uniq=0.7, lr_dis=1.0, sky_l=None, sky_r=None):
    """The maps of oracle.process (same keys), for 4 or 8 paths; the sky mask
    `sky` serves both views unless sky_l / sky_r give a view its own."""
    ctl, ctr = census(left, s), census(right, s)
    sky_l, sky_r = masks(sky, sky_l, sky_r)
    out = {}
    out["disp"], out["sub"] = view_maps(cost_volume(ctl, ctr, D, s, 0, sky_l), paths, P1, P2, uniq)
    out["disp_beta"], out["sub_beta"] = view_maps(cost_volume(ctl, ctr, D, s, 1, sky_r), paths, P1, P2, uniq)
    out["lr"] = oracle.lr_check(out["sub"], out["sub_beta"], D, s, lr_dis)
    out["final"] = oracle.post_filter(out["lr"], D, s)
    return out


@functools.lru_cache(maxsize=None)
def expected(shape, paths=4):
    """recipe() of a SHAPES entry, computed once per session; read-only."""
    h, w, D, s, kind, sky = shape
    left, right, mask = make_inputs(*shape)
    out = recipe(left, right, D, s, mask, paths)
    for a in out.values():
        a.setflags(write=False)
    return out


def bits(a):
    """An array as what the bit-exact comparisons compare: floats as their float32 bit patterns,
    everything else as int64 (a meaning of its own: neither support.bits nor support.f32_bits)."""
    a = np.ascontiguousarray(a)
    return a.astype(np.float32, copy=False).view(np.uint32) if a.dtype.kind == "f" else a.astype(np.int64)


def assert_bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float32 or want.dtype == np.float32:
        g, w = bits(got.astype(np.float32)), bits(want.astype(np.float32))
    else:
        g, w = got.astype(np.int64), want.astype(np.int64)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, (f"{what}: {bad.size}/{g.size} mismatches, first at flat index "
                           f"{bad[0]}: got {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}")
