"""Expected maps of a volume frame with the cost filters on
(sgm_set_volume_filter), composed from the oracle's stage
functions: volume_recipe's right-view derivation from the RAW left volume,
oracle.hfilter(5 // s) and oracle.vfilter(3 // s) on each view on its own (as
SGM::process filters each DSI it built, SGM.cpp:66-72), then the rest of
volume_recipe.  oracle.hfilter / oracle.vfilter are pinned to the reference's
own binaries by tests/test_reference_parity.py.  Also the test volumes:
non-integer fp32 of mixed magnitudes, where a reordered sum or a fused
add-subtract changes bits, and one whose recursion undershoots below zero.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
import volume_recipe as vr

H_BIT, V_BIT = 1, 2


def filtered(C, s=1, filters=H_BIT | V_BIT):
    """One view's volume through the filters `filters` names, horizontal first."""
    C = np.ascontiguousarray(C, np.float32)
    if filters & H_BIT:
        C = oracle.hfilter(C, 5 // s)
    if filters & V_BIT:
        C = oracle.vfilter(C, 3 // s)
    return C


def recipe(C, m=0, s=1, paths=8, filters=H_BIT | V_BIT, P1=10, P2=100, uniq=0.7, lr_dis=1.0):
    """volume_recipe.recipe's maps of the raw left volume C with each view filtered on its own:
    "disp", "sub", "ratio", "sub_beta", "ratio_beta", "lr", "final"."""
    H, W, D = C.shape
    out = {}
    out["disp"], out["sub"], out["ratio"] = vr.view_maps(filtered(C, s, filters), m, paths, P1, P2, uniq)
    _, out["sub_beta"], out["ratio_beta"] = vr.view_maps(filtered(vr.derive_right(C, m, s), s, filters), m, paths,
                                                         P1, P2, uniq)
    out["lr"] = oracle.lr_check(out["sub"], out["sub_beta"], D + m, s, lr_dis)
    out["final"] = oracle.post_filter(out["lr"], D + m, s)
    return out


def caller_side(C, m=0, s=1, paths=8, filters=H_BIT | V_BIT):
    """What a caller gets who filters the left volume and hands it to an unfiltering two-view
    frame: the right view is derived from the FILTERED left volume.  Not the library's order."""
    return vr.recipe(filtered(C, s, filters), m, s, paths)


def mixed_volume(h, w, D, seed=3):
    """Uniform in [0, 1000) with about 1% of the elements multiplied by 1000."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1000.0, (h, w, D))
    c = np.where(rng.uniform(size=c.shape) < 0.01, c * 1000.0, c)
    return np.ascontiguousarray(c.astype(np.float32))


def undershoot_volume(h, w, D, seed=5):
    """The mixed volume with a block of columns at 999999 beside zeros: after the drop the
    recursion's sum goes below zero."""
    c = mixed_volume(h, w, D, seed)
    a = w // 3
    c[:, a:a + 4, :] = 999999.0
    c[:, a + 4:a + 4 + max(6, w // 4), :] = 0.0
    return c


def surface_volume(h, w, D, seed=7):
    """volume_recipe's planted surface without its binary16 rounding, plus a little fp32 noise:
    maps with structure for the frame tests (the LR check keeps pixels), non-integer costs."""
    rng = np.random.default_rng(seed)
    c = vr.noise_volume(h, w, D, seed).astype(np.float64) + rng.uniform(0.0, 1.0, (h, w, D))
    return np.ascontiguousarray(c.astype(np.float32))


@functools.lru_cache(maxsize=None)
def frame_volume(h, w, D, f16=False):
    """The frame tests' left volume (f16: rounded to binary16, what an fp16 source holds); read-only."""
    c = surface_volume(h, w, D)
    if f16:
        c = np.ascontiguousarray(c.astype(np.float16).astype(np.float32))
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(h, w, D, m=0, s=1, paths=8, f16=False, filters=H_BIT | V_BIT):
    """recipe() of frame_volume, computed once per session; read-only."""
    out = recipe(frame_volume(h, w, D, f16), m, s, paths, filters)
    for a in out.values():
        a.setflags(write=False)
    return out


bits = vr.bits
