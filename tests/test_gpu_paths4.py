"""The 4-path aggregation mode (params.paths = 4: the reference's USE_8_PATH
off, inc/SGM.h:7; S = ((L1+L2)+L3)+L4, SGM.cpp:387-388) on the GPU, bit for
bit against the recipe composed from the oracle's stage functions
(tests/paths4_recipe.py; tests/test_paths4_cpu.py pins the recipe itself).

Shapes: the minimum size, W < 16 and H < 8 (a single partial segment), W mod
16 in {0, 1, 7, 11, 13, 14, 15}, H mod 8 in {0, 1, 2, 3, 5}, every D, scale 2,
sky masks."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import paths4_recipe as p4
from stereo_matching_amd import SGM, SGMError, _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 8-path schedules' launch classes a 4-path frame must not report
EIGHT_PATH_CLASSES = ("stage_a", "stage_b", "stage_a_d", "stage_b_d2", "sweep_L8_acc", "slant_down",
                      "slant_up")
# the 4-path schedule's one choice by size, forced either way (sgm_create.hip
# sgm_create): 0 = the one-launch H pair, 1 = forward + two-wave
# backward launches
SWITCHES = ("SGM_P4_HPAIR",)


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _two_views(shape, env=None, **kw):
    """(raw, lr) of a two-view 4-path frame."""
    h, w, D, s, kind, sky = shape
    left, right, mask = p4.make_inputs(*shape)
    with _Env(env or {}):
        with SGM(h, w, s, D, paths=4, **kw) as sgm:
            sgm.process(left, right, mask, mask)
            return sgm.get_raw_disp().copy(), sgm.get_lr_disp().copy(), sgm.device_bytes


@pytest.mark.parametrize("shape", p4.SHAPES, ids=p4.IDS)
def test_two_views(shape):
    h, w, D, s, kind, sky = shape
    want = p4.expected(shape)
    raw, lr, _ = _two_views(shape)
    p4.assert_bits_equal(raw, want["disp"], "raw WTA map")
    p4.assert_bits_equal(lr, want["lr"], "LR map")
    left, right, mask = p4.make_inputs(*shape)
    with SGM(h, w, s, D, paths=4, post_filter=True) as sgm:
        sgm.process(left, right, mask, mask)
        p4.assert_bits_equal(sgm.get_disp(), want["final"], "get_disp()")


@pytest.mark.parametrize("shape", p4.SHAPES, ids=p4.IDS)
def test_one_view(shape):
    h, w, D, s, kind, sky = shape
    want = p4.expected(shape)
    left, right, mask = p4.make_inputs(*shape)
    with SGM(h, w, s, D, paths=4, views=1) as sgm:
        sgm.process(left, right, mask, mask)
        p4.assert_bits_equal(sgm.get_raw_disp(), want["disp"], "left raw map")
        p4.assert_bits_equal(sgm.get_lr_disp(), want["sub"], "left sub-pixel map")
    with SGM(h, w, s, D, paths=4, views=1, view="right") as sgm:
        sgm.process(left, right, mask, mask)
        p4.assert_bits_equal(sgm.get_raw_disp(), want["disp_beta"], "right raw map")
        p4.assert_bits_equal(sgm.get_lr_disp(), want["sub_beta"], "right sub-pixel map")


DEVICE = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
dev = torch.device("cuda", 0)
torch.cuda.init()                      # torch's runtime first, as in bench.py
import paths4_recipe as p4
from stereo_matching_amd import SGM
shape = p4.SHAPES[4]
h, w, D, s, kind, sky = shape
left, right, mask = p4.make_inputs(*shape)
want = p4.expected(shape)
pitch, spitch, opitch = w + 64, w + 32, w + 16
L = torch.full((h, pitch), 5, dtype=torch.uint8, device=dev)
R = torch.full((h, pitch), 250, dtype=torch.uint8, device=dev)
L[:, :w] = torch.from_numpy(left).to(dev)
R[:, :w] = torch.from_numpy(right).to(dev)
S = torch.full((2, h, spitch), 255, dtype=torch.uint8, device=dev)
S[:, :, :w] = torch.from_numpy(mask).to(dev)
for views, key in ((2, "lr"), (1, "sub")):
    out = torch.full((h, opitch), -9.0, dtype=torch.float32, device=dev)
    with SGM(h, w, 1, D, device=0, paths=4, views=views) as sgm:
        sgm.process_device(L.data_ptr(), R.data_ptr(), out.data_ptr(), pitch=pitch,
                           d_sky_l=S[0].data_ptr(), d_sky_r=S[1].data_ptr(), sky_pitch=spitch,
                           out_pitch=opitch)
        sgm.check()
    got = out.cpu().numpy()
    p4.assert_bits_equal(got[:, :w], want[key], key)
    assert (got[:, w:] == -9.0).all(), "output padding written"
print("paths4 device ok")
"""


def test_process_device_pitched_no_raw_map():
    r = subprocess.run([sys.executable, "-c", DEVICE, ROOT], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "paths4 device ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("shape", [p4.SHAPES[3], p4.SHAPES[5]], ids=[p4.IDS[3], p4.IDS[5]])
def test_stage_aggregate(shape):
    h, w, D, s, kind, sky = shape
    left, right, mask = p4.make_inputs(*shape)
    cost = p4.cost_volume(p4.census(left, s), p4.census(right, s), D, s, 0, mask)
    want = p4.expected(shape)
    with SGM(h, w, s, D, paths=4) as sgm:
        d, f = sgm.stage_aggregate(cost)
        p4.assert_bits_equal(d, want["disp"], "stage_aggregate disp")
        p4.assert_bits_equal(f, want["sub"], "stage_aggregate sub")


def test_stage_path():
    shape = p4.SHAPES[2]
    h, w, D, s, kind, sky = shape
    left, right, mask = p4.make_inputs(*shape)
    cost = p4.cost_volume(p4.census(left, s), p4.census(right, s), D, s, 0, mask)
    with SGM(h, w, s, D, paths=4) as sgm:
        for k in range(4):
            L, m = sgm.stage_path(k, cost)
            Lo, mo = oracle.path(cost, k)
            p4.assert_bits_equal(L, Lo, f"L{k + 1}")
            p4.assert_bits_equal(m, mo, f"minL{k + 1}")
        for k in range(4, 8):
            with pytest.raises(SGMError) as e:
                sgm.stage_path(k, cost)
            assert e.value.code == _capi.SGM_ERR_INVALID_ARG


# (D = 32, 64, 128, 256: by size every shape here runs the split H pair, so
# only the switch reaches the one-launch H pair at each width)
@pytest.mark.parametrize("shape", [p4.SHAPES[k] for k in (2, 3, 4, 5)], ids=[p4.IDS[k] for k in (2, 3, 4, 5)])
@pytest.mark.parametrize("value", ["0", "1"])
@pytest.mark.parametrize("switch", SWITCHES)
def test_switches_force_both_alternatives(shape, switch, value):
    want = p4.expected(shape)
    raw, lr, _ = _two_views(shape, {switch: value})
    p4.assert_bits_equal(raw, want["disp"], f"{switch}={value} raw WTA map")
    p4.assert_bits_equal(lr, want["lr"], f"{switch}={value} LR map")


def _profile(shape, env, **kw):
    h, w, D, s, kind, sky = shape
    left, right, mask = p4.make_inputs(*shape)
    with _Env(env):
        with SGM(h, w, s, D, **kw) as sgm:
            sgm.set_profiling(True)
            sgm.process(left, right, mask, mask)
            return sgm.get_profile()


def test_profile_classes():
    shape = p4.SHAPES[3]
    prof = _profile(shape, {}, paths=4)
    for name in EIGHT_PATH_CLASSES:
        assert name not in prof, sorted(prof)
    for name in ("census", "cost_h", "vfwd", "lr"):
        assert name in prof, sorted(prof)
    assert "final4" in prof, sorted(prof)
    # both views share each launch
    assert prof["final4"][0] == 1 and prof["vfwd"][0] == 1, prof
    # few rows: the two-launch H pair by default; the switch forces either form
    assert "hpair4_fwd" in prof and "hpair4_bwd" in prof and "hpair4" not in prof, sorted(prof)
    one = _profile(shape, {"SGM_P4_HPAIR": "0"}, paths=4)
    assert "hpair4" in one and "hpair4_fwd" not in one and "hpair4_bwd" not in one, sorted(one)
    split = _profile(shape, {"SGM_P4_HPAIR": "1"}, paths=4)
    assert "hpair4_fwd" in split and "hpair4_bwd" in split and "hpair4" not in split, sorted(split)
    # a default handle still runs the 8-path launches
    eight = _profile(shape, {})
    assert "stage_a" in eight and not any(k.startswith(("final4", "hpair4")) for k in eight), sorted(eight)


def test_device_bytes_smaller():
    for h, w, s, D, views in ((48, 150, 1, 64, 2), (50, 141, 1, 128, 1), (96, 300, 2, 64, 2)):
        with SGM(h, w, s, D, views=views) as a, SGM(h, w, s, D, views=views, paths=4) as b:
            assert 0 < b.device_bytes < a.device_bytes, (h, w, D, views)


def test_other_path_counts_are_rejected():
    for bad in (5, 2, 16, -4):
        with pytest.raises((ValueError, SGMError)):
            SGM(48, 150, 1, 64, paths=bad)
    # the C-ABI itself
    import ctypes
    p = _capi.default_params(48, 150, 1, 64)
    p.paths = 5
    handle = ctypes.c_void_p()
    assert _capi.lib().sgm_create(ctypes.byref(p), 0, ctypes.byref(handle)) == _capi.SGM_ERR_INVALID_ARG
    assert not handle.value


def test_zero_and_eight_mean_eight_paths():
    shape = p4.SHAPES[3]
    h, w, D, s, kind, sky = shape
    left, right, mask = p4.make_inputs(*shape)
    ref = oracle.process(left, right, D, s, mask, mask)
    maps = []
    for paths in (0, 8):
        with SGM(h, w, s, D, paths=paths) as sgm:
            assert sgm.params.paths == paths
            sgm.process(left, right, mask, mask)
            maps.append((sgm.get_raw_disp().copy(), sgm.get_lr_disp().copy(), sgm.get_disp().copy()))
    for raw, lr, final in maps:
        p4.assert_bits_equal(raw, ref["disp"], "raw WTA map")
        p4.assert_bits_equal(lr, ref["lr"], "LR map")
        p4.assert_bits_equal(final, ref["final"], "get_disp()")


def test_slant_and_band_switches_are_ignored():
    shape = p4.SHAPES[4]
    want = p4.expected(shape)
    base = _two_views(shape)
    for env in ({"SGM_SLANT": "1"}, {"SGM_BAND_ROWS": "16"}, {"SGM_SLANT": "1", "SGM_BAND_ROWS": "16"}):
        raw, lr, nbytes = _two_views(shape, env)
        p4.assert_bits_equal(raw, base[0], f"{env} raw WTA map")
        p4.assert_bits_equal(lr, base[1], f"{env} LR map")
        assert nbytes == base[2], env   # no band carries, no slanted-tile buffers
        prof = _profile(shape, env, paths=4)
        for name in EIGHT_PATH_CLASSES:
            assert name not in prof, (env, sorted(prof))
    p4.assert_bits_equal(base[1], want["lr"], "LR map")
