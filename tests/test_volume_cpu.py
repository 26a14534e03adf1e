"""The caller's-volume recipe (tests/volume_recipe.py) against the oracle, on
the CPU: it is the frame from C on, its derived right volume is an identity of
the reference's raw DSIs wherever the column index is not clamped, and the
volumes the GPU tests use exercise the LR check."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
import volume_recipe as vr
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.build()


@pytest.mark.parametrize("h,w,D,s", [(24, 80, 32, 1), (20, 40, 128, 1), (24, 80, 32, 2)])
def test_recipe_is_the_frame_from_c_on(h, w, D, s):
    # (a) fed the oracle's filtered DSI, the left maps are oracle.process's, bit for bit
    left, right = vr.road_pair(h, w, D, s)
    ref = oracle.process(left, right, D, scale=s, views=1)
    disp, sub, _ = vr.view_maps(vr.road_volume(h, w, D, s), 0, 8)
    assert np.array_equal(vr.bits(sub), vr.bits(ref["sub"]))
    assert np.array_equal(disp, ref["disp"])


@pytest.mark.parametrize("h,w,D,s,floor", [(24, 80, 32, 1, 0.75), (24, 80, 32, 2, 0.75), (12, 300, 64, 1, 0.75)])
def test_derived_right_volume_is_the_raw_right_dsi_where_unclamped(h, w, D, s, floor):
    # (b) no filters, no mask: ham(ctL[j + k], ctR[j]) is the left DSI at column j + k
    ctl, ctr = vr.road_tables(h, w, D, s)
    got = vr.derive_right(oracle.dsi(ctl, ctr, D, s, 0, None), 0, s)
    want = oracle.dsi(ctl, ctr, D, s, 1, None)
    keep = vr.unclamped(w, D, 0, s)
    assert keep.mean() >= floor  # (24 x 80, D = 32: 0.81)
    assert np.array_equal(vr.bits(got)[:, keep], vr.bits(want)[:, keep])
    assert not np.array_equal(vr.bits(got), vr.bits(want))  # the clamped columns do differ


def test_derived_right_volume_by_hand():
    C = np.arange(2 * 5 * 4, dtype=np.float32).reshape(2, 5, 4)
    R = vr.derive_right(C, 2, 2)  # shifts (d + 2) // 2 = 1, 1, 2, 2
    for i in range(2):
        for j in range(5):
            for d in range(4):
                assert R[i, j, d] == C[i, min(j + (d + 2) // 2, 4), d]


# (name, min_disp) of every aggregate case of tests/test_gpu_volume.py
GPU_CASES = [(n, 0) for n in vr.GPU_VOLUMES] + [("road_24x80_D32", 16), ("noise_24x80_D32", 16)]


@pytest.mark.parametrize("name,m", GPU_CASES)
@pytest.mark.parametrize("f16", [False, True])
def test_gpu_volumes_exercise_the_lr_check(name, m, f16):
    # (c) between 5% and 95% valid after the LR check, and at least one pixel it invalidated
    D = vr.GPU_VOLUMES[name][3]
    e = vr.expected(name, m, 8, f16)
    inv = np.float32(D + m + 1)
    valid = float((e["lr"] != inv).mean())
    assert 0.05 <= valid <= 0.95, valid
    assert ((e["lr"] == inv) & (e["sub"] != inv)).any()
    c = vr.gpu_volume(name, f16)
    assert c.min() >= 0.0 and c.max() <= 999999.0 and np.isfinite(c).all()
    if f16:
        assert np.array_equal(c, c.astype(np.float16).astype(np.float32))


def test_sources_hold_the_volume():
    C = vr.noise_volume(3, 5, 32)
    for layout in ("hwd", "dhw"):
        for variant in vr.VARIANTS:
            store, off, (sr, sc, sd) = vr.source(C, layout, np.float32, variant)
            assert (sd == 1) != (sc == 1)
            i, j, d = 2, 3, 17
            assert store[off + i * sr + j * sc + d * sd] == C[i, j, d]
            assert off + 2 * sr + 4 * sc + 31 * sd < store.size
            assert (store == 7.0).sum() >= store.size - C.size


def test_surface_is_declared():
    header = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    assert "enum { SGM_VOL_F32 = 0, SGM_VOL_F16 = 1 };" in header
    assert "#define SGM_HIP_VERSION 2 " in header  # the struct and the version stay
    assert {"sgm_volume_import_device", "sgm_aggregate_device"} <= set(_capi.EXPORTS)
    assert (_capi.SGM_VOL_F32, _capi.SGM_VOL_F16) == (0, 1)
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    assert "sgm_volume.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]


def test_python_surface_refuses_host_arrays():
    # torch is imported inside the methods only; a numpy volume is pointed at stage_aggregate
    from stereo_matching_amd.solver import SGM
    s = SGM.__new__(SGM)
    s.rows, s.cols, s.max_disp, s.device = 3, 5, 32, 0
    with pytest.raises(TypeError, match="stage_aggregate"):
        s._volume(np.zeros((3, 5, 32), np.float32), None)
    s._h = None
