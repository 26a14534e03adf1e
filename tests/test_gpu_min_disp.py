"""A minimum disparity m (sgm_set_min_disp, SGM(..., min_disp=m)) on the GPU: the
search range is disparities [m, m + D), every map leaves in true disparity (invalid = D + m + 1).  Bit for bit against
the recipe composed from the oracle's stage functions
(tests/min_disp_recipe.py; tests/test_min_disp_cpu.py pins the recipe itself,
the recovery condition included, which these tests inherit through
bit-equality).

Shapes: a shift beyond the row (every lookup clamps), noise (ties,
rejections), scale 2, a sky mask (sky pixels report m), m = D, D + m > 256,
and widths 16k + {1, 2, 3, 4} under the forced slanted schedule (strip edges).
The D >= 64 shapes also run under SGM_SLANT=1 and SGM_BAND_ROWS=16."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import min_disp_recipe as md
import oracle
import pyref
from stereo_matching_amd import GPU_SGM, SGM, SGMError, _capi

pytestmark = pytest.mark.gpu

SCHEDULES = {"default": {}, "slant": {"SGM_SLANT": "1"}, "bands16": {"SGM_BAND_ROWS": "16"}}
BIG = [x for x in md.SHAPES if x[2] >= 64]


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


def _check_frame(shape, env, paths=8):
    h, w, D, m, s, kind, sky = shape
    want = md.expected(shape, paths)
    left, right, mask = md.make_inputs(shape)
    with _Env(env):
        two = SGM(h, w, s, D, min_disp=m, paths=paths, confidence=True)
        lft = SGM(h, w, s, D, min_disp=m, paths=paths, views=1)
        rgt = SGM(h, w, s, D, min_disp=m, paths=paths, views=1, view="right")
        pf = SGM(h, w, s, D, min_disp=m, paths=paths, post_filter=True)
    with two, lft, rgt, pf:
        assert two.invalid_disp == D + m + 1
        two.process(left, right, mask, mask)
        md.assert_bits_equal(two.get_raw_disp(), want["disp"], "raw WTA map")
        md.assert_bits_equal(two.get_lr_disp(), want["lr"], "LR map")
        md.assert_bits_equal(two.get_confidence(0), want["ratio"], "left confidence")
        md.assert_bits_equal(two.get_confidence(1), want["ratio_beta"], "right confidence")
        md.assert_bits_equal(two.get_disp(), want["final"], "get_disp()")
        lft.process(left, right, mask, mask)
        md.assert_bits_equal(lft.get_raw_disp(), want["disp"], "left raw map (one view)")
        md.assert_bits_equal(lft.get_lr_disp(), want["sub"], "left sub-pixel map")
        rgt.process(left, right, mask, mask)
        md.assert_bits_equal(rgt.get_raw_disp(), want["disp_beta"], "right raw map")
        md.assert_bits_equal(rgt.get_lr_disp(), want["sub_beta"], "right sub-pixel map")
        pf.process(left, right, mask, mask)
        md.assert_bits_equal(pf.get_disp(), want["final"], "post-filtered frame")


@pytest.mark.parametrize("shape", md.SHAPES, ids=md.IDS)
def test_frames(shape):
    _check_frame(shape, {})


@pytest.mark.parametrize("env", ["slant", "bands16"])
@pytest.mark.parametrize("shape", BIG, ids=[md.shape_id(x) for x in BIG])
def test_frames_other_schedules(shape, env):
    _check_frame(shape, SCHEDULES[env])


@pytest.mark.parametrize("shape", md.STRIP_SHAPES, ids=md.STRIP_IDS)
def test_strip_edges_slanted(shape):
    _check_frame(shape, SCHEDULES["slant"])


def test_four_paths():
    _check_frame(md.SHAPES[5], {}, paths=4)


def test_sky_pixels_report_min_disp():
    shape = md.SHAPES[4]
    h, w, D, m, s, kind, sky = shape
    left, right, mask = md.make_inputs(shape)
    with SGM(h, w, s, D, min_disp=m, views=1) as sgm:
        sgm.process(left, right, mask, mask)
        assert (sgm.get_raw_disp()[mask == 255] == m).all()
        assert (sgm.get_lr_disp()[mask == 255] == np.float32(m)).all()


@pytest.mark.parametrize("views", [2, 1])
def test_zero_is_the_default(views):
    h, w, D, s = 50, 141, 128, 1
    left, right = md.synthetic.stereo_pair(h, w, D, pair_index=3)
    mask = md.synthetic.sky_mask(h, w)
    maps = []
    for kw in ({}, {"min_disp": 0}):
        with SGM(h, w, s, D, views=views, **kw) as sgm:
            assert sgm.invalid_disp == D + 1
            sgm.process(left, right, mask, mask)
            maps.append((sgm.get_raw_disp().copy(), sgm.get_lr_disp().copy(), sgm.get_disp().copy(),
                         sgm.device_bytes))
    for k, what in enumerate(("raw", "lr / sub", "final")):
        md.assert_bits_equal(maps[1][k], maps[0][k], what)
    assert maps[0][3] == maps[1][3]       # no shifted tables at min_disp = 0
    ref = oracle.process(left, right, D, s, mask, mask)
    md.assert_bits_equal(maps[1][1], ref["lr" if views == 2 else "sub"], "oracle")
    with SGM(h, w, s, D, views=views, min_disp=16) as sgm:   # two census tables more
        assert sgm.device_bytes == maps[0][3] + 2 * 8 * h * w


def test_stage_entry_points():
    shape = md.SHAPES[4]
    h, w, D, m, s, kind, sky = shape
    left, right, mask = md.make_inputs(shape)
    want = md.expected(shape, lk=True)
    ctl, ctr = md.census(left, s), md.census(right, s)
    ctl_s, ctr_s = md.shift_tables(ctl, ctr, m // s)
    with SGM(h, w, s, D, min_disp=m) as sgm:
        # the census stage returns the unshifted tables, the cost stage shifts
        assert np.array_equal(sgm.stage_census(left), ctl)
        assert np.array_equal(sgm.stage_census(right), ctr)
        c0 = md.cost_volume(ctl, ctr_s, D, s, 0, mask)
        c1 = md.cost_volume(ctl_s, ctr, D, s, 1, mask)
        md.assert_bits_equal(sgm.stage_cost(ctl, ctr, 0, mask), c0, "stage_cost left")
        md.assert_bits_equal(sgm.stage_cost(ctl, ctr, 1, mask), c1, "stage_cost right")
        d, f = sgm.stage_aggregate(c0)
        md.assert_bits_equal(d, want["disp"], "stage_aggregate disp")
        md.assert_bits_equal(f, want["sub"], "stage_aggregate sub")
        md.assert_bits_equal(sgm.stage_lr(want["sub"], want["sub_beta"]), want["lr"], "stage_lr")
    # the side stages on a light handle created with the same min_disp
    with SGM(h, w, s, D, min_disp=m, aux_only=True) as aux:
        assert aux.invalid_disp == D + m + 1
        md.assert_bits_equal(aux.stage_lr(want["sub"], want["sub_beta"]), want["lr"], "aux stage_lr")
        md.assert_bits_equal(aux.post_filter(want["lr"]), want["final"], "stage_post_filter")
        md.assert_bits_equal(aux.lk_refine(left, right, want["final"]), want["lk"], "lk_refine")
        assert not np.array_equal(want["lk"], want["final"])      # LKRefine moved something
        # the confidence filter writes D + m + 1
        got = aux.confidence_filter(want["sub"], want["ratio"], 0.5)
        exp = np.where(want["ratio"] > np.float32(0.5), np.float32(D + m + 1), want["sub"])
        assert (want["ratio"] > np.float32(0.5)).any()
        md.assert_bits_equal(got, exp, "confidence_filter")
        # colormap: the colours of F - m over D (the invalid marker maps to D + 1)
        F = np.array(want["final"])
        F[0, :D] = np.arange(D, dtype=np.float32) + np.float32(m)
        F[1, :3] = np.float32([m, D + m - 1, D + m + 1])
        assert np.array_equal(aux.colormap(F), pyref.colormap(F - np.float32(m), D))
        # point cloud: invalid is D + m + 1
        F[2, :4] = np.float32([D + m + 1, D + 1, m + 0.5, D + m - 1])
        cam = (721.5377, 721.5377, 609.5593, 172.854)
        xyz, pix = aux.point_cloud(F, left, *cam)
        want_xyz, want_pix = pyref.point_cloud(F, left, D + m, s, *cam)
        assert xyz.shape == want_xyz.shape and xyz.shape[0] > 0
        assert np.array_equal(xyz.view(np.uint64), want_xyz.view(np.uint64))
        assert np.array_equal(pix, want_pix)


def test_lk_refine_frame_scale2():
    shape = md.SHAPES[3]
    h, w, D, m, s, kind, sky = shape
    left, right, mask = md.make_inputs(shape)
    want = md.expected(shape, lk=True)
    with SGM(h, w, s, D, min_disp=m, post_filter=True, lk_refine=True) as sgm:
        sgm.process(left, right)
        md.assert_bits_equal(sgm.get_disp(), want["lk"], "post_filter + LKRefine frame")


def test_gpu_sgm_class_passes_min_disp():
    shape = md.SHAPES[2]
    h, w, D, m, s, kind, sky = shape
    left, right, _ = md.make_inputs(shape)
    want = md.expected(shape)
    with GPU_SGM(h, w, s, D, min_disp=m) as g:
        assert g.invalid_disp == D + m + 1
        g.process(left, right)
        md.assert_bits_equal(g.get_disp(), oracle.post_filter(want["sub"], D + m, s), "GPU_SGM")


def test_two_handles_meet_in_lr_check_device():
    shape = md.SHAPES[5]
    h, w, D, m, s, kind, sky = shape
    left, right, _ = md.make_inputs(shape)
    want = md.expected(shape)
    dev = torch.device("cuda", 0)
    dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    fl = torch.empty((h, w), dtype=torch.float32, device=dev)
    fr = torch.empty_like(fl)
    out = torch.empty_like(fl)
    with SGM(h, w, s, D, min_disp=m, views=1) as L, \
            SGM(h, w, s, D, min_disp=m, views=1, view="right") as R, \
            SGM(h, w, s, D, min_disp=m, aux_only=True) as aux:
        L.process_device(dl.data_ptr(), dr.data_ptr(), fl.data_ptr())
        R.process_device(dl.data_ptr(), dr.data_ptr(), fr.data_ptr())
        L.check()
        R.check()
        aux.lr_check_device(fl.data_ptr(), fr.data_ptr(), out.data_ptr())
        aux.check()
        md.assert_bits_equal(out.cpu().numpy(), want["lr"], "lr_check_device")
        aux.post_filter_device(out.data_ptr())
        aux.check()
        md.assert_bits_equal(out.cpu().numpy(), want["final"], "post_filter_device")


@pytest.mark.timeout(120)
def test_post_filtered_frame_replays_from_a_hip_graph():
    shape = md.SHAPES[5]
    h, w, D, m, s, kind, sky = shape
    left, right, _ = md.make_inputs(shape)
    want = md.expected(shape)
    dev = torch.device("cuda", 0)
    with SGM(h, w, s, D, min_disp=m, post_filter=True, post_filter_launches=8) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
        d_l = torch.empty((h, w), dtype=torch.uint8, device=dev)
        d_r = torch.empty_like(d_l)
        out_e = torch.empty((h, w), dtype=torch.float32, device=dev)
        out_g = torch.full((h, w), -1.0, dtype=torch.float32, device=dev)
        with torch.cuda.stream(stream):
            d_l.copy_(torch.from_numpy(left))
            d_r.copy_(torch.from_numpy(right))
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out_e.data_ptr(),
                               stream=stream.cuda_stream)
        torch.cuda.synchronize(dev)
        sgm.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out_g.data_ptr(),
                               stream=stream.cuda_stream)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            graph.replay()
        torch.cuda.synchronize(dev)
        sgm.check()
        md.assert_bits_equal(out_g.cpu().numpy(), out_e.cpu().numpy(), "replayed vs eager")
        md.assert_bits_equal(out_g.cpu().numpy(), want["final"], "replayed vs recipe")


@pytest.mark.parametrize("scale,solver,m", [(1, 0, -1), (2, 0, 1), (1, 0, 65535 - 64), (1, 1, 16)],
                         ids=["negative", "not_a_multiple_of_scale", "u16_overflow", "bm"])
def test_rejections(scale, solver, m):
    lib = _capi.lib()
    p = _capi.default_params(96, 300, scale, 64)
    p.solver = solver
    p.views = 1 if solver else 2
    handle = ctypes.c_void_p()
    assert lib.sgm_create(ctypes.byref(p), 0, ctypes.byref(handle)) == _capi.SGM_OK
    try:
        before = lib.sgm_device_bytes(handle)
        assert lib.sgm_set_min_disp(handle, m) == _capi.SGM_ERR_INVALID_ARG
        assert b"sgm_set_min_disp" in lib.sgm_last_error(handle)
        inv = ctypes.c_int()
        assert lib.sgm_get_invalid_disp(handle, ctypes.byref(inv)) == _capi.SGM_OK
        assert inv.value == 64 + 1 and lib.sgm_device_bytes(handle) == before   # nothing changed
        assert lib.sgm_set_min_disp(handle, 0) == _capi.SGM_OK
    finally:
        lib.sgm_destroy(handle)
    # the Python surface raises the same code and leaves no handle behind
    if solver == 0:
        with pytest.raises(SGMError) as e:
            SGM(96, 300, scale, 64, min_disp=m)
        assert e.value.code == _capi.SGM_ERR_INVALID_ARG
    # the largest accepted value is one below the refused one
    if m == 65535 - 64:
        with SGM(24, 40, 1, 32, min_disp=65535 - 32 - 1, aux_only=True) as aux:
            assert aux.invalid_disp == 65535


def test_set_and_clear_on_a_live_handle():
    """The setter after frames have run: the next frame follows the new range,
    and 0 brings the handle back to the default maps and device bytes."""
    shape = md.SHAPES[5]
    h, w, D, m, s, kind, sky = shape
    left, right, _ = md.make_inputs(shape)
    want = md.expected(shape)
    ref = oracle.process(left, right, D, s)
    lib = _capi.lib()
    with SGM(h, w, s, D) as sgm:
        base = sgm.device_bytes
        sgm.process(left, right)
        md.assert_bits_equal(sgm.get_lr_disp(), ref["lr"], "default range")
        _capi.check(lib.sgm_set_min_disp(sgm._h, m), sgm._h)
        assert sgm.device_bytes == base + 2 * 8 * h * w
        sgm.process(left, right)
        md.assert_bits_equal(sgm.get_lr_disp(), want["lr"], "after sgm_set_min_disp(m)")
        md.assert_bits_equal(sgm.get_raw_disp(), want["disp"], "raw after sgm_set_min_disp(m)")
        _capi.check(lib.sgm_set_min_disp(sgm._h, 0), sgm._h)
        assert sgm.device_bytes == base
        sgm.process(left, right)
        md.assert_bits_equal(sgm.get_lr_disp(), ref["lr"], "after sgm_set_min_disp(0)")
