"""The per-pixel match confidence (sgm_set_confidence): the uniqueness test's
own quotient min_cost / sec_min_cost (SGM.cpp:392-409), stored by every final
pass beside the sub-pixel map, bit for bit against the recipe composed from
the oracle's stage functions (tests/confidence_recipe.py;
tests/test_confidence_cpu.py pins the recipe itself).

Shapes (paths4_recipe.SHAPES): the minimum 3 x 5 frame, W < D (clamped columns:
tied costs, pixels without a second value), D = 32 (half a wave), 64, 128 and
256, scale 2, sky masks; every schedule that ends in a WTA."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import confidence_recipe as cr
from stereo_matching_amd import BM, SGM, SGMError, _capi

pytestmark = pytest.mark.gpu

VIEWS = (("left", 0), ("right", 1))


class _Env:
    """Environment switches read at sgm_create (as test_gpu_schedules._run sets them)."""

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


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("shape", cr.SHAPES, ids=cr.IDS)
def test_two_views(shape, paths):
    h, w, D, s, kind, sky = shape
    left, right, mask = cr.make_inputs(*shape)
    want = cr.expected(shape, paths)
    with SGM(h, w, s, D, paths=paths, confidence=True) as sgm:
        sgm.process(left, right, mask, mask)
        for name, v in VIEWS:
            cr.assert_bits_equal(sgm.get_confidence(v), want[v], f"{name} ratio map")


ONE_VIEW = [cr.SHAPES[k] for k in (0, 4, 5)]


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("shape", ONE_VIEW, ids=[cr.IDS[k] for k in (0, 4, 5)])
def test_one_view_handles(shape, paths):
    h, w, D, s, kind, sky = shape
    left, right, mask = cr.make_inputs(*shape)
    want = cr.expected(shape, paths)
    for name, v in VIEWS:
        with SGM(h, w, s, D, paths=paths, views=1, view=name, confidence=True) as sgm:
            sgm.process(left, right, mask, mask)
            cr.assert_bits_equal(sgm.get_confidence(v), want[v], f"{name}-view handle's ratio map")


@pytest.mark.parametrize("env", [{}, {"SGM_BAND_ROWS": "16"}, {"SGM_BAND_ROWS": "0"}, {"SGM_SLANT": "1"}],
                         ids=["default", "bands16", "whole", "slant"])
@pytest.mark.parametrize("h,w,D", cr.SCHEDULE_SHAPES)
def test_schedules(h, w, D, env):
    left, right, mask = cr.schedule_inputs(h, w, D)
    want = cr.schedule_expected(h, w, D)
    with _Env(env):
        with SGM(h, w, 1, D, confidence=True) as sgm:
            sgm.process(left, right, mask, mask)
            for name, v in VIEWS:
                cr.assert_bits_equal(sgm.get_confidence(v), want[v], f"{env} {name} ratio map")


def test_schedules_one_view_slant_and_bands():
    # the row-major final passes of the one-view schedules
    h, w, D = cr.SCHEDULE_SHAPES[0]
    left, right, mask = cr.schedule_inputs(h, w, D)
    want = cr.schedule_expected(h, w, D)
    for env in ({"SGM_SLANT": "1"}, {"SGM_BAND_ROWS": "16"}):
        with _Env(env):
            with SGM(h, w, 1, D, views=1, confidence=True) as sgm:
                sgm.process(left, right, mask, mask)
                cr.assert_bits_equal(sgm.get_confidence(0), want[0], f"{env} one-view ratio map")


def test_stage_aggregate_stores_the_ratio():
    for shape, paths in ((cr.SHAPES[3], 8), (cr.SHAPES[5], 4)):
        h, w, D, s, kind, sky = shape
        left, right, mask = cr.make_inputs(*shape)
        cost = cr.cost_volume(cr.census(left, s), cr.census(right, s), D, s, 0, mask)
        with SGM(h, w, s, D, paths=paths, confidence=True) as sgm:
            sgm.stage_aggregate(cost)
            cr.assert_bits_equal(sgm.get_confidence(0), cr.expected(shape, paths)[0], "stage_aggregate ratio")


def test_pitched_destination():
    shape = cr.SHAPES[4]
    h, w, D, s, kind, sky = shape
    left, right, mask = cr.make_inputs(*shape)
    want = cr.expected(shape, 8)
    dev = torch.device("cuda", 0)
    pitch = w + 7
    for views, todo in ((2, VIEWS), (1, VIEWS[:1])):
        with SGM(h, w, s, D, views=views, confidence=True) as sgm:
            sgm.process(left, right, mask, mask)
            for name, v in todo:
                buf = torch.full((h, pitch), -9.0, dtype=torch.float32, device=dev)
                torch.cuda.synchronize(dev)
                sgm.confidence_device(buf.data_ptr(), view=v, pitch=pitch)
                sgm.check()
                got = buf.cpu().numpy()
                cr.assert_bits_equal(got[:, :w], want[v], f"views={views} {name} pitched ratio map")
                assert (got[:, w:] == -9.0).all(), "padding written"


def test_disparity_maps_unchanged_by_the_switch():
    shape = cr.SHAPES[6]
    h, w, D, s, kind, sky = shape
    left, right, mask = cr.make_inputs(*shape)
    for paths in (8, 4):
        with SGM(h, w, s, D, paths=paths) as off:
            off.process(left, right, mask, mask)
            lr0, raw0 = off.get_lr_disp().copy(), off.get_raw_disp().copy()
            nbytes = off.device_bytes
        with SGM(h, w, s, D, paths=paths, confidence=True) as sgm:
            assert sgm.device_bytes == nbytes + 2 * sgm.rows * sgm.cols * 4
            sgm.process(left, right, mask, mask)
            cr.assert_bits_equal(sgm.get_lr_disp(), lr0, "LR map with confidence on")
            cr.assert_bits_equal(sgm.get_raw_disp(), raw0, "raw map with confidence on")
            sgm.set_confidence(False)
            assert sgm.device_bytes == nbytes
            sgm.process(left, right, mask, mask)
            cr.assert_bits_equal(sgm.get_lr_disp(), lr0, "LR map after set_confidence(False)")
            cr.assert_bits_equal(sgm.get_raw_disp(), raw0, "raw map after set_confidence(False)")
            with pytest.raises(SGMError):
                sgm.get_confidence()
            sgm.set_confidence(True)   # and on again
            sgm.process(left, right, mask, mask)
            cr.assert_bits_equal(sgm.get_confidence(0), cr.expected(shape, paths)[0], "ratio after re-enabling")


def _refused(fn):
    with pytest.raises(SGMError) as e:
        fn()
    assert e.value.code == _capi.SGM_ERR_INVALID_ARG, e.value


def test_refusals():
    h, w, D = 48, 150, 64
    dev = torch.device("cuda", 0)
    buf = torch.zeros((h, w), dtype=torch.float32, device=dev)
    with SGM(h, w, 1, D) as sgm:                       # before enabling
        _refused(lambda: sgm.confidence_device(buf.data_ptr()))
        _refused(lambda: sgm.get_confidence())
        sgm.set_confidence(True)
        _refused(lambda: sgm.confidence_device(buf.data_ptr(), view=2))
        _refused(lambda: sgm.confidence_device(buf.data_ptr(), pitch=w - 1))
        sgm.confidence_device(buf.data_ptr())
        sgm.check()
    with BM(h, w, 1, D) as bm:
        _refused(lambda: bm.set_confidence(True))
        _refused(lambda: bm.confidence_device(buf.data_ptr()))
    with SGM(h, w, 1, D, aux_only=True) as aux:
        _refused(lambda: aux.set_confidence(True))
        _refused(lambda: aux.confidence_device(buf.data_ptr()))
    with SGM(h, w, 1, D, views=1, confidence=True) as one:   # the view a one-view handle lacks
        _refused(lambda: one.confidence_device(buf.data_ptr(), view=1))
        one.confidence_device(buf.data_ptr(), view=0)
        one.check()
    with SGM(h, w, 1, D, views=1, view="right", confidence=True) as one:
        _refused(lambda: one.confidence_device(buf.data_ptr(), view=0))
        one.confidence_device(buf.data_ptr(), view=1)
        one.check()
    with pytest.raises(SGMError):
        SGM(h, w, 1, D, aux_only=True, confidence=True)
    # the C-ABI's null checks
    L = _capi.lib()
    assert L.sgm_set_confidence(None, 1) == _capi.SGM_ERR_INVALID_ARG
    assert L.sgm_confidence_device(None, 0, ctypes.c_void_p(buf.data_ptr()), w, None) == _capi.SGM_ERR_INVALID_ARG


def test_filter():
    shape = cr.SHAPES[3]
    h, w, D, s, kind, sky = shape
    left, right, mask = cr.make_inputs(*shape)
    with SGM(h, w, s, D, confidence=True) as sgm:
        sgm.process(left, right, mask, mask)
        lr = sgm.get_lr_disp().copy()
        ratio = sgm.get_confidence(0)
    cr.assert_bits_equal(ratio, cr.expected(shape, 8)[0], "left ratio map")
    with SGM(h, w, s, D, aux_only=True) as aux:    # any handle of the working size serves
        got = aux.confidence_filter(lr, ratio, 0.5)
        want = np.where(ratio > np.float32(0.5), np.float32(D + 1), lr)
        assert 0 < (want != lr).sum() < lr.size     # the stricter ratio removes some pixels
        cr.assert_bits_equal(got, want, "confidence_filter(0.5)")
        # 1.0 changes nothing wherever the quotient stays below 1 (next to this
        # shape's sky mask a negative path cost can push it above: those go)
        got1 = aux.confidence_filter(lr, ratio, 1.0)
        cr.assert_bits_equal(got1, np.where(ratio > np.float32(1.0), np.float32(D + 1), lr),
                             "confidence_filter(1.0)")
        # pitched device maps, in place, padding untouched
        dev = torch.device("cuda", 0)
        pd, pr = w + 5, w + 3
        d_f = torch.full((h, pd), -9.0, dtype=torch.float32, device=dev)
        d_r = torch.full((h, pr), 2.0, dtype=torch.float32, device=dev)
        d_f[:, :w] = torch.from_numpy(lr).to(dev)
        d_r[:, :w] = torch.from_numpy(ratio).to(dev)
        torch.cuda.synchronize(dev)
        aux.confidence_filter_device(d_f.data_ptr(), d_r.data_ptr(), 0.5, pitch=pd, ratio_pitch=pr)
        aux.check()
        out = d_f.cpu().numpy()
        cr.assert_bits_equal(out[:, :w], want, "confidence_filter_device(0.5)")
        assert (out[:, w:] == -9.0).all(), "padding written"


def test_filter_one_changes_nothing_without_masks():
    shape = cr.SHAPES[2]
    h, w, D, s, kind, sky = shape
    assert not sky
    left, right, mask = cr.make_inputs(*shape)
    with SGM(h, w, s, D, confidence=True) as sgm:
        sgm.process(left, right)
        lr = sgm.get_lr_disp().copy()
        ratio = sgm.get_confidence(0)
        assert (ratio >= 0).all() and (ratio < 1).all()
        cr.assert_bits_equal(sgm.confidence_filter(lr, ratio, 1.0), lr, "confidence_filter(1.0)")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("views,slant", [(2, False), (1, False), (2, True)])
def test_frame_and_confidence_replay_from_a_hip_graph(views, slant, monkeypatch):
    from stereo_matching_amd import synthetic
    monkeypatch.setenv("SGM_SLANT", "1" if slant else "0")
    h, w, D = 96, 260, 128
    dev = torch.device("cuda", 0)
    with SGM(h, w, 1, D, views=views, confidence=True) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
        d_l = torch.empty((h, w), dtype=torch.uint8, device=dev)
        d_r = torch.empty_like(d_l)
        maps = {k: [torch.empty((h, w), dtype=torch.float32, device=dev) for _ in range(1 + views)]
                for k in ("eager", "graph")}

        def frame(out):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out[0].data_ptr(), stream=stream.cuda_stream)
            for v in range(views):
                sgm.confidence_device(out[1 + v].data_ptr(), view=v, stream=stream.cuda_stream)

        def load(k):
            left, right = synthetic.stereo_pair(h, w, D, pair_index=k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))

        load(0)
        with torch.cuda.stream(stream):
            frame(maps["eager"])  # warm-up
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(maps["graph"])
        torch.cuda.synchronize(dev)
        for k in (1, 2):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
                frame(maps["eager"])
            torch.cuda.synchronize(dev)
            for i, (g, e) in enumerate(zip(maps["graph"], maps["eager"])):
                cr.assert_bits_equal(g.cpu().numpy(), e.cpu().numpy(), f"replay {k} map {i}")
            assert float(maps["graph"][1].abs().max()) > 0   # (a ratio map, not the memset's zeros)
