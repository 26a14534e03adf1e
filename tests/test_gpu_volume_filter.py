"""The reference's cost filters on a finished volume (sgm_set_volume_filter,
sgm_filter_volume_device), bit for bit against the oracle's
filters and tests/volume_filter_recipe.py: the stage on widths around the
kernel's block, the device call on torch tensors, aggregate() and SAD / SSD
frames with the setting, the census tie, the caller-side equivalence, off is
off, a HIP graph replay and the refusals."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oracle
import volume_filter_recipe as fr
import volume_recipe as vr
import window_cost_recipe as wc
from stereo_matching_amd import BM, SGM, _capi
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 7.0


def block():
    return _capi.lib().sgm_volume_filter_block()


def widths():
    """The smallest legal width (one filter step) and both sides of the main loop's block."""
    U = block()
    return [5, 6, 7, 5 + U - 1, 5 + U, 5 + U + 1, 5 + 2 * U + 1]


def want(C, s, bits):
    return fr.filtered(C, s, bits)


def same(a, b):
    return np.array_equal(fr.bits(a), fr.bits(b))


# ------------------------------------------------------ the stage against the oracle

@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("scale", [1, 2])
def test_stage_equals_the_oracle_at_every_width(D, scale):
    for k, w in enumerate(widths()):
        rows = (3, 4, 9)[k % 3]
        C = fr.mixed_volume(rows, w, D, seed=100 + k)
        with SGM(rows * scale, w * scale, scale, D, views=1) as s:
            for bits in (1, 2, 3):
                got = s.stage_filter_volume(C, bool(bits & 1), bool(bits & 2))
                assert same(got, want(C, scale, bits)), (w, rows, bits)


@pytest.mark.parametrize("rows", [3, 4, 9])
def test_stage_rows_and_a_width_below_d(rows):
    D, w = 64, 37  # cols < D
    C = fr.mixed_volume(rows, w, D, seed=rows)
    with SGM(rows, w, 1, D) as s:
        for bits in (1, 2, 3):
            assert same(s.stage_filter_volume(C, bool(bits & 1), bool(bits & 2)), want(C, 1, bits)), bits


def test_stage_undershoot_volume():
    rows, w, D = 9, 70, 32
    C = fr.undershoot_volume(rows, w, D)
    with SGM(rows, w, 1, D, views=1) as s:
        got = s.stage_filter_volume(C)
        assert got.min() < 0.0
        assert same(got, want(C, 1, 3))
        assert same(s.stage_filter_volume(C, True, False), want(C, 1, 1))


# ------------------------------------------------------ the device call on a torch tensor

def test_filter_volume_on_torch_tensors():
    rows, w, D = 9, 70, 64
    C = fr.mixed_volume(rows, w, D)
    with SGM(rows, w, 1, D) as s:
        for bits in (1, 2, 3):
            h, v = bool(bits & 1), bool(bits & 2)
            stage = s.stage_filter_volume(C, h, v)
            # torch's default stream (through the handle's own)
            t = torch.tensor(C, device=DEV)
            assert s.filter_volume(t, h, v) is t
            torch.cuda.synchronize(DEV)
            assert same(t.cpu().numpy(), stage)
            # the handle's stream
            own = torch.cuda.ExternalStream(s.stream, device=DEV)
            with torch.cuda.stream(own):
                t = torch.tensor(C, device=DEV)
                s.filter_volume(t, h, v)
            own.synchronize()
            assert same(t.cpu().numpy(), stage)
            # a side stream, inside a canary
            side = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(side):
                buf = torch.full((C.size + 128,), CANARY, dtype=torch.float32, device=DEV)
                t = buf[64:64 + C.size].view(rows, w, D)
                t.copy_(torch.from_numpy(C))
                s.filter_volume(t, h, v)
            side.synchronize()
            b = buf.cpu().numpy()
            assert same(b[64:64 + C.size].reshape(C.shape), stage)
            assert (b[:64] == CANARY).all() and (b[64 + C.size:] == CANARY).all()
        with pytest.raises(TypeError, match="stage_filter_volume"):
            s.filter_volume(C)
        with pytest.raises(ValueError, match="contiguous"):
            s.filter_volume(torch.zeros((D, rows, w), device=DEV).permute(1, 2, 0))


# ------------------------------------------------------ frames

def device_volume(C, layout, dtype, variant):
    store, off, (sr, sc, sd) = vr.source(C, layout, dtype, variant)
    t = torch.from_numpy(store).to(DEV)
    H, W, D = C.shape
    if layout == "hwd":
        return torch.as_strided(t, (H, W, D), (sr, sc, sd), off)
    return torch.as_strided(t, (D, H, W), (sd, sr, sc), off)


# (h, w, D, scale, views, paths, min_disp, layout, fp16, variant)
AGG_CASES = [
    (12, 37, 32, 1, 1, 8, 0, "hwd", False, "dense"),
    (12, 37, 32, 1, 2, 8, 0, "dhw", True, "padded"),
    (12, 37, 32, 1, 2, 4, 0, "hwd", False, "padded"),
    (12, 37, 32, 1, 1, 4, 0, "dhw", False, "dense"),
    (9, 70, 64, 1, 2, 8, 16, "hwd", True, "batch"),
    (9, 70, 64, 1, 2, 4, 16, "dhw", False, "offset"),
    (9, 70, 64, 2, 2, 8, 0, "dhw", False, "padded"),
    (9, 70, 64, 2, 1, 8, 0, "hwd", True, "dense"),
    (24, 80, 128, 1, 2, 8, 0, "hwd", False, "padded"),
]


@pytest.mark.parametrize("h,w,D,scale,views,paths,m,layout,f16,variant", AGG_CASES)
def test_aggregate_with_the_setting_equals_the_recipe(h, w, D, scale, views, paths, m, layout, f16, variant):
    C = fr.frame_volume(h, w, D, f16)
    e = fr.expected(h, w, D, m, scale, paths, f16)
    src = device_volume(C, layout, np.float16 if f16 else np.float32, variant)
    with SGM(h * scale, w * scale, scale, D, views=views, paths=paths, min_disp=m, confidence=True,
             volume_filter=(True, True)) as s:
        assert s.volume_filter == (True, True)
        before = s.device_bytes
        raw = torch.zeros((h, w), dtype=torch.int16, device=DEV)
        got = s.aggregate(src, layout=layout, raw=raw)
        s.check()
        assert same(got.cpu().numpy(), e["lr"] if views == 2 else e["sub"])
        assert np.array_equal(raw.cpu().numpy().view(np.uint16).astype(np.int64), e["disp"].astype(np.int64))
        assert same(s.get_confidence(0), e["ratio"])
        if views == 2:
            assert same(s.get_confidence(1), e["ratio_beta"])
        assert s.device_bytes == before
        # each filter alone
        for bits in (1, 2):
            s.set_volume_filter(bool(bits & 1), bool(bits & 2))
            e1 = fr.expected(h, w, D, m, scale, paths, f16, bits)
            got = s.aggregate(src, layout=layout)
            s.check()
            assert same(got.cpu().numpy(), e1["lr"] if views == 2 else e1["sub"]), bits


def test_aggregate_post_filter_with_a_budget_and_confidence():
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    e = fr.expected(h, w, D)
    with SGM(h, w, 1, D, post_filter=True, post_filter_launches=8, confidence=True,
             volume_filter=(True, True)) as s:
        got = s.aggregate(torch.tensor(C, device=DEV))
        s.check()
        assert same(got.cpu().numpy(), e["final"])
        assert same(s.get_confidence(0), e["ratio"])


@pytest.mark.parametrize("kind", ["sad", "ssd"])
@pytest.mark.parametrize("h,w,D,scale,views", [(12, 37, 32, 1, 2), (9, 70, 64, 2, 2), (12, 37, 32, 1, 1)])
def test_window_cost_frames_with_the_setting(kind, h, w, D, scale, views):
    left, right = vr.road_pair(h, w, D, scale)
    C = wc.volume(left, right, D, kind, scale, 0)
    e = fr.recipe(C, 0, scale)
    with SGM(h * scale, w * scale, scale, D, views=views, cost=kind, volume_filter=(True, True)) as s:
        s.process(left, right)
        assert same(s.get_lr_disp(), e["lr"] if views == 2 else e["sub"])
        s.set_volume_filter(False, True)
        e2 = fr.recipe(C, 0, scale, 8, 2)
        s.process(left, right)
        assert same(s.get_lr_disp(), e2["lr"] if views == 2 else e2["sub"])


@pytest.mark.parametrize("h,w,D,scale", [(24, 80, 32, 1), (24, 80, 32, 2), (20, 40, 128, 1)])
def test_the_census_frame_from_its_own_raw_dsi(h, w, D, scale):
    left, right = vr.road_pair(h, w, D, scale)
    ctl, ctr = vr.road_tables(h, w, D, scale)
    raw_dsi = oracle.dsi(ctl, ctr, D, scale, 0, None)
    with SGM(h * scale, w * scale, scale, D, views=1, volume_filter=(True, True)) as s:
        s.process(left, right)  # (a census frame: the setting plays no part)
        frame_sub, frame_raw = s.get_lr_disp().copy(), s.get_raw_disp().copy()
        raw = torch.zeros((h, w), dtype=torch.int16, device=DEV)
        got = s.aggregate(torch.tensor(raw_dsi, device=DEV), raw=raw)
        s.check()
        assert same(got.cpu().numpy(), frame_sub)
        assert np.array_equal(raw.cpu().numpy().view(np.uint16), frame_raw.astype(np.uint16))


# ------------------------------------------------------ equivalence, off is off

def test_filter_then_aggregate_equals_the_setting_on_one_view():
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    with SGM(h, w, 1, D, views=1) as s:
        t = s.filter_volume(torch.tensor(C, device=DEV))
        a = s.aggregate(t).cpu().numpy()
        s.set_volume_filter(True, True)
        b = s.aggregate(torch.tensor(C, device=DEV)).cpu().numpy()
        s.check()
    assert same(a, b) and same(a, fr.expected(h, w, D)["sub"])


def test_two_views_filter_after_the_derivation():
    # the caller filters only the left volume, so the right view differs by definition: the
    # library's order, derive then filter, is the recipe's (seen in the right view's confidence
    # map; the LR check may well keep the same pixels either way)
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    lib_order, caller_order = fr.expected(h, w, D), fr.caller_side(C)
    assert not same(lib_order["ratio_beta"], caller_order["ratio_beta"])
    with SGM(h, w, 1, D, confidence=True) as s:
        t = s.filter_volume(torch.tensor(C, device=DEV))
        a = s.aggregate(t).cpu().numpy()
        a_beta = s.get_confidence(1).copy()
        s.set_volume_filter(True, True)
        b = s.aggregate(torch.tensor(C, device=DEV)).cpu().numpy()
        b_beta = s.get_confidence(1).copy()
        s.check()
    assert same(a, caller_order["lr"]) and same(a_beta, caller_order["ratio_beta"])
    assert same(b, lib_order["lr"]) and same(b_beta, lib_order["ratio_beta"])
    assert not same(b_beta, caller_order["ratio_beta"])


@pytest.mark.parametrize("views", [1, 2])
def test_off_is_off(views):
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    src = torch.tensor(C, device=DEV)
    with SGM(h, w, 1, D, views=views) as s:
        assert s.volume_filter == (False, False)
        fresh = s.aggregate(src).cpu().numpy()
    with SGM(h, w, 1, D, views=views) as s:
        s.set_volume_filter(True, True)
        on = s.aggregate(src).cpu().numpy()
        s.set_volume_filter(False, False)
        assert s.volume_filter == (False, False)
        off = s.aggregate(src).cpu().numpy()
        s.check()
    assert same(off, fresh) and not same(on, fresh)
    assert same(fresh, vr.recipe(C)["lr" if views == 2 else "sub"])


# ------------------------------------------------------ graph capture

@pytest.mark.timeout(120)
def test_filtered_aggregate_replays_from_a_hip_graph():
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    e = fr.expected(h, w, D)
    with SGM(h, w, 1, D, post_filter=True, post_filter_launches=8, volume_filter=(True, True)) as s:
        stream = torch.cuda.ExternalStream(s.stream, device=DEV)
        out = torch.empty((h, w), dtype=torch.float32, device=DEV)
        with torch.cuda.stream(stream):
            cost = torch.tensor(C, device=DEV)
            s.aggregate(cost, out=out)  # once eagerly before capturing
        torch.cuda.synchronize(DEV)
        s.check()
        assert same(out.cpu().numpy(), e["final"])
        before = s.device_bytes
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            s.aggregate(cost, out=out)
        torch.cuda.synchronize(DEV)
        out.zero_()
        with torch.cuda.stream(stream):
            graph.replay()
        torch.cuda.synchronize(DEV)
        s.check()
        assert same(out.cpu().numpy(), e["final"])
        assert s.device_bytes == before


# ------------------------------------------------------ refusals

def test_refusals_change_nothing():
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    L = _capi.lib()
    vol = torch.tensor(C, device=DEV)

    def refused(s, word, f):
        with pytest.raises(SGMError, match=word) as ei:
            f()
        assert ei.value.code == _capi.SGM_ERR_INVALID_ARG

    def device_call(s, ptr, bits, stream=None):
        _capi.check(L.sgm_filter_volume_device(s._h, ctypes.c_void_p(ptr), bits, ctypes.c_void_p(stream)), s._h)

    with SGM(h, w, 1, D) as s:
        s.set_volume_filter(True, False)
        refused(s, "filters", lambda: _capi.check(L.sgm_set_volume_filter(s._h, 4), s._h))
        refused(s, "filters", lambda: _capi.check(L.sgm_set_volume_filter(s._h, -1), s._h))
        assert s.volume_filter == (True, False)
        refused(s, "filters", lambda: device_call(s, vol.data_ptr(), 0))
        refused(s, "filters", lambda: device_call(s, vol.data_ptr(), 4))
        refused(s, "NULL", lambda: device_call(s, 0, 3))
        refused(s, "aligned", lambda: device_call(s, vol.data_ptr() + 4, 3))
        refused(s, "hipStreamLegacy", lambda: device_call(s, vol.data_ptr(), 3, 1))
    for word, make in [("BM", lambda: BM(h, w, 1, D)), ("aux_only", lambda: SGM(h, w, 1, D, aux_only=True)),
                       ("SGM_VIEW_RIGHT", lambda: SGM(h, w, 1, D, views=1, view="right"))]:
        with make() as s:
            refused(s, word, lambda: s.set_volume_filter(True, True))
            assert s.volume_filter == (False, False)
    with SGM(h, w, 1, D, aux_only=True) as s:
        refused(s, "aux_only", lambda: device_call(s, vol.data_ptr(), 3))
        refused(s, "aux_only", lambda: s.stage_filter_volume(C))
    torch.cuda.synchronize(DEV)
    assert same(vol.cpu().numpy(), C)
