"""A caller's device cost volume in, maps out (sgm_volume_import_device,
sgm_aggregate_device), bit for bit against tests/volume_recipe.py:
the import of both views from every layout, element type and stride form, the
frame from the cost volume on (8 and 4 paths, one and two views, min_disp,
scale 2, confidence, post filter, reprojection), every schedule's handle, a HIP
graph replay, the refusals and the torch surface."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oracle
import reproject_recipe as rp
import volume_recipe as vr
from stereo_matching_amd import BM, SGM, _capi
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 7.0


def device_volume(C, layout, dtype, variant):
    """C as a strided torch device tensor (vr.source): shape (H, W, D) or, dhw, (D, H, W)."""
    store, off, (sr, sc, sd) = vr.source(C, layout, dtype, variant)
    t = torch.from_numpy(store).to(DEV)
    H, W, D = C.shape
    if layout == "hwd":
        return torch.as_strided(t, (H, W, D), (sr, sc, sd), off)
    return torch.as_strided(t, (D, H, W), (sd, sr, sc), off)


def import_volume_values(h, w, D, dtype, seed):
    """A volume for the import: fp16, every binary16 class in range (zero, subnormals, 65504);
    fp32, arbitrary bit patterns in [0, 999999]."""
    rng = np.random.default_rng(seed)
    if dtype == np.float16:
        c = rng.integers(0, 0x7C00, (h, w, D), dtype=np.uint16)
        c.reshape(-1)[:6] = [0, 1, 0x03FF, 0x0400, 0x7BFF, 0x3C00]
        return c.view(np.float16).astype(np.float32)
    c = rng.uniform(0.0, 999999.0, (h, w, D)).astype(np.float32)
    c.reshape(-1)[:4] = [0.0, 999999.0, 1e-40, np.float32(1.17549435e-38)]
    return c


def guarded_out(h, w, D, shift=0):
    """(buffer, view): a (h, w, D) float32 destination inside a canary-filled buffer; shift: the
    destination's offset from 256-byte alignment, in floats."""
    n = h * w * D
    buf = torch.full((n + 128,), CANARY, dtype=torch.float32, device=DEV)
    return buf, buf[64 + shift:64 + shift + n].view(h, w, D)


def assert_guards(buf, n, shift=0):
    b = buf.cpu().numpy()
    assert (b[:64 + shift] == CANARY).all() and (b[64 + shift + n:] == CANARY).all()


LEFT_SHAPES = [(3, 5, 32), (5, 33, 64), (7, 63, 32), (7, 64, 32), (7, 65, 128), (4, 130, 256)]
RIGHT_SHAPES = [(3, 5, 32), (5, 33, 32), (7, 65, 128), (4, 130, 256)]  # W < D; W = D + 1; more than one tile


@pytest.mark.parametrize("h,w,D", LEFT_SHAPES)
def test_import_left_is_the_relayout(h, w, D):
    with SGM(h, w, 1, D, aux_only=True) as s:
        for k, dtype in enumerate((np.float32, np.float16)):
            C = import_volume_values(h, w, D, dtype, 11 + k)
            for layout in ("hwd", "dhw"):
                for v, variant in enumerate(vr.VARIANTS):
                    src = device_volume(C, layout, dtype, variant)
                    shift = v % 2  # (an unaligned destination too)
                    buf, out = guarded_out(h, w, D, shift)
                    got = s.import_volume(src, 0, layout=layout, out=out)
                    torch.cuda.synchronize(DEV)
                    assert got is out
                    assert np.array_equal(vr.bits(out.cpu().numpy()), vr.bits(C)), (layout, dtype, variant)
                    assert_guards(buf, h * w * D, shift)


@pytest.mark.parametrize("h,w,D", RIGHT_SHAPES)
@pytest.mark.parametrize("scale,m", [(1, 0), (1, 16), (2, 0), (2, 16)])
def test_import_right_is_the_gather(h, w, D, scale, m):
    with SGM(h * scale, w * scale, scale, D, aux_only=True, min_disp=m) as s:
        for k, dtype in enumerate((np.float32, np.float16)):
            C = import_volume_values(h, w, D, dtype, 23 + k)
            want = vr.derive_right(C, m, scale)
            for layout in ("hwd", "dhw"):
                for v, variant in enumerate(vr.VARIANTS):
                    src = device_volume(C, layout, dtype, variant)
                    buf, out = guarded_out(h, w, D, v % 2)
                    s.import_volume(src, 1, layout=layout, out=out)
                    torch.cuda.synchronize(DEV)
                    assert np.array_equal(vr.bits(out.cpu().numpy()), vr.bits(want)), (layout, dtype, variant)
                    assert_guards(buf, h * w * D, v % 2)


@pytest.mark.parametrize("m", [0, 16])
def test_import_right_of_a_census_volume_is_the_right_dsi_where_unclamped(m):
    h, w, D = 24, 80, 32
    ctl, ctr = vr.road_tables(h, w, D)
    with SGM(h, w, 1, D, min_disp=m) as s:
        left = s.stage_cost(ctl, ctr, view=0, filters=0)
        want = s.stage_cost(ctl, ctr, view=1, filters=0)
        got = s.import_volume(torch.tensor(left, device=DEV), 1).cpu().numpy()
    keep = vr.unclamped(w, D, m, 1)
    assert keep.mean() > 0.5
    assert np.array_equal(vr.bits(got)[:, keep], vr.bits(want)[:, keep])
    assert np.array_equal(vr.bits(got), vr.bits(vr.derive_right(left, m, 1)))


# (volume, paths, views, layout, fp16, min_disp)
AGG_CASES = [
    ("road_24x80_D32", 8, 2, "hwd", False, 0),
    ("road_24x80_D32", 8, 2, "dhw", True, 0),
    ("noise_24x80_D32", 8, 2, "dhw", False, 0),
    ("noise_24x80_D32", 4, 2, "hwd", True, 0),
    ("road_24x80_D32", 4, 1, "dhw", False, 0),
    ("road_24x80_D32", 8, 1, "hwd", True, 0),
    ("road_24x80_D32", 8, 2, "dhw", False, 16),
    ("noise_24x80_D32", 4, 2, "hwd", True, 16),
    ("road_20x40_D128", 8, 2, "dhw", True, 0),
    ("noise_20x40_D128", 8, 2, "hwd", False, 0),
    ("noise_20x40_D128", 4, 1, "dhw", True, 0),
    ("road_12x72_D256", 8, 2, "hwd", True, 0),
    ("noise_12x72_D256", 8, 2, "dhw", False, 0),
    ("road_12x72_D256", 4, 2, "dhw", False, 0),
    ("road_24x80_D32_s2", 8, 2, "dhw", True, 0),
    ("road_24x80_D32_s2", 8, 2, "hwd", False, 0),
]


@pytest.mark.parametrize("name,paths,views,layout,f16,m", AGG_CASES)
def test_aggregate_equals_the_recipe(name, paths, views, layout, f16, m):
    _, h, w, D, scale = vr.GPU_VOLUMES[name]
    C = vr.gpu_volume(name, f16)
    e = vr.expected(name, m, paths, f16)
    src = device_volume(C, layout, np.float16 if f16 else np.float32, "batch" if f16 else "padded")
    want = e["lr"] if views == 2 else e["sub"]
    q = rp.camera_q(700.5, 699.25, w / 2 - 0.5, h / 2 + 0.25, 0.12)
    kw = dict(views=views, paths=paths, min_disp=m)
    with SGM(h * scale, w * scale, scale, D, confidence=True, reproject=q, **kw) as s:
        buf = torch.full((h + 2, w + 3), CANARY, dtype=torch.float32, device=DEV)
        out = buf[1:h + 1, :w] if views == 2 else torch.empty((h, w), dtype=torch.float32, device=DEV)
        raw = torch.zeros((h, w), dtype=torch.int16, device=DEV)
        got = s.aggregate(src, layout=layout, out=out, raw=raw)
        s.check()
        g = got.cpu().numpy()
        assert np.array_equal(vr.bits(g), vr.bits(want))
        assert np.array_equal(raw.cpu().numpy().view(np.uint16).astype(np.int64), e["disp"].astype(np.int64))
        assert np.array_equal(vr.bits(s.get_confidence(0)), vr.bits(e["ratio"]))
        if views == 2:
            assert np.array_equal(vr.bits(s.get_confidence(1)), vr.bits(e["ratio_beta"]))
            b = buf.cpu().numpy()
            assert (b[0] == CANARY).all() and (b[-1] == CANARY).all() and (b[:, w:] == CANARY).all()
        else:
            d, f = s.stage_aggregate(C)  # the host path's maps of the same volume
            assert np.array_equal(vr.bits(g), vr.bits(f)) and np.array_equal(d, raw.cpu().numpy().view(np.uint16))
        rw = rp.reproject(want, q, D + m + 1, scale)
        assert np.array_equal(rp.bits(s.get_xyz()), rp.bits(rw["xyz"]))
        assert np.array_equal(rp.bits(s.get_depth()), rp.bits(rw["depth"]))
    if views == 2:
        with SGM(h * scale, w * scale, scale, D, post_filter=True, **kw) as s:
            for budget in (0, 8):
                s.set_post_filter_launches(budget)
                got = s.aggregate(src, layout=layout)
                s.check()
                assert np.array_equal(vr.bits(got.cpu().numpy()), vr.bits(e["final"])), budget


def test_one_view_pitched_map_is_the_dense_one():
    # a views = 1 handle into a padded map: the map is copied out of the handle's own
    name = "noise_24x80_D32"
    _, h, w, D, _ = vr.GPU_VOLUMES[name]
    src = device_volume(vr.gpu_volume(name), "dhw", np.float32, "dense")
    with SGM(h, w, 1, D, views=1) as s:
        buf = torch.full((h + 2, w + 3), CANARY, dtype=torch.float32, device=DEV)
        got = s.aggregate(src, out=buf[1:h + 1, :w])
        s.check()
        assert np.array_equal(vr.bits(got.cpu().numpy()), vr.bits(vr.expected(name)["sub"]))
        b = buf.cpu().numpy()
        assert (b[0] == CANARY).all() and (b[-1] == CANARY).all() and (b[:, w:] == CANARY).all()


@pytest.mark.parametrize("env", [{}, {"SGM_BAND_ROWS": "16"}, {"SGM_BAND_ROWS": "0"}, {"SGM_SLANT": "1"}])
def test_every_schedules_handle_gives_the_same_map(env, monkeypatch):
    for k in ("SGM_BAND_ROWS", "SGM_SLANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "noise_80x240_D256"  # (a size the slanted passes' own tests run)
    _, h, w, D, _ = vr.GPU_VOLUMES[name]
    left, right = vr.road_pair(h, w, D)
    frame = oracle.process(left, right, D, final=False)["lr"]
    src = device_volume(vr.gpu_volume(name), "dhw", np.float32, "dense")
    with SGM(h, w, 1, D) as s:
        s.process(left, right)
        assert np.array_equal(vr.bits(s.get_lr_disp()), vr.bits(frame))
        before = s.device_bytes
        got = s.aggregate(src).cpu().numpy()
        s.check()
        assert np.array_equal(vr.bits(got), vr.bits(vr.expected(name)["lr"]))
        assert s.device_bytes == before
        s.process(left, right)  # the import has not disturbed frame state
        assert np.array_equal(vr.bits(s.get_lr_disp()), vr.bits(frame))


@pytest.mark.timeout(120)
def test_aggregate_replays_from_a_hip_graph():
    names = ["road_24x80_D32", "noise_24x80_D32"]
    _, h, w, D, _ = vr.GPU_VOLUMES[names[0]]
    with SGM(h, w, 1, D, post_filter=True, post_filter_launches=8) as s:
        stream = torch.cuda.ExternalStream(s.stream, device=DEV)
        cost = torch.empty((D, h, w), dtype=torch.float16, device=DEV)
        out = torch.empty((h, w), dtype=torch.float32, device=DEV)

        def load(name):
            with torch.cuda.stream(stream):
                cost.copy_(torch.from_numpy(np.ascontiguousarray(vr.gpu_volume(name, True).transpose(2, 0, 1))))

        load(names[0])
        with torch.cuda.stream(stream):
            s.aggregate(cost, out=out)  # once eagerly before capturing
        torch.cuda.synchronize(DEV)
        s.check()
        before = s.device_bytes
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            s.aggregate(cost, out=out)  # (the current stream is the capture's)
        torch.cuda.synchronize(DEV)
        for name in (names[1], names[0], names[1]):
            load(name)
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize(DEV)
            s.check()
            assert np.array_equal(vr.bits(out.cpu().numpy()), vr.bits(vr.expected(name, 0, 8, True)["final"])), name
            assert s.device_bytes == before


def test_refusals_raise_and_leave_the_map_alone():
    h, w, D = 24, 80, 32
    C = vr.gpu_volume("noise_24x80_D32")
    cost = torch.tensor(C, device=DEV)
    out = torch.full((h, w), CANARY, dtype=torch.float32, device=DEV)
    L = _capi.lib()

    def call(s, vol, d_out=None, pitch=w, stream=None):
        rc = L.sgm_aggregate_device(s._h, ctypes.byref(vol) if vol is not None else None,
                                    ctypes.c_void_p(out.data_ptr() if d_out is None else d_out or None), pitch,
                                    None, ctypes.c_void_p(stream))
        _capi.check(rc, s._h)

    def vol(sr=w * D, sc=D, sd=1, dtype=0, ptr=None):
        return _capi.Volume(cost.data_ptr() if ptr is None else ptr, dtype, sr, sc, sd)

    with SGM(h, w, 1, D) as s:
        bad = [("NULL", lambda: call(s, None)), ("NULL", lambda: call(s, vol(ptr=0))),
               ("d_out", lambda: call(s, vol(), d_out=0)), ("out_pitch", lambda: call(s, vol(), pitch=w - 1)),
               ("dtype", lambda: call(s, vol(dtype=2))), ("both 1", lambda: call(s, vol(sc=1))),
               ("neither", lambda: call(s, vol(sc=2 * D, sd=2, sr=2 * w * D))),
               ("overlapping", lambda: call(s, vol(sr=w * D - 1))), ("negative", lambda: call(s, vol(sr=-w * D))),
               ("hipStreamLegacy", lambda: call(s, vol(), stream=1)),  # (void *)1: the legacy default stream
               ("hipStreamLegacy", lambda: _capi.check(L.sgm_volume_import_device(
                   s._h, ctypes.byref(vol()), 0, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(1)), s._h))]
        for word, f in bad:
            with pytest.raises(SGMError, match=word) as ei:
                f()
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
    for word, make in [("BM", lambda: BM(h, w, 1, D)), ("aux_only", lambda: SGM(h, w, 1, D, aux_only=True)),
                       ("SGM_VIEW_RIGHT", lambda: SGM(h, w, 1, D, views=1, view="right")),
                       ("lk_refine", lambda: SGM(h, w, 1, D, lk_refine=True))]:
        with make() as s:
            with pytest.raises(SGMError, match=word) as ei:
                call(s, vol())
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
    torch.cuda.synchronize(DEV)
    assert (out.cpu().numpy() == CANARY).all()


def test_torch_surface():
    name = "noise_24x80_D32"
    _, h, w, D, _ = vr.GPU_VOLUMES[name]
    C = vr.gpu_volume(name)
    want = vr.expected(name)["lr"]
    with SGM(h, w, 1, D) as s:
        # the default stream is the current torch stream: produced on a side stream just before
        # the call and consumed without a manual sync
        side = torch.cuda.Stream(device=DEV)
        host = torch.tensor(C).pin_memory()
        with torch.cuda.stream(side):
            big = torch.zeros((64, 1024, 1024), device=DEV)
            for _ in range(4):
                big += 1.0  # (keeps the stream busy ahead of the producer)
            cost = (host.to(DEV, non_blocking=True) + big[0, 0, 0] - 4.0).permute(2, 0, 1).contiguous()
            got = s.aggregate(cost)
        side.synchronize()
        assert tuple(got.shape) == (h, w) and got.dtype == torch.float32 and got.device == cost.device
        assert np.array_equal(vr.bits(got.cpu().numpy()), vr.bits(want))
        # a permuted view keeps its strides: (D, H, W) storage seen as (H, W, D)
        got = s.aggregate(cost.permute(1, 2, 0))
        torch.cuda.synchronize(DEV)
        assert np.array_equal(vr.bits(got.cpu().numpy()), vr.bits(want))
        # torch's default stream passed by its handle, 0 (torch.cuda.current_stream().cuda_stream):
        # ordered on it, and the next calls on the handle's own stream work
        fresh = torch.tensor(C, device=DEV)
        got = s.aggregate(fresh, stream=torch.cuda.default_stream(DEV).cuda_stream)
        vol = s.import_volume(fresh, 0, stream=0)
        assert np.array_equal(vr.bits(got.cpu().numpy()), vr.bits(want))
        assert np.array_equal(vr.bits(vol.cpu().numpy()), vr.bits(C))
        s.check()
        assert s.post_filter(got.cpu().numpy()).shape == (h, w)
        with pytest.raises(TypeError, match="stage_aggregate"):
            s.aggregate(C)
        with pytest.raises(ValueError, match="shape"):
            s.aggregate(cost[:, :, :-1])
        with pytest.raises(ValueError, match="layout"):
            s.aggregate(cost, layout="whd")
        with pytest.raises(TypeError, match="float32 or float16"):
            s.aggregate(cost.double())
        with pytest.raises(ValueError, match="device"):
            s.aggregate(cost.cpu())
    with SGM(32, 32, 1, 32) as s:  # rows = cols = D: the shape does not say which axis is which
        cube = torch.zeros((32, 32, 32), device=DEV)
        with pytest.raises(ValueError, match="layout="):
            s.aggregate(cube)
        s.aggregate(cube, layout="dhw")
        s.import_volume(cube, 1, layout="hwd")
        torch.cuda.synchronize(DEV)
