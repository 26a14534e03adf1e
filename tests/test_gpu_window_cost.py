"""The reference's SAD / SSD window costs on the GPU (sgm_window_cost_device,
sgm_set_cost), bit for bit against tests/window_cost_recipe.py:
the producer launch over the shapes that reach every edge of its tiles, frames
on a window cost against `recipe volume -> SGM.aggregate` on a census handle of
the same parameters, a HIP graph replay, the refusals and the way back to the
census."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import gray_recipe
import reproject_recipe as rp
import resize_recipe
import window_cost_cases as cases
import window_cost_recipe as wc
from stereo_matching_amd import BM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 7.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def produce(s, left, right, kind, pad=0):
    """window_cost of host images into a canary-guarded buffer; pad: extra bytes per image row,
    filled with a value the images never hold next to (a pitched input)."""
    h, w = left.shape
    rows, cols, D = s.rows, s.cols, s.max_disp
    imgs = []
    for img in (left, right):
        t = torch.full((h, w + pad), 0xEE, dtype=torch.uint8, device=DEV)
        t[:, :w] = dev(img)
        imgs.append(t[:, :w])
    n = rows * cols * D
    buf = torch.full((n + 128,), CANARY, dtype=torch.float32, device=DEV)
    out = buf[64:64 + n].view(rows, cols, D)
    got = s.window_cost(imgs[0], imgs[1], kind, out=out)
    torch.cuda.synchronize(DEV)
    assert got is out
    b = buf.cpu().numpy()
    assert (b[:64] == CANARY).all() and (b[64 + n:] == CANARY).all()
    return out.cpu().numpy()


# the issue's cases 1-5, 7, 8 and 10, plus min_disp at scale 2
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_producer_equals_the_recipe(name, kind):
    h, w, D, scale, m, _, _ = cases.CASES[name]
    left, right = cases.inputs(name)
    with SGM(h, w, scale, D, aux_only=True, min_disp=m) as s:
        got = produce(s, left, right, kind)
    assert np.array_equal(wc.bits(got), wc.bits(cases.expected(name, kind)))


def test_the_largest_numerator():
    # case 10: all 255 against all 0 under SSD, 63 * 255^2 through both divisions
    left, right = cases.inputs("extreme_10x20_D32")
    with SGM(10, 20, 1, 32, aux_only=True) as s:
        assert (produce(s, left, right, "ssd") == np.float32(65025)).all()


def tile_widths():
    """Case 6: one column more and one column less than the producer's own column tile, and
    than two of them."""
    tj = _capi.lib().sgm_window_cost_tile_cols()
    assert tj >= 8
    return [tj - 1, tj + 1, 2 * tj - 1, 2 * tj + 1]


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("D,scale", [(64, 1), (32, 1), (32, 2)])
@pytest.mark.parametrize("k", range(4))
def test_tile_edges(k, D, scale, kind):
    cols = tile_widths()[k]
    h, w = 18 * scale, cols * scale  # (18 rows: more than one row band at either scale's window)
    left, right = synthetic.stereo_pair(h, w, D, pair_index=20 + k, kind="noise")
    with SGM(h, w, scale, D, aux_only=True) as s:
        got = produce(s, left, right, kind)
    assert np.array_equal(wc.bits(got), wc.bits(wc.volume(left, right, D, kind, scale)))


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("scale", [1, 2])
def test_pitched_input(kind, scale):
    h, w, D = 22 * scale, 70 * scale, 64
    left, right = synthetic.stereo_pair(h, w, D, pair_index=31, kind="road")
    with SGM(h, w, scale, D, aux_only=True) as s:
        got = produce(s, left, right, kind, pad=13)
    assert np.array_equal(wc.bits(got), wc.bits(wc.volume(left, right, D, kind, scale)))


def test_host_twin_and_any_handle_serves():
    name = "edge_24x33_D32"
    h, w, D, _, _, _, _ = cases.CASES[name]
    left, right = cases.inputs(name)
    for kw in (dict(), dict(aux_only=True), dict(views=1, paths=4)):
        with SGM(h, w, 1, D, **kw) as s:
            for kind in wc.KINDS:
                assert np.array_equal(wc.bits(s.stage_window_cost(left, right, kind)),
                                      wc.bits(cases.expected(name, kind)))


# ------------------------------------------------------------------ frames

Q = rp.camera_q(700.5, 699.25, 40.0, 12.5, 0.12)
# what a frame is asked for beyond (views, paths): every map the two handles hold is compared
FRAME_CASES = [
    ("edge_24x33_D32", dict(views=1)),
    ("road_48x170_D64", dict(views=2)),
    ("road_48x170_D64", dict(views=2, paths=4)),
    ("road_48x170_D64", dict(views=1, paths=4)),
    ("road_48x170_D64", dict(views=2, post_filter=True, post_filter_launches=8)),
    ("road_48x170_D64", dict(views=2, confidence=True)),
    ("road_48x170_D64", dict(views=2, reproject=Q)),
    ("m16_48x170_D64", dict(views=2, confidence=True, reproject=Q)),
    ("odd_s2_51x99_D32", dict(views=2)),
    ("narrow_20x40_D128", dict(views=2, post_filter=True, post_filter_launches=8)),
    ("wide_36x300_D256", dict(views=2)),
]


def frame_maps(s, run):
    """The maps a handle holds after `run` enqueued a frame (or an aggregate call) into a map."""
    out = torch.full((s.rows, s.cols), CANARY, dtype=torch.float32, device=DEV)
    raw = torch.zeros((s.rows, s.cols), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize(DEV)
    run(out, raw)
    s.check()
    torch.cuda.synchronize(DEV)
    maps = {"out": out.cpu().numpy(), "raw": raw.cpu().numpy().astype(np.float32)}
    return maps


def extra_maps(s, kw, maps):
    if kw.get("confidence"):
        for v in range(kw["views"]):
            maps[f"ratio{v}"] = s.get_confidence(v)
    if kw.get("reproject") is not None:
        maps["xyz"], maps["depth"] = s.get_xyz(), s.get_depth()
    return maps


def assert_same_maps(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(wc.bits(got[k]), wc.bits(want[k])), k
    assert not (want["out"] == CANARY).all()


def census_handle_maps(volume, h, w, scale, D, m, kw):
    """recipe volume -> SGM.aggregate on a census handle of the same parameters"""
    with SGM(h, w, scale, D, min_disp=m, **kw) as s:
        assert s.cost == "census"
        c = dev(volume)
        maps = frame_maps(s, lambda out, raw: s.aggregate(c, layout="hwd", out=out, raw=raw))
        return extra_maps(s, kw, maps)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name,kw", FRAME_CASES)
def test_frame_equals_recipe_volume_through_aggregate(name, kw, kind):
    h, w, D, scale, m, _, _ = cases.CASES[name]
    left, right = cases.inputs(name)
    want = census_handle_maps(cases.expected(name, kind), h, w, scale, D, m, kw)
    with SGM(h, w, scale, D, min_disp=m, cost=kind, **kw) as s:
        assert s.cost == kind
        dl, dr = dev(left), dev(right)
        before = s.device_bytes
        got = frame_maps(s, lambda out, raw: s.process_device(dl.data_ptr(), dr.data_ptr(), out.data_ptr(),
                                                              d_raw=raw.data_ptr()))
        got = extra_maps(s, kw, got)
        assert s.device_bytes == before
        assert_same_maps(got, want)
        # the host API's frame gives the same map
        s.process(left, right)
        host = s.get_disp() if kw.get("post_filter") else s.get_lr_disp()
        assert np.array_equal(wc.bits(host), wc.bits(want["out"]))


@pytest.mark.parametrize("kind", wc.KINDS)
def test_frame_behind_an_input_size(kind):
    h, w, D = 24, 80, 32
    src = [resize_recipe.random_image(37, 101, 5 + v) for v in (0, 1)]
    left, right = (resize_recipe.resize(x, h, w) for x in src)
    kw = dict(views=2)
    want = census_handle_maps(wc.volume(left, right, D, kind), h, w, 1, D, 0, kw)
    with SGM(h, w, 1, D, cost=kind, input_size=(37, 101), **kw) as s:
        s.process(src[0], src[1])
        assert np.array_equal(s.get_resized(0), left) and np.array_equal(s.get_resized(1), right)
        assert np.array_equal(wc.bits(s.get_lr_disp()), wc.bits(want["out"]))


@pytest.mark.parametrize("kind", wc.KINDS)
def test_frame_behind_a_colour_format(kind):
    h, w, D = 24, 80, 32
    src = [gray_recipe.random_image(h, w, 3, 9 + v) for v in (0, 1)]
    left, right = (gray_recipe.gray(x, "bgr8") for x in src)
    kw = dict(views=2)
    want = census_handle_maps(wc.volume(left, right, D, kind), h, w, 1, D, 0, kw)
    with SGM(h, w, 1, D, cost=kind, input_format="bgr8", **kw) as s:
        s.process(src[0], src[1])
        assert np.array_equal(wc.bits(s.get_lr_disp()), wc.bits(want["out"]))


def test_lk_refine_is_allowed_on_a_window_cost_frame():
    # the frame has images: post_filter + LKRefine after the shared tail, as the side stage runs it
    h, w, D = 48, 170, 64
    left, right = cases.inputs("road_48x170_D64")
    want = census_handle_maps(cases.expected("road_48x170_D64", "sad"), h, w, 1, D, 0, dict(views=2))["out"]
    with SGM(h, w, 1, D, cost="sad", lk_refine=True) as s, SGM(h, w, 1, D, aux_only=True) as aux:
        s.process(left, right)
        assert np.array_equal(wc.bits(s.get_disp()), wc.bits(aux.lk_refine(left, right, want)))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", wc.KINDS)
def test_frame_replays_from_a_hip_graph(kind):
    h, w, D = 48, 170, 64
    with SGM(h, w, 1, D, cost=kind, post_filter=True, post_filter_launches=8) as s:
        stream = torch.cuda.ExternalStream(s.stream, device=DEV)
        d_l = torch.empty((h, w), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_e = torch.empty((h, w), dtype=torch.float32, device=DEV)
        out_g = torch.empty_like(out_e)

        def frame(out):
            s.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)

        def load(k):
            left, right = synthetic.stereo_pair(h, w, D, pair_index=k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))

        load(0)
        with torch.cuda.stream(stream):
            frame(out_e)  # once eagerly before capturing
        torch.cuda.synchronize(DEV)
        s.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(out_g)
        torch.cuda.synchronize(DEV)
        for k in (1, 2):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
                frame(out_e)
            torch.cuda.synchronize(DEV)
            s.check()
            assert np.array_equal(wc.bits(out_g.cpu().numpy()), wc.bits(out_e.cpu().numpy())), k
        # (and the eager frame is the recipe's: the last pair's volume through a census handle)
        left, right = synthetic.stereo_pair(h, w, D, pair_index=2)
        want = census_handle_maps(wc.volume(left, right, D, kind), h, w, 1, D, 0,
                                  dict(views=2, post_filter=True, post_filter_launches=8))
        assert np.array_equal(wc.bits(out_g.cpu().numpy()), wc.bits(want["out"]))


def test_window_cost_is_capturable_and_feeds_aggregate():
    # the round trip as two calls: window_cost -> aggregate equals the frame
    name, kind = "road_48x170_D64", "ssd"
    h, w, D = 48, 170, 64
    left, right = cases.inputs(name)
    with SGM(h, w, 1, D) as s, SGM(h, w, 1, D, cost=kind) as f:
        stream = torch.cuda.ExternalStream(s.stream, device=DEV)
        dl, dr = dev(left), dev(right)
        vol = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize(DEV)
        with torch.cuda.stream(stream):
            s.window_cost(dl, dr, kind, out=vol)
        torch.cuda.synchronize(DEV)
        vol.zero_()
        torch.cuda.synchronize(DEV)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            s.window_cost(dl, dr, kind, out=vol)
        torch.cuda.synchronize(DEV)
        assert (vol.cpu().numpy() == 0).all()  # (captured, not run)
        with torch.cuda.stream(stream):
            graph.replay()
            got = s.aggregate(vol)
        torch.cuda.synchronize(DEV)
        s.check()
        assert np.array_equal(wc.bits(vol.cpu().numpy()), wc.bits(cases.expected(name, kind)))
        f.process(left, right)
        assert np.array_equal(wc.bits(got.cpu().numpy()), wc.bits(f.get_lr_disp()))


# ---------------------------------------------------------------- refusals

def test_refusals():
    h, w, D = 24, 80, 32
    L = _capi.lib()
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    mask = synthetic.sky_mask(h, w)
    dl, dr, dm = dev(left), dev(right), dev(mask)
    out = torch.full((h, w), CANARY, dtype=torch.float32, device=DEV)
    vol = torch.full((h, w, D), CANARY, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(h, w, 1, D, cost="sad") as s:
        # a non-NULL mask on a frame call, device and host
        for kw in (dict(d_sky_l=dm.data_ptr()), dict(d_sky_r=dm.data_ptr())):
            with pytest.raises(SGMError, match="sky masks") as ei:
                s.process_device(dl.data_ptr(), dr.data_ptr(), out.data_ptr(), **kw)
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
        with pytest.raises(SGMError, match="sky masks"):
            s.process(left, right, mask)
        with pytest.raises(SGMError, match="sky masks"):
            s.process(left, right, None, mask)
        # a bad kind
        for k in (3, -1):
            rc = L.sgm_set_cost(s._h, k)
            assert rc == _capi.SGM_ERR_INVALID_ARG and b"kind" in L.sgm_last_error(s._h)
        assert s.cost == "sad"
        with pytest.raises(ValueError, match="cost"):
            s.set_cost("mi")

        def call(kind=1, l=dl.data_ptr(), r=dr.data_ptr(), pitch=w, dst=vol.data_ptr(), stream=None):
            _capi.check(L.sgm_window_cost_device(s._h, kind, ctypes.c_void_p(l), ctypes.c_void_p(r), pitch,
                                                 ctypes.c_void_p(dst), ctypes.c_void_p(stream)), s._h)

        for word, f in [("kind", lambda: call(kind=0)), ("kind", lambda: call(kind=3)),
                        ("NULL image", lambda: call(l=None)), ("NULL image", lambda: call(r=None)),
                        ("pitch", lambda: call(pitch=w - 1)), ("d_dst", lambda: call(dst=None)),
                        ("float pointer", lambda: call(dst=vol.data_ptr() + 2)),
                        ("hipStreamLegacy", lambda: call(stream=1))]:  # (void *)1: the legacy default stream
            with pytest.raises(SGMError, match=word) as ei:
                f()
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
    for word, make in [("BM", lambda: BM(h, w, 1, D)), ("aux_only", lambda: SGM(h, w, 1, D, aux_only=True)),
                       ("SGM_VIEW_RIGHT", lambda: SGM(h, w, 1, D, views=1, view="right")),
                       ("sky_detect", lambda: SGM(h, w, 1, D, sky_detect=True))]:
        with make() as s:
            with pytest.raises(SGMError, match=word) as ei:
                s.set_cost("sad")
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
            assert s.cost == "census"
    with pytest.raises(SGMError, match="sky_detect"):
        SGM(h, w, 1, D, sky_detect=True, cost="ssd")
    with pytest.raises(ValueError, match="cost"):
        SGM(h, w, 1, D, cost="mi")
    torch.cuda.synchronize(DEV)
    assert (out.cpu().numpy() == CANARY).all() and (vol.cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("views", [1, 2])
def test_back_to_the_census_equals_a_fresh_handle(views):
    h, w, D = 48, 170, 64
    left, right = cases.inputs("road_48x170_D64")
    mask = synthetic.sky_mask(h, w)
    kw = dict(views=views, confidence=True)
    with SGM(h, w, 1, D, **kw) as fresh:
        fresh.process(left, right, mask, mask if views == 2 else None)
        want = {"lr": fresh.get_lr_disp().copy(), "raw": fresh.get_raw_disp().copy(),
                "ratio": fresh.get_confidence(0)}
    with SGM(h, w, 1, D, **kw) as s:
        s.set_cost("sad")
        s.process(left, right)
        sad = s.get_lr_disp().copy()
        s.set_cost("census")
        assert s.cost == "census"
        s.process(left, right, mask, mask if views == 2 else None)
        assert np.array_equal(wc.bits(s.get_lr_disp()), wc.bits(want["lr"]))
        assert np.array_equal(s.get_raw_disp(), want["raw"])
        assert np.array_equal(wc.bits(s.get_confidence(0)), wc.bits(want["ratio"]))
        assert not np.array_equal(wc.bits(sad), wc.bits(want["lr"]))
