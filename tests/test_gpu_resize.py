"""The input resize on the GPU (sgm_resize_device / sgm_stage_resize /
sgm_set_input_size), bit-exact against tests/resize_recipe.py:
the stand-alone call over every path of the kernel (half size, general, border
clamps, identity, the node's own sizes; dense and padded buffers; aux_only and
full handles), then frames: an input_size handle fed raw images equals a plain
handle fed recipe(raw), for every kind of handle, through the device entry
point, replayed from a HIP graph, and switched off again."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import resize_recipe as rr
from support import bits
from stereo_matching_amd import BM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 0xA5
# (source rows, cols) -> (destination rows, cols)
SHAPES = [
    ((37, 53), (24, 80)),        # down in y, up in x
    ((24, 80), (24, 80)),        # identity
    ((48, 160), (24, 80)),       # the half-size path
    ((48, 161), (24, 80)),       # half in y only: the general path
    ((49, 160), (24, 80)),       # half in x only
    ((90, 250), (24, 80)),       # more than 2x down: pixels are skipped, not averaged
    ((1, 1), (24, 80)),          # the smallest source: every border clamp
    ((2, 3), (24, 80)),          # ... and with one interior interval per axis
    ((375, 1242), (360, 1240)),  # the node's own sizes
]
IDS = [f"{s[0]}x{s[1]}_to_{d[0]}x{d[1]}" for s, d in SHAPES]


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def sources(sh, sw):
    return [rr.random_image(sh, sw, 11 + sh + sw), rr.fit(rr.kitti_crop()[40:, 300:], sh, sw)]


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(dst, aux):
        key = (dst, aux)
        if key not in made:
            made[key] = SGM(dst[0], dst[1], 1, 32, aux_only=aux)
        return made[key]

    yield get
    for s in made.values():
        s.close()


def padded(img, pitch, device=False):
    buf = np.full((img.shape[0], pitch), SENTINEL, np.uint8)
    buf[:, : img.shape[1]] = img
    return torch.from_numpy(buf).to(DEV) if device else buf


@pytest.mark.parametrize("aux", [True, False], ids=["aux_only", "full"])
@pytest.mark.parametrize("src_shape,dst_shape", SHAPES, ids=IDS)
def test_resize_matches_the_recipe(handles, src_shape, dst_shape, aux):
    sgm = handles(dst_shape, aux)
    (sh, sw), (dh, dw) = src_shape, dst_shape
    for img in sources(sh, sw):
        want = rr.resize(img, dh, dw)
        # host buffers: dense, then a padded source
        assert np.array_equal(sgm.resize(img), want)
        out = np.empty((dh, dw), np.uint8)
        host = padded(img, sw + 5)
        _capi.check(sgm._lib.sgm_stage_resize(sgm._h, _p(host), sh, sw, sw + 5, _p(out)), sgm._h)
        assert np.array_equal(host, padded(img, sw + 5))
        assert np.array_equal(out, want)
        # device buffers: dense, then padded on both sides; the padding survives
        for sp, dp in ((sw, dw), (sw + 11, dw + 7)):
            d_src = padded(img, sp, device=True)
            d_dst = torch.full((dh, dp), SENTINEL, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize(DEV)          # (the handle's stream is not ordered with torch's)
            sgm.resize_device(d_src.data_ptr(), sh, sw, d_dst.data_ptr(), src_pitch=sp, dst_pitch=dp)
            sgm.check()
            got = d_dst.cpu().numpy()
            assert np.array_equal(got[:, :dw], want), (sp, dp)
            assert (got[:, dw:] == SENTINEL).all()
            assert np.array_equal(d_src.cpu().numpy(), padded(img, sp))


# ------------------------------------------------------------------ frames

FRAME = (24, 80, 32)   # working rows, cols, D
RAW_SHAPES = [(37, 53), (48, 160)]
VARIANTS = {
    "views2": dict(views=2),
    "left": dict(views=1),
    "right": dict(views=1, view="right"),
    "scale2": dict(views=2, s=2),
    "paths4": dict(views=2, paths=4),
    "min_disp8": dict(views=2, min_disp=8),
    "bm": dict(cls=BM),
    "config5": dict(views=2, sky_detect=True, post_filter=True, lk_refine=True, post_filter_launches=8),
}


def make(variant, input_size=None):
    kw = dict(VARIANTS[variant])
    cls = kw.pop("cls", SGM)
    s = kw.pop("s", 1)
    H, W, D = FRAME
    if cls is SGM:
        kw["confidence"] = True
    return cls(H * s, W * s, s, D, input_size=input_size, **kw)


def raw_pair(shape, k=0):
    return synthetic.stereo_pair(shape[0], shape[1], 32, pair_index=5 + k, kind="road")


def frame_maps(sgm, left, right):
    sgm.process(left, right)
    m = {"out": sgm.get_disp() if sgm.params.post_filter or sgm.params.lk_refine else sgm.get_lr_disp(),
         "raw": sgm.get_raw_disp()}
    if sgm.params.solver == _capi.SGM_SOLVER_SGM:
        m["conf"] = sgm.get_confidence(1 if sgm.params.view == _capi.SGM_VIEW_RIGHT else 0)
        if sgm.params.views == 2:
            m["conf_r"] = sgm.get_confidence(1)
    return m


@pytest.mark.parametrize("raw_shape", RAW_SHAPES, ids=["37x53", "48x160"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_input_size_frame_equals_plain_frame_of_the_recipe(variant, raw_shape):
    left, right = raw_pair(raw_shape)
    with make(variant, raw_shape) as sized, make(variant) as plain:
        assert sized.input_size == raw_shape and plain.input_size == (0, 0)
        rl, rr_ = rr.resize(left, plain.h, plain.w), rr.resize(right, plain.h, plain.w)
        got, want = frame_maps(sized, left, right), frame_maps(plain, rl, rr_)
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), k
        assert np.array_equal(sized.get_resized(0), rl)
        assert np.array_equal(sized.get_resized(1), rr_)
        if raw_shape != (plain.h, plain.w):      # a full-size image is now the wrong size
            with pytest.raises(ValueError):
                sized.process(rl, rr_)


def test_device_entry_point_with_pitched_raw_images():
    H, W, D = FRAME
    sh, sw = RAW_SHAPES[0]
    left, right = raw_pair((sh, sw))
    pitch = sw + 19
    d_l, d_r = padded(left, pitch, device=True), padded(right, pitch, device=True)
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    raw = torch.zeros((H, W), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize(DEV)                  # (the handle's stream is not ordered with torch's)
    with SGM(H, W, 1, D, input_size=(sh, sw)) as sized, SGM(H, W, 1, D) as plain:
        with pytest.raises(SGMError):            # a pitch below the raw width
            sized.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), pitch=sw - 1)
        sized.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), pitch=pitch, d_raw=raw.data_ptr())
        sized.check()
        # the handle-owned resized image, read on the device
        ptr, rp = ctypes.c_void_p(), ctypes.c_int()
        _capi.check(sized._lib.sgm_get_resized(sized._h, 0, ctypes.byref(ptr), ctypes.byref(rp)), sized._h)
        assert ptr.value and rp.value == W
        assert np.array_equal(sized.get_resized(0), rr.resize(left, H, W))
        plain.process(rr.resize(left, H, W), rr.resize(right, H, W))
        assert np.array_equal(bits(out.cpu().numpy()), bits(plain.get_lr_disp()))
        assert np.array_equal(raw.cpu().numpy().view(np.uint16), plain.get_raw_disp())
    assert (d_l.cpu().numpy()[:, sw:] == SENTINEL).all()


@pytest.mark.timeout(120)
def test_input_size_frame_replays_from_a_hip_graph():
    H, W, D = FRAME
    sh, sw = RAW_SHAPES[0]
    with SGM(H, W, 1, D, input_size=(sh, sw)) as sgm, SGM(H, W, 1, D) as plain:
        stream = torch.cuda.ExternalStream(sgm.stream, device=DEV)
        d_l = torch.empty((sh, sw), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_g = torch.empty((H, W), dtype=torch.float32, device=DEV)

        def frame(st):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out_g.data_ptr(), stream=st)

        def load(k):
            left, right = raw_pair((sh, sw), k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))
            return left, right

        load(0)
        with torch.cuda.stream(stream):
            frame(stream.cuda_stream)  # warm-up (the capture needs no first-call work)
        torch.cuda.synchronize(DEV)
        sgm.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(stream.cuda_stream)
        torch.cuda.synchronize(DEV)
        for k in (1, 2):
            left, right = load(k)
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize(DEV)
            sgm.check()
            plain.process(rr.resize(left, H, W), rr.resize(right, H, W))
            assert np.array_equal(bits(out_g.cpu().numpy()), bits(plain.get_lr_disp())), k
            assert np.array_equal(sgm.get_resized(1), rr.resize(right, H, W)), k


def test_switching_the_input_size_off_restores_the_handle():
    H, W, D = FRAME
    left, right = synthetic.stereo_pair(H, W, D, pair_index=2, kind="road")
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D) as plain:
        before = sgm.device_bytes
        sgm.set_input_size(37, 53)
        assert sgm.device_bytes == before + 2 * H * W + 2 * 37 * 53
        sgm.set_input_size(90, 250)              # another size: the staging is re-allocated
        assert sgm.device_bytes == before + 2 * H * W + 2 * 90 * 250
        sgm.process(*raw_pair((90, 250)))
        sgm.set_input_size(0, 0)
        assert sgm.device_bytes == before == plain.device_bytes and sgm.input_size == (0, 0)
        sgm.process(left, right)
        plain.process(left, right)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(plain.get_lr_disp()))
        assert np.array_equal(sgm.get_raw_disp(), plain.get_raw_disp())
        with pytest.raises(SGMError, match="no input size"):
            sgm.get_resized(0)


def test_errors():
    H, W, D = FRAME
    img = rr.random_image(37, 53, 3)
    d_src = torch.from_numpy(img).to(DEV)
    d_dst = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D, aux_only=True) as aux:
        for rows, cols in ((-1, 53), (37, -1), (-1, -1), (0, 53), (37, 0)):
            with pytest.raises(SGMError, match="sgm_set_input_size") as e:
                sgm.set_input_size(rows, cols)
            assert e.value.code == _capi.SGM_ERR_INVALID_ARG
        assert sgm.input_size == (0, 0)
        with pytest.raises(SGMError, match="aux_only"):
            aux.set_input_size(37, 53)
        for s in (sgm, aux):
            with pytest.raises(SGMError, match="src_pitch"):      # src_pitch < src_cols
                s.resize_device(d_src.data_ptr(), 37, 53, d_dst.data_ptr(), src_pitch=52)
            with pytest.raises(SGMError, match="src_pitch"):
                s.resize(img, pitch=52)
            with pytest.raises(SGMError, match="dst_pitch"):
                s.resize_device(d_src.data_ptr(), 37, 53, d_dst.data_ptr(), dst_pitch=W - 1)
            for rows, cols in ((0, 53), (37, 0), (-3, 53)):
                with pytest.raises(SGMError, match="source size"):
                    s.resize_device(d_src.data_ptr(), rows, cols, d_dst.data_ptr(), src_pitch=64)
            with pytest.raises(SGMError, match="NULL"):
                s.resize_device(0, 37, 53, d_dst.data_ptr())
            with pytest.raises(SGMError, match="NULL"):
                s.resize_device(d_src.data_ptr(), 37, 53, 0)
            with pytest.raises(SGMError, match="NULL"):
                _capi.check(s._lib.sgm_stage_resize(s._h, None, 37, 53, 53, _p(img)), s._h)
            with pytest.raises(SGMError, match="NULL"):
                _capi.check(s._lib.sgm_stage_resize(s._h, _p(img), 37, 53, 53, None), s._h)
        # sgm_get_resized: no input size; before any frame; a view that is neither image
        with pytest.raises(SGMError, match="no input size"):
            sgm.get_resized(0)
        sgm.set_input_size(37, 53)
        with pytest.raises(SGMError, match="no frame"):
            sgm.get_resized(0)
        sgm.process(*raw_pair((37, 53)))
        assert sgm.get_resized(0).shape == (H, W)
        for view in (2, -1):
            with pytest.raises(SGMError, match="view"):
                sgm.get_resized(view)
        ptr, rp = ctypes.c_void_p(), ctypes.c_int()
        assert sgm._lib.sgm_get_resized(sgm._h, 0, None, ctypes.byref(rp)) == _capi.SGM_ERR_INVALID_ARG
        assert sgm._lib.sgm_get_resized(sgm._h, 0, ctypes.byref(ptr), None) == _capi.SGM_ERR_INVALID_ARG
        sgm.set_input_size(40, 60)               # a new size: the old frame's image is gone
        with pytest.raises(SGMError, match="no frame"):
            sgm.get_resized(0)
