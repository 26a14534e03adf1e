"""Rectification on the GPU (sgm_set_rectify / sgm_remap_device /
sgm_stage_remap), bit-exact against tests/rectify_recipe.py over
every pixel: the stand-alone call over sources from 1 x 1, dense and padded
buffers, both views, aux_only and full handles and a part-filled workgroup in x
and y; then frames: a handle with maps set, fed raw images, equals a plain
handle fed recipe(raw), for every kind of handle, through the device entry
point, replayed from a HIP graph, with the maps replaced and switched off
again; every error; the valid mask."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import rectify_recipe as rc
from support import bits
from stereo_matching_amd import BM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 0xA5
SOURCES = [(1, 1), (2, 3), (37, 53), (129, 200)]
HANDLES = [(24, 80), (17, 65), (360, 1240)]    # (17 x 65: a part-filled workgroup in x and in y)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def rig(h, w, sh, sw):
    """(src_h, src_w, mapx_l, mapy_l, mapx_r, mapy_r): the generator's maps of both views."""
    return (sh, sw, *rc.maps(h, w, sh, sw, 0), *rc.maps(h, w, sh, sw, 1))


def padded(img, pitch, device=False):
    buf = np.full((img.shape[0], pitch), SENTINEL, np.uint8)
    buf[:, : img.shape[1]] = img
    return torch.from_numpy(buf).to(DEV) if device else buf


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


@pytest.mark.parametrize("aux", [True, False], ids=["aux_only", "full"])
@pytest.mark.parametrize("dst_shape", HANDLES, ids=[f"to_{h}x{w}" for h, w in HANDLES])
@pytest.mark.parametrize("src_shape", SOURCES, ids=[f"{h}x{w}" for h, w in SOURCES])
def test_remap_matches_the_recipe(handles, src_shape, dst_shape, aux):
    sgm = handles(dst_shape, aux)
    (sh, sw), (dh, dw) = src_shape, dst_shape
    r = rig(dh, dw, sh, sw)
    sgm.set_rectify(*r)
    assert sgm.rectify_size == (sh, sw)
    img = rc.random_image(sh, sw, 11 + sh + sw)
    for view in (0, 1):
        mx, my = r[2 + 2 * view], r[3 + 2 * view]
        want = rc.remap(img, mx, my)
        assert np.array_equal(sgm.rectify_valid(view), rc.convert(mx, my, sh, sw)[4])
        # host buffers: dense, then a padded source
        assert np.array_equal(sgm.remap(img, view), want)
        host = padded(img, sw + 5)
        assert np.array_equal(sgm.remap(host, view, pitch=sw + 5), want)
        assert np.array_equal(host, padded(img, sw + 5))
        # device buffers: dense, then padded on both sides; the padding survives
        for sp, dp in ((sw, dw), (sw + 11, dw + 7)):
            d_src = padded(img, sp, device=True)
            d_dst = torch.full((dh, dp), SENTINEL, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize(DEV)          # (the handle's stream is not ordered with torch's)
            sgm.remap_device(d_src.data_ptr(), d_dst.data_ptr(), view, src_pitch=sp, dst_pitch=dp)
            sgm.check()
            got = d_dst.cpu().numpy()
            assert np.array_equal(got[:, :dw], want), (view, sp, dp)
            assert (got[:, dw:] == SENTINEL).all()
            assert np.array_equal(d_src.cpu().numpy(), padded(img, sp))


def test_identity_maps_return_the_source():
    # (the last column's and row's second taps lie past the image: weight 0, never loaded)
    h, w = 24, 80
    mx, my = rc.identity_maps(h, w)
    img = rc.random_image(h, w, 5)
    d_src = torch.from_numpy(img).to(DEV)
    d_dst = torch.zeros((h, w), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(h, w, 1, 32, aux_only=True, rectify=(h, w, mx, my, mx, my)) as sgm:
        sgm.remap_device(d_src.data_ptr(), d_dst.data_ptr(), 1)
        sgm.check()
        assert np.array_equal(d_dst.cpu().numpy(), img)
        assert np.array_equal(sgm.remap(img, 0), img)


# ------------------------------------------------------------------ frames

FRAME = (24, 80, 32)   # working rows, cols, D
RAW = (37, 53)
VARIANTS = {
    "views2": dict(views=2),
    "left": dict(views=1),
    "right": dict(views=1, view="right"),
    "paths4": dict(views=2, paths=4),
    "min_disp8": dict(views=2, min_disp=8),
    "config5": dict(views=2, sky_detect=True, post_filter=True, lk_refine=True, post_filter_launches=8),
    "bm": dict(cls=BM),
}


def make(variant, rectify=None):
    kw = dict(VARIANTS[variant])
    cls = kw.pop("cls", SGM)
    H, W, D = FRAME
    if cls is SGM:
        kw["confidence"] = True
    return cls(H, W, 1, D, rectify=rectify, **kw)


def raw_pair(shape=RAW, k=0):
    return synthetic.stereo_pair(shape[0], shape[1], 32, pair_index=5 + k, kind="road")


def recipe_pair(r, left, right):
    return rc.remap(left, r[2], r[3]), rc.remap(right, r[4], r[5])


def frame_maps(sgm, left, right):
    sgm.process(left, right)
    m = {"out": sgm.get_disp() if sgm.params.post_filter or sgm.params.lk_refine else sgm.get_lr_disp(),
         "raw": sgm.get_raw_disp()}
    if sgm.params.solver == _capi.SGM_SOLVER_SGM:
        m["conf"] = sgm.get_confidence(1 if sgm.params.view == _capi.SGM_VIEW_RIGHT else 0)
        if sgm.params.views == 2:
            m["conf_r"] = sgm.get_confidence(1)
    return m


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rectify_frame_equals_plain_frame_of_the_recipe(variant):
    H, W, _ = FRAME
    r = rig(H, W, *RAW)
    left, right = raw_pair()
    rl, rr = recipe_pair(r, left, right)
    with make(variant, r) as rect, make(variant) as plain:
        assert rect.rectify_size == RAW and plain.rectify_size == (0, 0)
        got, want = frame_maps(rect, left, right), frame_maps(plain, rl, rr)
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), k
        assert np.array_equal(rect.rectified(0), rl)
        assert np.array_equal(rect.rectified(1), rr)
        with pytest.raises(ValueError):          # a full-size image is now the wrong size
            rect.process(rl, rr)


def test_side_by_side_frame_through_the_device_entry_point():
    # one raw side-by-side camera frame split by pitch, on a caller's stream
    H, W, D = FRAME
    sh, sw = RAW
    r = rig(H, W, sh, sw)
    left, right = raw_pair()
    pitch = 2 * sw + 13
    frame = padded(np.hstack([left, right]), pitch, device=True)
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    raw = torch.zeros((H, W), dtype=torch.int16, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(H, W, 1, D, rectify=r) as rect, SGM(H, W, 1, D) as plain:
        with pytest.raises(SGMError):            # a pitch below the raw width
            rect.process_device(frame.data_ptr(), frame.data_ptr() + sw, out.data_ptr(), pitch=sw - 1)
        rect.process_device(frame.data_ptr(), frame.data_ptr() + sw, out.data_ptr(), pitch=pitch,
                            d_raw=raw.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        rect.check()
        rl, rr = recipe_pair(r, left, right)
        # the handle-owned rectified image, read on the device
        ptr, rp = ctypes.c_void_p(), ctypes.c_int()
        _capi.check(rect._lib.sgm_get_rectified(rect._h, 0, ctypes.byref(ptr), ctypes.byref(rp)), rect._h)
        assert ptr.value and rp.value == W
        assert np.array_equal(rect.rectified(0), rl) and np.array_equal(rect.rectified(1), rr)
        plain.process(rl, rr)
        assert np.array_equal(bits(out.cpu().numpy()), bits(plain.get_lr_disp()))
        assert np.array_equal(raw.cpu().numpy().view(np.uint16), plain.get_raw_disp())
    assert (frame.cpu().numpy()[:, 2 * sw:] == SENTINEL).all()


@pytest.mark.timeout(120)
def test_rectify_frame_with_a_fill_budget_replays_from_a_hip_graph():
    H, W, D = FRAME
    sh, sw = RAW
    r = rig(H, W, sh, sw)
    kw = dict(post_filter=True, post_filter_launches=8)
    with SGM(H, W, 1, D, rectify=r, **kw) as sgm, SGM(H, W, 1, D, **kw) as plain:
        stream = torch.cuda.ExternalStream(sgm.stream, device=DEV)
        d_l = torch.empty((sh, sw), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_g = torch.empty((H, W), dtype=torch.float32, device=DEV)
        out_e = torch.empty_like(out_g)

        def frame(st, out):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=st)

        def load(k):
            left, right = raw_pair(RAW, k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))
            return left, right

        load(0)
        with torch.cuda.stream(stream):
            frame(stream.cuda_stream, out_g)  # warm-up (the capture needs no first-call work)
        torch.cuda.synchronize(DEV)
        sgm.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(stream.cuda_stream, out_g)
        torch.cuda.synchronize(DEV)
        for k in (1, 2):
            left, right = load(k)
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize(DEV)
            sgm.check()
            with torch.cuda.stream(stream):
                frame(stream.cuda_stream, out_e)     # the eager frame on the same images
            torch.cuda.synchronize(DEV)
            sgm.check()
            assert np.array_equal(bits(out_g.cpu().numpy()), bits(out_e.cpu().numpy())), k
            rl, rr = recipe_pair(r, left, right)
            plain.process(rl, rr)
            assert np.array_equal(bits(out_g.cpu().numpy()), bits(plain.get_disp())), k
            assert np.array_equal(sgm.rectified(1), rr), k


def test_replacing_the_maps_and_switching_them_off_restores_the_handle():
    H, W, D = FRAME
    left, right = synthetic.stereo_pair(H, W, D, pair_index=2, kind="road")
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D) as plain, SGM(H, W, 1, D, aux_only=True) as aux:
        before, aux_before = sgm.device_bytes, aux.device_bytes
        sgm.set_rectify(*rig(H, W, 37, 53))
        # two packed maps of 8 B per pixel, two rectified images, two staged raw images
        assert sgm.device_bytes == before + 2 * 8 * H * W + 2 * H * W + 2 * 37 * 53
        aux.set_rectify(*rig(H, W, 37, 53))      # (it runs no frames: the maps alone)
        assert aux.device_bytes == aux_before + 2 * 8 * H * W
        r2 = rig(H, W, 129, 200)                 # other maps of another source: replaced
        sgm.set_rectify(*r2)
        assert sgm.device_bytes == before + 2 * 8 * H * W + 2 * H * W + 2 * 129 * 200
        with pytest.raises(SGMError, match="no frame"):
            sgm.rectified(0)
        l2, rt2 = raw_pair((129, 200))
        sgm.process(l2, rt2)
        rl, rr = recipe_pair(r2, l2, rt2)
        assert np.array_equal(sgm.rectified(0), rl) and np.array_equal(sgm.rectified(1), rr)
        plain.process(rl, rr)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(plain.get_lr_disp()))
        r3 = (129, 200, r2[4], r2[5], r2[2], r2[3])          # same source size, the views' maps swapped
        sgm.set_rectify(*r3)
        assert np.array_equal(sgm.remap(l2, 0), rc.remap(l2, r2[4], r2[5]))
        for s, b in ((sgm, before), (aux, aux_before)):
            s.set_rectify(0, 0)
            assert s.device_bytes == b and s.rectify_size == (0, 0)
            s.set_rectify(0, 0)                  # off twice is off
        assert sgm.device_bytes == plain.device_bytes
        sgm.process(left, right)
        plain.process(left, right)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(plain.get_lr_disp()))
        assert np.array_equal(sgm.get_raw_disp(), plain.get_raw_disp())
        with pytest.raises(SGMError, match="no maps"):
            sgm.rectified(0)
        sgm.set_input_size(37, 53)               # the other input stage is free again
        sgm.set_input_size(0, 0)


def test_switching_the_inactive_stage_off_changes_nothing():
    # the class layer keeps taking the active stage's images: a raw frame after the no-op call equals the
    # plain frame of the recipe, a full-size image stays the wrong size, and the device entry point's
    # default pitch stays the raw width
    import resize_recipe as rr
    H, W, D = FRAME
    r = rig(H, W, *RAW)
    left, right = raw_pair()
    d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D) as plain:
        for stage, off_other, want_pair in (
                (lambda: sgm.set_rectify(*r), lambda: sgm.set_input_size(0, 0), recipe_pair(r, left, right)),
                (lambda: sgm.set_input_size(*RAW), lambda: sgm.set_rectify(0, 0),
                 (rr.resize(left, H, W), rr.resize(right, H, W)))):
            stage()
            off_other()
            assert (sgm.in_h, sgm.in_w) == RAW
            plain.process(*want_pair)
            sgm.process(left, right)
            assert np.array_equal(bits(sgm.get_lr_disp()), bits(plain.get_lr_disp()))
            assert np.array_equal(sgm.get_raw_disp(), plain.get_raw_disp())
            with pytest.raises(ValueError):
                sgm.process(*want_pair)
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr())     # (default pitch)
            sgm.check()
            assert np.array_equal(bits(out.cpu().numpy()), bits(plain.get_lr_disp()))
            sgm.set_rectify(0, 0)
            sgm.set_input_size(0, 0)
            assert (sgm.in_h, sgm.in_w) == (H, W)


def test_errors():
    H, W, D = FRAME
    sh, sw = RAW
    r = rig(H, W, sh, sw)
    img = rc.random_image(sh, sw, 3)
    d_src = torch.from_numpy(img).to(DEV)
    d_dst = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    out = np.empty((H, W), np.uint8)
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D, aux_only=True) as aux:
        for s in (sgm, aux):
            L, h = s._lib, s._h
            m = [_p(a) for a in r[2:]]

            def refused(rc_, what):
                assert rc_ == _capi.SGM_ERR_INVALID_ARG
                msg = L.sgm_last_error(h).decode()
                assert what in msg, msg

            # sgm_set_rectify: sizes, maps, pitch
            for rows, cols in ((-1, sw), (sh, -1), (32768, sw), (sh, 32768), (0, 0)):   # (0, 0) with maps
                refused(L.sgm_set_rectify(h, rows, cols, *m, W), "source sizes must be in")
            for rows, cols in ((0, sw), (sh, 0)):
                refused(L.sgm_set_rectify(h, rows, cols, *m, W), "both sizes are zero")
            for k in range(4):
                refused(L.sgm_set_rectify(h, sh, sw, *(m[:k] + [None] + m[k + 1:]), W), "NULL map")
            refused(L.sgm_set_rectify(h, sh, sw, None, None, None, None, W), "NULL map")
            refused(L.sgm_set_rectify(h, sh, sw, *m, W - 1), "map_pitch")
            assert s.rectify_size == (0, 0)
            # remap and rectified calls with no maps set
            refused(L.sgm_remap_device(h, 0, d_src.data_ptr(), sw, d_dst.data_ptr(), W, None), "no maps")
            refused(L.sgm_stage_remap(h, 0, _p(img), sw, _p(out)), "no maps")
            refused(L.sgm_stage_rectified(h, 0, _p(out)), "no maps")
            refused(L.sgm_stage_rectify_valid(h, 0, _p(out)), "no maps")
            ptr, rp = ctypes.c_void_p(), ctypes.c_int()
            refused(L.sgm_get_rectified(h, 0, ctypes.byref(ptr), ctypes.byref(rp)), "no maps")
            s.set_rectify(*r)
            # views, pitches, NULL images
            for view in (2, -1):
                refused(L.sgm_remap_device(h, view, d_src.data_ptr(), sw, d_dst.data_ptr(), W, None), "view")
                refused(L.sgm_stage_remap(h, view, _p(img), sw, _p(out)), "view")
                refused(L.sgm_stage_rectify_valid(h, view, _p(out)), "view")
            refused(L.sgm_remap_device(h, 0, d_src.data_ptr(), sw - 1, d_dst.data_ptr(), W, None), "src_pitch")
            refused(L.sgm_stage_remap(h, 0, _p(img), sw - 1, _p(out)), "src_pitch")
            refused(L.sgm_remap_device(h, 0, d_src.data_ptr(), sw, d_dst.data_ptr(), W - 1, None), "dst_pitch")
            refused(L.sgm_remap_device(h, 0, None, sw, d_dst.data_ptr(), W, None), "NULL")
            refused(L.sgm_remap_device(h, 0, d_src.data_ptr(), sw, None, W, None), "NULL")
            refused(L.sgm_stage_remap(h, 0, None, sw, _p(out)), "NULL")
            refused(L.sgm_stage_remap(h, 0, _p(img), sw, None), "NULL")
            refused(L.sgm_stage_rectified(h, 0, None), "NULL")
            refused(L.sgm_stage_rectify_valid(h, 0, None), "NULL")
            assert L.sgm_get_rectified(h, 0, None, ctypes.byref(rp)) == _capi.SGM_ERR_INVALID_ARG
            assert L.sgm_get_rectified(h, 0, ctypes.byref(ptr), None) == _capi.SGM_ERR_INVALID_ARG
            refused(L.sgm_get_rectified(h, 0, ctypes.byref(ptr), ctypes.byref(rp)), "no frame")
            with pytest.raises(ValueError):      # the class layer checks the maps' shape
                s.set_rectify(sh, sw, r[2][:, :-1], r[3], r[4], r[5])
        # one input stage at a time, in both directions
        with pytest.raises(SGMError, match="sgm_set_input_size: rectification maps are set"):
            sgm.set_input_size(40, 60)
        assert (sgm.in_h, sgm.in_w) == RAW       # (a refused call changes nothing)
        sgm.set_input_size(0, 0)                 # (off stays allowed)
        assert sgm.rectify_size == RAW and (sgm.in_h, sgm.in_w) == RAW
        sgm.set_rectify(0, 0)
        sgm.set_input_size(40, 60)
        with pytest.raises(SGMError, match="sgm_set_rectify: an input size is set"):
            sgm.set_rectify(*r)
        assert (sgm.in_h, sgm.in_w) == (40, 60)
        sgm.set_rectify(0, 0)                    # (off stays allowed)
        assert sgm.input_size == (40, 60) and sgm.rectify_size == (0, 0) and (sgm.in_h, sgm.in_w) == (40, 60)
        sgm.set_input_size(0, 0)
        assert (sgm.in_h, sgm.in_w) == (H, W)
        # an aux_only handle holds maps but runs no frames; views after a frame
        sgm.set_rectify(*r)
        sgm.process(*raw_pair())
        for view in (2, -1):
            with pytest.raises(SGMError, match="view"):
                sgm.rectified(view)
        d_out = torch.empty((H, W), dtype=torch.float32, device=DEV)
        with pytest.raises(SGMError, match="aux_only"):
            aux.process_device(d_src.data_ptr(), d_src.data_ptr(), d_out.data_ptr())
