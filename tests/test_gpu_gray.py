"""Colour input on the GPU (sgm_set_input_format / sgm_gray_device /
sgm_stage_gray / sgm_get_input_gray), bit-exact against
tests/gray_recipe.py over every pixel: the stand-alone conversion over every
format, widths around the four-pixel group and the workgroup, dense, padded and
misaligned buffers; then frames: a colour handle fed colour images equals a grey
handle with the same input stage fed recipe.gray(raw), for every kind of handle
and every input stage (none: the conversion launch; an input size or maps: the
fused resize and remap launches), through the device entry point, replayed from
a HIP graph; the device bytes; every error."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import gray_recipe as gr
import rectify_recipe as rc
import resize_recipe as rr
from support import bits
from stereo_matching_amd import BM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 0xA5
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 257)
HEIGHTS = (1, 2, 17)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------- stand-alone conversion

def layouts(w, bpp):
    """(name, source offset, source pitch, destination offset, destination pitch)."""
    yield "dense", 0, w * bpp, 0, w
    yield "padded", 0, w * bpp + 5, 0, w + 7
    for o in (1, 2, 3):
        yield f"offset{o}", o, w * bpp, o, w


def flat(rows_bytes, off, pitch):
    """A sentinel-filled byte buffer holding the rows at off + y * pitch, with slack on both sides."""
    h, n = rows_bytes.shape
    buf = np.full(off + h * pitch + 16, SENTINEL, np.uint8)
    for y in range(h):
        buf[off + y * pitch: off + y * pitch + n] = rows_bytes[y]
    return buf


@pytest.mark.parametrize("aux", [True, False], ids=["aux_only", "full"])
@pytest.mark.parametrize("fmt", gr.FORMATS)
def test_gray_matches_the_recipe(fmt, aux):
    bpp = gr.bytes_per_pixel(fmt)
    cases = []
    for h in HEIGHTS:
        for w in WIDTHS:
            img = gr.random_image(h, w, bpp, 7 * h + w)
            want = gr.gray(img, fmt)
            for name, so, sp, do, dp in layouts(w, bpp):
                src = flat(img.reshape(h, w * bpp), so, sp)
                d_src = torch.from_numpy(src).to(DEV)
                d_dst = torch.full((do + h * dp + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
                cases.append((h, w, name, so, sp, do, dp, src, want, d_src, d_dst))
    torch.cuda.synchronize(DEV)                  # (the handle's stream is not ordered with torch's)
    with SGM(24, 80, 1, 32, aux_only=aux) as sgm:
        for h, w, name, so, sp, do, dp, src, want, d_src, d_dst in cases:
            sgm.gray_device(fmt, d_src.data_ptr() + so, h, w, d_dst.data_ptr() + do, src_pitch=sp, dst_pitch=dp)
        sgm.check()
        for h, w, name, so, sp, do, dp, src, want, d_src, d_dst in cases:
            got = d_dst.cpu().numpy()
            # the image, and every byte before, between and after its rows
            assert np.array_equal(got, flat(want, do, dp)), (h, w, name)
            assert np.array_equal(d_src.cpu().numpy(), src), (h, w, name)
        # host buffers (the size is the call's own, whatever the handle's)
        for h, w in ((1, 1), (17, 65), (37, 257)):
            img = gr.random_image(h, w, bpp, h + w)
            assert np.array_equal(sgm.gray(img, fmt), gr.gray(img, fmt))


# ------------------------------------------------------------------ frames

FRAME = (24, 80, 32)   # working rows, cols, D
RAW = (37, 53)
STAGES = ("none", "size", "rectify")
VARIANTS = {
    "views2": dict(views=2),
    "left": dict(views=1),
    "right": dict(views=1, view="right"),
    "paths4": dict(views=2, paths=4),
    "min_disp8": dict(views=2, min_disp=8),
    "config5": dict(views=2, sky_detect=True, post_filter=True, lk_refine=True, post_filter_launches=8),
    "bm": dict(cls=BM),
}


def rig(h, w, sh, sw):
    return (sh, sw, *rc.maps(h, w, sh, sw, 0), *rc.maps(h, w, sh, sw, 1))


def stage_kw(stage, h=FRAME[0], w=FRAME[1], raw=RAW):
    if stage == "size":
        return dict(input_size=raw)
    if stage == "rectify":
        return dict(rectify=rig(h, w, *raw))
    return {}


def raw_shape(stage):
    return FRAME[:2] if stage == "none" else RAW


def staged(stage, g, view, h=FRAME[0], w=FRAME[1]):
    """The recipe chain after the conversion: what the frame matches."""
    if stage == "size":
        return rr.resize(g, h, w)
    if stage == "rectify":
        return rc.remap(g, *rc.maps(h, w, g.shape[0], g.shape[1], view))
    return g


def colourise(g, fmt, seed=0):
    """A colour image whose channels differ, from a grey one (so a stereo pair stays a stereo pair)."""
    ch = gr.bytes_per_pixel(fmt)
    out = np.empty(g.shape + (ch,), np.uint8)
    out[..., 0] = g
    out[..., 1] = g.astype(np.int64) * 3 // 4 + 17
    out[..., 2] = 255 - g
    if ch == 4:
        out[..., 3] = np.random.default_rng(seed).integers(0, 256, g.shape, dtype=np.uint8)
    return out


def colour_pair(shape, fmt, k=0):
    left, right = synthetic.stereo_pair(shape[0], shape[1], 32, pair_index=5 + k, kind="road")
    return colourise(left, fmt, 1), colourise(right, fmt, 2)


def make(variant, stage="none", fmt="gray8"):
    kw = dict(VARIANTS[variant])
    cls = kw.pop("cls", SGM)
    H, W, D = FRAME
    if cls is SGM:
        kw["confidence"] = True
    return cls(H, W, 1, D, input_format=fmt, **stage_kw(stage), **kw)


def frame_maps(sgm, left, right):
    sgm.process(left, right)
    m = {"out": sgm.get_disp() if sgm.params.post_filter or sgm.params.lk_refine else sgm.get_lr_disp(),
         "raw": sgm.get_raw_disp()}
    if sgm.params.solver == _capi.SGM_SOLVER_SGM:
        m["conf"] = sgm.get_confidence(1 if sgm.params.view == _capi.SGM_VIEW_RIGHT else 0)
        if sgm.params.views == 2:
            m["conf_r"] = sgm.get_confidence(1)
    return m


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_colour_frame_equals_grey_frame_of_the_recipe(variant, stage):
    fmt = gr.FORMATS[(list(VARIANTS).index(variant) + STAGES.index(stage)) % 4]
    left, right = colour_pair(raw_shape(stage), fmt)
    gl, gr_ = gr.gray(left, fmt), gr.gray(right, fmt)
    with make(variant, stage, fmt) as colour, make(variant, stage) as grey:
        assert colour.input_format == fmt and grey.input_format == "gray8"
        assert (colour.in_h, colour.in_w, colour.in_ch) == (*raw_shape(stage), gr.bytes_per_pixel(fmt))
        got, want = frame_maps(colour, left, right), frame_maps(grey, gl, gr_)
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), k
        assert np.array_equal(colour.input_gray(0), staged(stage, gl, 0))
        assert np.array_equal(colour.input_gray(1), staged(stage, gr_, 1))
        if stage == "size":                      # the input stage's own getter hands out the same image
            assert np.array_equal(colour.get_resized(1), colour.input_gray(1))
        if stage == "rectify":
            assert np.array_equal(colour.rectified(1), colour.input_gray(1))
        with pytest.raises(ValueError):          # a grey image is now the wrong shape
            colour.process(gl, gr_)


EDGES = [("size", (24, 80), (1, 1)), ("size", (24, 80), (2, 3)), ("size", (24, 80), (48, 160)),
         ("rectify", (24, 80), (1, 1)), ("rectify", (24, 80), (2, 3)),
         ("none", (17, 65), (17, 65)), ("size", (17, 65), (37, 53)), ("rectify", (17, 65), (37, 53))]


@pytest.mark.parametrize("fmt", gr.FORMATS)
def test_fused_kernels_edges_through_input_gray(fmt):
    bpp = gr.bytes_per_pixel(fmt)
    made = {}
    try:
        for stage, (h, w), raw in EDGES:
            if (h, w) not in made:
                made[(h, w)] = SGM(h, w, 1, 32, views=1)
            sgm = made[(h, w)]
            sgm.set_input_size(0, 0)
            sgm.set_rectify(0, 0)
            sgm.set_input_format(fmt)
            if stage == "size":
                sgm.set_input_size(*raw)
            if stage == "rectify":
                sgm.set_rectify(*rig(h, w, *raw))
            left = gr.random_image(raw[0], raw[1], bpp, 3 + raw[0])
            right = gr.random_image(raw[0], raw[1], bpp, 4 + raw[1])
            sgm.process(left, right)
            for view, img in ((0, left), (1, right)):
                want = staged(stage, gr.gray(img, fmt), view, h, w)
                assert np.array_equal(sgm.input_gray(view), want), (stage, h, w, raw, view)
    finally:
        for s in made.values():
            s.close()


@pytest.mark.parametrize("fmt", gr.FORMATS)
def test_grey_pixels_in_a_colour_frame_equal_the_grey_frame(fmt):
    H, W, D = FRAME
    left, right = synthetic.stereo_pair(H, W, D, pair_index=2, kind="road")
    with SGM(H, W, 1, D, input_format=fmt) as colour, SGM(H, W, 1, D) as grey:
        colour.process(gr.from_gray(left, fmt), gr.from_gray(right, fmt))
        grey.process(left, right)
        assert np.array_equal(bits(colour.get_lr_disp()), bits(grey.get_lr_disp()))
        assert np.array_equal(colour.get_raw_disp(), grey.get_raw_disp())
        assert np.array_equal(colour.input_gray(0), left) and np.array_equal(colour.input_gray(1), right)


def test_side_by_side_bgr_frame_through_the_device_entry_point():
    # one side-by-side colour camera frame split by pitch, on a caller's stream
    H, W, D = FRAME
    left, right = colour_pair((H, W), "bgr8")
    pitch = 2 * W * 3 + 13
    both = np.hstack([left, right]).reshape(H, 2 * W * 3)
    buf = np.full((H, pitch), SENTINEL, np.uint8)
    buf[:, : 2 * W * 3] = both
    frame = torch.from_numpy(buf).to(DEV)
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    raw = torch.zeros((H, W), dtype=torch.int16, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(H, W, 1, D, input_format="bgr8") as colour, SGM(H, W, 1, D) as grey:
        with pytest.raises(SGMError, match="pitch"):     # a pitch below cols x bytes per pixel
            colour.process_device(frame.data_ptr(), frame.data_ptr() + 3 * W, out.data_ptr(), pitch=3 * W - 1)
        colour.process_device(frame.data_ptr(), frame.data_ptr() + 3 * W, out.data_ptr(), pitch=pitch,
                              d_raw=raw.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        colour.check()
        gl, gr_ = gr.gray(left, "bgr8"), gr.gray(right, "bgr8")
        # the handle-owned grey image, read on the device
        ptr, gp = ctypes.c_void_p(), ctypes.c_int()
        _capi.check(colour._lib.sgm_get_input_gray(colour._h, 0, ctypes.byref(ptr), ctypes.byref(gp)), colour._h)
        assert ptr.value and gp.value == W
        assert np.array_equal(colour.input_gray(0), gl) and np.array_equal(colour.input_gray(1), gr_)
        grey.process(gl, gr_)
        assert np.array_equal(bits(out.cpu().numpy()), bits(grey.get_lr_disp()))
        assert np.array_equal(raw.cpu().numpy().view(np.uint16), grey.get_raw_disp())
    assert np.array_equal(frame.cpu().numpy(), buf)


@pytest.mark.timeout(120)
def test_colour_frame_with_a_fill_budget_replays_from_a_hip_graph():
    H, W, D = FRAME
    fmt = "rgba8"
    kw = dict(post_filter=True, post_filter_launches=8)
    with SGM(H, W, 1, D, input_format=fmt, **kw) as sgm, SGM(H, W, 1, D, **kw) as grey:
        stream = torch.cuda.ExternalStream(sgm.stream, device=DEV)
        d_l = torch.empty((H, W, 4), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_g = torch.empty((H, W), dtype=torch.float32, device=DEV)
        out_e = torch.empty_like(out_g)

        def frame(st, out):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=st)

        def load(k):
            left, right = colour_pair((H, W), fmt, k)
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
            gl, gr_ = gr.gray(left, fmt), gr.gray(right, fmt)
            grey.process(gl, gr_)
            assert np.array_equal(bits(out_g.cpu().numpy()), bits(grey.get_disp())), k
            assert np.array_equal(sgm.input_gray(1), gr_), k


def test_device_bytes_and_switching_the_format_off_restores_the_handle():
    H, W, D = FRAME
    sh, sw = RAW
    left, right = synthetic.stereo_pair(H, W, D, pair_index=2, kind="road")
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D) as plain:
        before = sgm.device_bytes
        for fmt in ("bgr8", "rgba8"):            # the format alone; changing it re-sizes the staging
            bpp = gr.bytes_per_pixel(fmt)
            sgm.set_input_format(fmt)
            assert sgm.device_bytes == before + 2 * H * W + 2 * H * W * bpp
        sgm.set_input_format("gray8")
        assert sgm.device_bytes == before
        # with an input size or maps, only the staging of the raw images grows
        sgm.set_input_size(sh, sw)
        with_size = sgm.device_bytes
        assert with_size == before + 2 * H * W + 2 * sh * sw
        sgm.set_input_format("bgra8")
        assert sgm.device_bytes == with_size + 2 * sh * sw * 3
        sgm.set_input_size(0, 0)                 # (the format stays: the full-size staging)
        assert sgm.device_bytes == before + 2 * H * W + 2 * H * W * 4
        sgm.set_rectify(*rig(H, W, sh, sw))
        assert sgm.device_bytes == before + 2 * 8 * H * W + 2 * H * W + 2 * sh * sw * 4
        sgm.set_input_format("gray8")
        assert sgm.device_bytes == before + 2 * 8 * H * W + 2 * H * W + 2 * sh * sw
        sgm.set_rectify(0, 0)
        assert sgm.device_bytes == before == plain.device_bytes
        assert sgm.input_format == "gray8" and (sgm.in_h, sgm.in_w, sgm.in_ch) == (H, W, 1)
        sgm.process(left, right)
        plain.process(left, right)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(plain.get_lr_disp()))
        assert np.array_equal(sgm.get_raw_disp(), plain.get_raw_disp())
        with pytest.raises(SGMError, match="grey"):
            sgm.input_gray(0)


@pytest.mark.parametrize("stage", ["size", "rectify"])
def test_either_order_of_format_and_stage_gives_the_same_frames(stage):
    H, W, D = FRAME
    fmt = "rgb8"
    left, right = colour_pair(RAW, fmt)
    set_stage = {"size": lambda s: s.set_input_size(*RAW), "rectify": lambda s: s.set_rectify(*rig(H, W, *RAW))}[stage]
    with SGM(H, W, 1, D) as a, SGM(H, W, 1, D) as b:
        a.set_input_format(fmt)
        set_stage(a)
        set_stage(b)
        b.set_input_format(fmt)
        assert a.device_bytes == b.device_bytes
        a.process(left, right)
        b.process(left, right)
        assert np.array_equal(bits(a.get_lr_disp()), bits(b.get_lr_disp()))
        assert np.array_equal(a.get_raw_disp(), b.get_raw_disp())
        for view, img in ((0, left), (1, right)):
            want = staged(stage, gr.gray(img, fmt), view)
            assert np.array_equal(a.input_gray(view), want) and np.array_equal(b.input_gray(view), want)


def test_errors():
    H, W, D = FRAME
    h0, w0 = 9, 31
    img = gr.random_image(h0, w0, 3, 3)
    d_src = torch.from_numpy(img).to(DEV)
    d_dst = torch.empty((h0, w0), dtype=torch.uint8, device=DEV)
    out = np.empty((h0, w0), np.uint8)
    full = np.empty((H, W), np.uint8)
    torch.cuda.synchronize(DEV)
    with SGM(H, W, 1, D) as sgm, SGM(H, W, 1, D, aux_only=True) as aux:
        for s in (sgm, aux):
            L, h = s._lib, s._h

            def refused(rc_, what):
                assert rc_ == _capi.SGM_ERR_INVALID_ARG
                msg = L.sgm_last_error(h).decode()
                assert what in msg, msg

            src, dst = d_src.data_ptr(), d_dst.data_ptr()
            # sgm_gray_device / sgm_stage_gray: pointers, sizes, formats, pitches
            refused(L.sgm_gray_device(h, 1, None, h0, w0, 3 * w0, dst, w0, None), "NULL")
            refused(L.sgm_gray_device(h, 1, src, h0, w0, 3 * w0, None, w0, None), "NULL")
            refused(L.sgm_stage_gray(h, 1, None, h0, w0, 3 * w0, _p(out)), "NULL")
            refused(L.sgm_stage_gray(h, 1, _p(img), h0, w0, 3 * w0, None), "NULL")
            for rows, cols in ((0, w0), (h0, 0), (-1, w0)):
                refused(L.sgm_gray_device(h, 1, src, rows, cols, 3 * w0, dst, w0, None), "size must be")
                refused(L.sgm_stage_gray(h, 1, _p(img), rows, cols, 3 * w0, _p(out)), "size must be")
            refused(L.sgm_gray_device(h, 0, src, h0, w0, 3 * w0, dst, w0, None), "grey already")
            refused(L.sgm_stage_gray(h, 0, _p(img), h0, w0, 3 * w0, _p(out)), "grey already")
            for bad in (5, -1):
                refused(L.sgm_gray_device(h, bad, src, h0, w0, 3 * w0, dst, w0, None), "unknown pixel format")
                refused(L.sgm_stage_gray(h, bad, _p(img), h0, w0, 3 * w0, _p(out)), "unknown pixel format")
                refused(L.sgm_set_input_format(h, bad), "unknown pixel format")
            refused(L.sgm_gray_device(h, 1, src, h0, w0, 3 * w0 - 1, dst, w0, None), "src_pitch")
            refused(L.sgm_stage_gray(h, 2, _p(img), h0, w0, 3 * w0 - 1, _p(out)), "src_pitch")
            refused(L.sgm_gray_device(h, 3, src, h0, w0, 3 * w0, dst, w0, None), "src_pitch")   # (4 bytes per pixel)
            refused(L.sgm_gray_device(h, 1, src, h0, w0, 3 * w0, dst, w0 - 1, None), "dst_pitch")
            # sgm_get_input_gray on a grey handle
            ptr, gp = ctypes.c_void_p(), ctypes.c_int()
            refused(L.sgm_get_input_gray(h, 0, ctypes.byref(ptr), ctypes.byref(gp)), "grey")
            refused(L.sgm_stage_input_gray(h, 0, _p(full)), "grey")
            refused(L.sgm_stage_input_gray(h, 0, None), "NULL")
            assert L.sgm_get_input_gray(h, 0, None, ctypes.byref(gp)) == _capi.SGM_ERR_INVALID_ARG
            assert L.sgm_get_input_gray(h, 0, ctypes.byref(ptr), None) == _capi.SGM_ERR_INVALID_ARG
            assert s.input_format == "gray8" and (s.in_h, s.in_w, s.in_ch) == (H, W, 1)
        # an aux_only handle runs no frames: no colour format (it still converts per call)
        with pytest.raises(SGMError, match="aux_only"):
            aux.set_input_format("bgr8")
        assert aux.input_format == "gray8"
        aux.set_input_format("gray8")
        assert np.array_equal(aux.gray(img, "bgr8"), gr.gray(img, "bgr8"))
        with pytest.raises(ValueError):
            sgm.set_input_format("yuv422")
        with pytest.raises(ValueError):          # the class layer checks the channel count
            sgm.gray(img, "bgra8")
        # a refused call changes nothing
        sgm.set_input_size(*RAW)
        sgm.set_input_format("rgb8")
        with pytest.raises(SGMError, match="unknown pixel format"):
            sgm.set_input_format(7)
        assert sgm.input_format == "rgb8" and (sgm.in_h, sgm.in_w, sgm.in_ch) == (*RAW, 3)
        # before any frame, then other views after one
        with pytest.raises(SGMError, match="no frame"):
            sgm.input_gray(0)
        sgm.process(*colour_pair(RAW, "rgb8"))
        for view in (2, -1):
            with pytest.raises(SGMError, match="view"):
                sgm.input_gray(view)
        sgm.set_input_format("bgr8")             # a new format: the old frame's image is gone
        with pytest.raises(SGMError, match="no frame"):
            sgm.input_gray(0)
