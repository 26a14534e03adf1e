"""Reprojection through Q on the GPU (sgm_set_reproject / sgm_reproject_device /
sgm_stage_reproject / sgm_get_reprojected), bit-exact against
tests/reproject_recipe.py on every element: the stand-alone call over widths
around the 64-column chunk and the 256-column workgroup, heights around the
four-row workgroup, both scales, two minimum disparities, each product alone and
all three, dense, padded and element-misaligned buffers with sentinels all
round, aux_only and full handles, a skewed Q and camera_q; then frames of every
kind of handle, whose products equal the recipe on the map the same call
returned (itself the oracle's); a frame replayed from a HIP graph; the
handle-owned buffers; the device bytes; the launch ledger; every error.

The stand-alone call works on the handle's working grid, and sgm_create takes no
working grid below 5 x 3 (the cost window), aux_only handles included: working
grids 1 to 4 columns wide or 1 or 2 rows high do not exist.  What those sizes
would exercise in the kernel -- a row's last chunk of 1, 2, 3 and 4 pixels
(3, 6, 9, 12 dwords of XYZ: none, one, two and three whole 16-byte stores), a
workgroup's last 1 and 2 rows -- runs here at widths 65 to 68 and 257 and heights
5 and 6, and test_working_grids_below_the_cost_window_do_not_exist pins that the
small grids are refused.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import gray_recipe as gr
import oracle
import reproject_recipe as rp
import resize_recipe as rr
from support import bits
from stereo_matching_amd import BM, SGM, _capi, camera_q, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENT32 = 0x5A5AA5A5
SENT16 = 0x5AA5
XYZ, DEPTH, DEPTH16 = rp.XYZ, rp.DEPTH, rp.DEPTH16
WIDTHS = (5, 63, 64, 65, 66, 67, 68, 257)
HEIGHTS = (3, 5, 6, 17)
SMALL = ((1, 17), (2, 17), (3, 17), (4, 17), (64, 1), (64, 2))   # (width, height): below the cost window
D0 = 32
CAM = (700.5, 699.25, 31.5, 8.25, 0.12)
NAMES = {XYZ: "xyz", DEPTH: "depth", DEPTH16: "depth16"}
CH = {XYZ: 3, DEPTH: 1, DEPTH16: 1}


def range_for(disp, q, invalid, scale):
    """A max_range with pixels on both sides of it: the median Z of the pixels valid without one."""
    r = rp.reproject(disp, q, invalid, scale)
    z = r["depth"][~r["missing"]]
    z = z[z > 0]
    assert z.size >= 2
    mr = float(np.float32(np.median(z)))
    w = rp.reproject(disp, q, invalid, scale, mr)
    assert (w["missing"] & ~r["missing"]).any() and (~w["missing"]).any()      # both sides of the test
    return mr


def check_hand_map(disp, D, m):
    inv = np.float32(D + m + 1)
    assert (disp == inv).any() and (disp == 0).any() and (disp == np.float32(D - 1)).any()
    assert (disp != np.floor(disp)).any()


class Buf:
    """A device buffer of `which`'s element type holding rows x (ch * cols) elements at element offset
    `off`, `pitch` elements apart, filled with a sentinel; .expect(img) is the host image of it."""

    def __init__(self, which, rows, cols, off, pad):
        self.n, self.rows, self.off = CH[which] * cols, rows, off
        self.pitch = self.n + pad
        self.u16 = which == DEPTH16
        self.size = off + rows * self.pitch + 8
        self.t = torch.full((self.size,), SENT16 if self.u16 else SENT32,
                            dtype=torch.int16 if self.u16 else torch.int32, device=DEV)
        self.ptr = self.t.data_ptr() + off * (2 if self.u16 else 4)

    def expect(self, img):
        img = bits(img).reshape(self.rows, self.n)
        e = np.full(self.size, SENT16 if self.u16 else SENT32, np.uint16 if self.u16 else np.uint32)
        for y in range(self.rows):
            e[self.off + y * self.pitch: self.off + y * self.pitch + self.n] = img[y]
        return e

    def host(self):
        return self.t.cpu().numpy().view(np.uint16 if self.u16 else np.uint32)


LAYOUTS = {"dense": (0, 0), "padded": (0, 7), "misaligned": (1, 0), "misaligned_padded": (3, 5)}
# (product set, layout): all three in every layout, each product alone dense and misaligned
RUNS = [(7, name) for name in LAYOUTS] + [(w, "dense") for w in (XYZ, DEPTH, DEPTH16)] + \
       [(w, "misaligned_padded") for w in (XYZ, DEPTH, DEPTH16)]


@pytest.mark.parametrize("form", ["0", "1"], ids=["store12", "store16_lds"])
@pytest.mark.parametrize("m", [0, 16])
@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("aux", [True, False], ids=["aux_only", "full"])
def test_stand_alone_call_matches_the_recipe(aux, scale, m, form, monkeypatch):
    # both XYZ store forms of the kernel (sgm_reproject.hip): the handle reads the switch in the setter
    monkeypatch.setenv("SGM_REPROJECT_STORE", form)
    qs = {"skewed": rp.skewed_q(), "camera_q": camera_q(*CAM).ravel()}
    assert np.all(qs["skewed"] != 0)
    assert np.array_equal(qs["camera_q"], rp.camera_q(*CAM))
    for H in HEIGHTS:
        for W in WIDTHS:
            disp = rp.hand_map(H, W, D0, m, seed=H + W)
            check_hand_map(disp, D0, m)
            off, pad = 1, 3                              # the map too: misaligned and padded
            src = np.full(off + H * (W + pad) + 4, -7.0, np.float32)
            for y in range(H):
                src[off + y * (W + pad): off + y * (W + pad) + W] = disp[y]
            d_src = torch.from_numpy(src).to(DEV)
            todo = []
            with SGM(H * scale, W * scale, scale, D0, aux_only=aux, min_disp=m) as sgm:
                assert (sgm.rows, sgm.cols) == (H, W)
                for qname, q in qs.items():
                    mr = range_for(disp, q, sgm.invalid_disp, scale)
                    ds = 1000.0 if qname == "camera_q" else 150.0
                    want = rp.reproject(disp, q, sgm.invalid_disp, scale, mr, ds)
                    assert want["missing"].any() and not want["missing"].all()
                    sgm.set_reproject(q, outputs=() if aux else ("depth16",), max_range=mr, depth_scale=ds)
                    torch.cuda.synchronize(DEV)          # (the handle's stream is not ordered with torch's)
                    for mask, layout in RUNS:
                        bufs = {w: Buf(w, H, W, *LAYOUTS[layout]) for w in (XYZ, DEPTH, DEPTH16) if mask & w}
                        torch.cuda.synchronize(DEV)
                        sgm.reproject_device(
                            d_src.data_ptr() + 4 * off, pitch=W + pad,
                            d_xyz=bufs[XYZ].ptr if XYZ in bufs else 0, xyz_pitch=bufs[XYZ].pitch if XYZ in bufs else 0,
                            d_depth=bufs[DEPTH].ptr if DEPTH in bufs else 0,
                            depth_pitch=bufs[DEPTH].pitch if DEPTH in bufs else 0,
                            d_depth16=bufs[DEPTH16].ptr if DEPTH16 in bufs else 0,
                            depth16_pitch=bufs[DEPTH16].pitch if DEPTH16 in bufs else 0)
                        todo.append((qname, mask, layout, bufs, want))
                    sgm.check()
                    # host buffers
                    got = sgm.reproject(disp)
                    for k in ("xyz", "depth", "depth16"):
                        assert np.array_equal(bits(got[k]), bits(want[k])), (H, W, qname, k)
                for qname, mask, layout, bufs, want in todo:
                    for w, b in bufs.items():
                        # the product, and every element before, between and after its rows
                        assert np.array_equal(b.host(), b.expect(want[NAMES[w]])), (H, W, qname, mask, layout, NAMES[w])
            assert np.array_equal(bits(d_src.cpu().numpy()), bits(src)), (H, W)


@pytest.mark.parametrize("aux", [True, False], ids=["aux_only", "full"])
def test_working_grids_below_the_cost_window_do_not_exist(aux):
    for w, h in SMALL:
        with pytest.raises(SGMError):
            SGM(h, w, 1, D0, aux_only=aux)


# ------------------------------------------------------------------ frames

def plane_pair(h, w, seed=1, shift=8, strip=0.7):
    """A fronto-parallel plane at `shift` pixels beside a strip the right image does not show: chosen on
    the CPU so that every kind of frame's oracle map holds between 5% and 50% invalid pixels."""
    left = synthetic.noise_image(h, w, seed)
    right = synthetic.noise_image(h, w, seed ^ 0x5555)
    c = int(w * strip)
    right[:, : c - shift] = left[:, shift:c]
    return left, right


CONFIGS = {"D32_s1": (24, 80, 32, 1), "D64_s2": (48, 160, 64, 2)}       # full h, w, D, scale: 24 x 80 working
KINDS = ("views2", "left", "bm", "post_filter", "lk_refine", "size_colour")
_oracle_maps = {}


def make(kind, h, w, D, s, **extra):
    if kind == "views2":
        return SGM(h, w, s, D, **extra)
    if kind == "left":
        return SGM(h, w, s, D, views=1, **extra)
    if kind == "bm":
        return BM(h, w, s, D, **extra)
    if kind == "post_filter":
        return SGM(h, w, s, D, post_filter=True, post_filter_launches=8, **extra)
    if kind == "lk_refine":
        return SGM(h, w, s, D, post_filter=True, lk_refine=True, post_filter_launches=8, **extra)
    assert kind == "size_colour"
    return SGM(h, w, s, D, input_size=(2 * h, 2 * w), input_format="bgr8", **extra)


def images(kind, h, w):
    """What process() takes, and the grey pair the frame matches (by the recipes)."""
    left, right = plane_pair(h, w)
    if kind != "size_colour":
        return (left, right), (left, right)
    raw = tuple(gr.from_gray(np.repeat(np.repeat(g, 2, 0), 2, 1), "bgr8") for g in (left, right))
    return raw, tuple(rr.resize(gr.gray(c, "bgr8"), h, w) for c in raw)


def oracle_map(kind, cfg):
    """The oracle's final map of a frame of `kind` (computed once, shared, never written)."""
    if (kind, cfg) not in _oracle_maps:
        h, w, D, s = CONFIGS[cfg]
        _, (left, right) = images(kind, h, w)
        if kind in ("views2", "size_colour"):
            m = oracle.process(left, right, D, s, final=False)["lr"]
        elif kind == "left":
            m = oracle.process(left, right, D, s, views=1)["sub"]
        elif kind == "bm":
            m = oracle.post_filter(oracle.bm_process(left, right, D, s).astype(np.float32), D, s)
        else:
            m = oracle.process(left, right, D, s)["final"]
            if kind == "lk_refine":
                m = oracle.lk_refine(left[::s, ::s][: h // s, : w // s], right[::s, ::s][: h // s, : w // s], m, D)
        m.setflags(write=False)
        _oracle_maps[(kind, cfg)] = m
    return _oracle_maps[(kind, cfg)]


def frame_map(sgm):
    return sgm.get_disp() if sgm.params.post_filter or sgm.params.lk_refine else sgm.get_lr_disp()


def frame_q(cfg):
    return camera_q(*CAM).ravel() if cfg == "D32_s1" else rp.skewed_q()


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_frame_products_equal_the_recipe_on_the_frames_map(kind, cfg):
    h, w, D, s = CONFIGS[cfg]
    ref = oracle_map(kind, cfg)
    invalid = float((ref == np.float32(D + 1)).mean())
    print(kind, cfg, "oracle map: invalid", invalid)
    assert invalid >= 0.05 and 1.0 - invalid >= 0.50
    q = frame_q(cfg)
    mr = range_for(ref, q, D + 1, s)
    raw, _ = images(kind, h, w)
    with make(kind, h, w, D, s) as sgm:
        sgm.set_reproject(q, outputs=("xyz", "depth", "depth16"), max_range=mr, depth_scale=250.0)
        sgm.process(*raw)
        got = frame_map(sgm)
        assert np.array_equal(bits(got), bits(ref))
        want = rp.reproject(got, q, sgm.invalid_disp, s, mr, 250.0)
        assert np.array_equal(bits(sgm.get_xyz()), bits(want["xyz"]))
        assert np.array_equal(bits(sgm.get_depth()), bits(want["depth"]))
        assert np.array_equal(sgm.get_depth16(), want["depth16"])
        assert want["depth16"].any() and want["missing"].any()


def test_constructor_keyword_gives_xyz_and_depth():
    h, w, D, s = CONFIGS["D32_s1"]
    q = camera_q(*CAM)
    left, right = plane_pair(h, w)
    with SGM(h, w, s, D, reproject=q) as sgm:
        qq, outputs, mr, ds = sgm.reprojection
        assert np.array_equal(qq, q) and outputs == XYZ | DEPTH and mr == 0.0 and ds == 1000.0
        sgm.process(left, right)
        want = rp.reproject(sgm.get_lr_disp(), q, sgm.invalid_disp, s)
        assert np.array_equal(bits(sgm.get_xyz()), bits(want["xyz"]))
        assert np.array_equal(bits(sgm.get_depth()), bits(want["depth"]))
        with pytest.raises(SGMError, match="not in the outputs"):
            sgm.get_depth16()
        sgm.set_reproject(None)
        assert sgm.reprojection is None


@pytest.mark.timeout(120)
def test_frame_with_a_fill_budget_replays_from_a_hip_graph():
    h, w, D, s = CONFIGS["D32_s1"]
    q = rp.skewed_q()
    with make("post_filter", h, w, D, s) as sgm:
        sgm.set_reproject(q, outputs=("xyz", "depth", "depth16"), max_range=900.0, depth_scale=50.0)
        stream = torch.cuda.ExternalStream(sgm.stream, device=DEV)
        d_l = torch.empty((h, w), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out = torch.empty((h // s, w // s), dtype=torch.float32, device=DEV)

        def frame(st):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=st)

        def load(k):
            left, right = plane_pair(h, w, seed=1 + k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))

        load(0)
        with torch.cuda.stream(stream):
            frame(stream.cuda_stream)                    # warm-up (the capture needs no first-call work)
        torch.cuda.synchronize(DEV)
        sgm.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(stream.cuda_stream)
        torch.cuda.synchronize(DEV)
        for k in (1, 2, 3):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize(DEV)
            sgm.check()
            replayed = {n: bits(f()).copy() for n, f in (("xyz", sgm.get_xyz), ("depth", sgm.get_depth),
                                                       ("depth16", sgm.get_depth16))}
            m = out.cpu().numpy()
            want = rp.reproject(m, q, sgm.invalid_disp, s, 900.0, 50.0)
            with torch.cuda.stream(stream):
                frame(stream.cuda_stream)                # the eager frame on the same images
            torch.cuda.synchronize(DEV)
            sgm.check()
            assert np.array_equal(bits(out.cpu().numpy()), bits(m)), k
            for n, f in (("xyz", sgm.get_xyz), ("depth", sgm.get_depth), ("depth16", sgm.get_depth16)):
                assert np.array_equal(replayed[n], bits(want[n])), (k, n)
                assert np.array_equal(bits(f()), bits(want[n])), (k, n)


def test_handle_owned_products_pointers_pitches_and_downloads():
    h, w, D, s = CONFIGS["D64_s2"]
    H, W = h // s, w // s
    q = rp.skewed_q()
    left, right = plane_pair(h, w)
    with SGM(h, w, s, D) as sgm:
        sgm.set_reproject(q, outputs=("xyz", "depth", "depth16"))
        L, hd = sgm._lib, sgm._h
        ptr, pitch = ctypes.c_void_p(), ctypes.c_int()
        assert L.sgm_get_reprojected(hd, XYZ, ctypes.byref(ptr), ctypes.byref(pitch)) == _capi.SGM_ERR_INVALID_ARG
        assert "no frame" in L.sgm_last_error(hd).decode()
        sgm.process(left, right)
        want = rp.reproject(sgm.get_lr_disp(), q, sgm.invalid_disp, s)
        seen = set()
        for which, tdt, ndt in ((XYZ, torch.int32, np.uint32), (DEPTH, torch.int32, np.uint32),
                                (DEPTH16, torch.int16, np.uint16)):
            _capi.check(L.sgm_get_reprojected(hd, which, ctypes.byref(ptr), ctypes.byref(pitch)), hd)
            assert ptr.value and pitch.value == CH[which] * W and ptr.value not in seen
            seen.add(ptr.value)
            # a device copy of the handle's buffer (process() has synchronised the frame)
            dst = torch.zeros((H * pitch.value,), dtype=tdt, device=DEV)
            torch.cuda.synchronize(DEV)
            assert _hip().hipMemcpy(dst.data_ptr(), ptr.value, dst.numel() * dst.element_size(), 3) == 0
            dev = dst.cpu().numpy().view(ndt)
            stage = {XYZ: sgm.get_xyz, DEPTH: sgm.get_depth, DEPTH16: sgm.get_depth16}[which]()
            assert np.array_equal(dev, bits(stage).ravel())
            assert np.array_equal(dev, bits(want[NAMES[which]]).ravel())


def _hip():
    """The HIP runtime the library runs on, for a plain device-to-device hipMemcpy (kind 3)."""
    rt = ctypes.CDLL(_capi.hip_runtimes()[0])
    rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return rt


def test_device_bytes_grow_by_the_products_and_return():
    h, w, D, s = CONFIGS["D64_s2"]
    npx = (h // s) * (w // s)
    q = rp.skewed_q()
    with SGM(h, w, s, D) as sgm, SGM(h, w, s, D) as plain, SGM(h, w, s, D, aux_only=True) as aux:
        before = sgm.device_bytes
        sizes = {"xyz": 12 * npx, "depth": 4 * npx, "depth16": 2 * npx}
        for outs in (("xyz",), ("depth",), ("depth16",), ("xyz", "depth"), ("depth", "depth16"),
                     ("xyz", "depth", "depth16"), ("depth16",)):
            sgm.set_reproject(q, outputs=outs)
            assert sgm.device_bytes == before + sum(sizes[o] for o in outs), outs
        sgm.set_reproject(None)
        assert sgm.device_bytes == before == plain.device_bytes
        aux_before = aux.device_bytes
        aux.set_reproject(q, outputs=())
        assert aux.device_bytes == aux_before            # Q alone
        aux.set_reproject(None)
        assert aux.device_bytes == aux_before
        left, right = plane_pair(h, w)
        sgm.process(left, right)
        plain.process(left, right)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(plain.get_lr_disp()))


def _ledger(sgm, left, right):
    sgm.set_profiling(True)
    sgm.process(left, right)
    prof = sgm.get_profile()
    sgm.set_profiling(False)
    return {k: (v[0], v[2]) for k, v in prof.items()}


@pytest.mark.parametrize("kind", ["views2", "left", "bm", "lk_refine"])
def test_launch_ledger_one_launch_more_and_off_equals_a_fresh_handle(kind):
    h, w, D, s = CONFIGS["D32_s1"]
    left, right = plane_pair(h, w)
    npx = float((h // s) * (w // s))
    with make(kind, h, w, D, s) as sgm, make(kind, h, w, D, s) as fresh:
        base = _ledger(fresh, left, right)
        assert "reproject" not in base
        sgm.set_reproject(rp.skewed_q(), outputs=("xyz", "depth", "depth16"))
        on = _ledger(sgm, left, right)
        assert on == dict(base, reproject=(1, npx))
        assert list(on)[-1] == "reproject"               # after the frame's last map stage
        sgm.set_reproject(None)
        assert _ledger(sgm, left, right) == base


def test_errors():
    h, w, D, s = CONFIGS["D32_s1"]
    H, W = h // s, w // s
    q = rp.skewed_q()
    good = dict(outputs=7, max_range=0.0, depth_scale=1000.0)

    def rec(qv=q, **kw):
        a = dict(good, **kw)
        return _capi.Reproject((ctypes.c_double * 16)(*qv), a["outputs"], a["max_range"], a["depth_scale"])

    d_disp = torch.zeros((H, W), dtype=torch.float32, device=DEV)
    d_xyz = torch.zeros((H, 3 * W), dtype=torch.float32, device=DEV)
    d_z = torch.zeros((H, W), dtype=torch.float32, device=DEV)
    d_16 = torch.zeros((H, W), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(h, w, s, D) as sgm, SGM(h, w, s, D, aux_only=True) as aux, \
            SGM(h, w, s, D, views=1, view="right") as right:
        for sg in (sgm, aux, right):
            L, hd = sg._lib, sg._h

            def refused(rc_, what):
                assert rc_ == _capi.SGM_ERR_INVALID_ARG
                msg = L.sgm_last_error(hd).decode()
                assert what in msg, msg

            if sg is right:                              # Q belongs to the left camera
                refused(L.sgm_set_reproject(hd, ctypes.byref(rec())), "SGM_VIEW_RIGHT")
                refused(L.sgm_reproject_device(hd, d_disp.data_ptr(), W, d_xyz.data_ptr(), 3 * W, None, 0, None, 0,
                                               None), "no Q is set")
                assert sg.reprojection is None
                continue
            p, x, z, u = d_disp.data_ptr(), d_xyz.data_ptr(), d_z.data_ptr(), d_16.data_ptr()
            # before the setter: no Q
            refused(L.sgm_reproject_device(hd, p, W, x, 3 * W, z, W, u, W, None), "no Q is set")
            refused(L.sgm_stage_reproject(hd, p, x, z, u), "no Q is set")
            # the setter's refusals change nothing
            for k in (0, 7, 15):
                for bad in (np.nan, np.inf, -np.inf):
                    qq = q.copy()
                    qq[k] = bad
                    refused(L.sgm_set_reproject(hd, ctypes.byref(rec(qq))), "not finite")
            refused(L.sgm_set_reproject(hd, ctypes.byref(rec(outputs=8))), "unknown bits")
            refused(L.sgm_set_reproject(hd, ctypes.byref(rec(outputs=-1))), "unknown bits")
            if sg is sgm:
                refused(L.sgm_set_reproject(hd, ctypes.byref(rec(outputs=0))), "outputs is 0")
            for bad in (-1.0, np.nan, np.inf):
                refused(L.sgm_set_reproject(hd, ctypes.byref(rec(max_range=bad))), "max_range")
            for bad in (0.0, -2.0, np.nan, np.inf):
                refused(L.sgm_set_reproject(hd, ctypes.byref(rec(outputs=4, depth_scale=bad))), "depth_scale")
                refused(L.sgm_set_reproject(hd, ctypes.byref(rec(outputs=7, depth_scale=bad))), "depth_scale")
            assert sg.reprojection is None
            got = _capi.Reproject()
            assert L.sgm_get_reproject(hd, ctypes.byref(got)) == _capi.SGM_OK and got.outputs == 0
            assert L.sgm_get_reproject(hd, None) == _capi.SGM_ERR_INVALID_ARG
            # depth_scale is not looked at without depth16
            sg.set_reproject(q, outputs=("xyz", "depth"), depth_scale=0.0)
            bytes_on = sg.device_bytes
            refused(L.sgm_set_reproject(hd, ctypes.byref(rec(outputs=8))), "unknown bits")
            assert sg.reprojection[1] == 3 and sg.device_bytes == bytes_on
            # the device call
            refused(L.sgm_reproject_device(hd, None, W, x, 3 * W, z, W, u, W, None), "NULL disparity map")
            refused(L.sgm_reproject_device(hd, p, W, None, 3 * W, None, W, None, W, None), "all three products")
            refused(L.sgm_reproject_device(hd, p, W - 1, x, 3 * W, z, W, u, W, None), "pitch")
            refused(L.sgm_reproject_device(hd, p, W, x, 3 * W - 1, z, W, u, W, None), "xyz_pitch")
            refused(L.sgm_reproject_device(hd, p, W, x, 3 * W, z, W - 1, u, W, None), "depth_pitch")
            refused(L.sgm_reproject_device(hd, p, W, x, 3 * W, z, W, u, W - 1, None), "depth16_pitch")
            assert L.sgm_reproject_device(hd, p, W, None, 0, z, W, None, 0, None) == _capi.SGM_OK   # skipped: no pitch
            refused(L.sgm_stage_reproject(hd, None, x, z, u), "NULL disparity map")
            refused(L.sgm_stage_reproject(hd, p, None, None, None), "all three products")
            sg.check()
            # the handle's products
            ptr, pitch = ctypes.c_void_p(), ctypes.c_int()
            refused(L.sgm_get_reprojected(hd, 3, ctypes.byref(ptr), ctypes.byref(pitch)), "one SGM_REPROJECT_")
            refused(L.sgm_get_reprojected(hd, 0, ctypes.byref(ptr), ctypes.byref(pitch)), "one SGM_REPROJECT_")
            refused(L.sgm_get_reprojected(hd, DEPTH16, ctypes.byref(ptr), ctypes.byref(pitch)), "not in the outputs")
            refused(L.sgm_get_reprojected(hd, XYZ, None, ctypes.byref(pitch)), "NULL")
            refused(L.sgm_get_reprojected(hd, XYZ, ctypes.byref(ptr), None), "NULL")
            refused(L.sgm_stage_reprojected(hd, XYZ, None), "NULL")
            if sg is sgm:                                # before any frame
                refused(L.sgm_get_reprojected(hd, XYZ, ctypes.byref(ptr), ctypes.byref(pitch)), "no frame")
                sg.process(*plane_pair(h, w))
                sg.get_xyz()
                sg.set_reproject(q, outputs=("xyz",))    # set again: the old frame's products are gone
                with pytest.raises(SGMError, match="no frame"):
                    sg.get_xyz()
            else:                                        # an aux_only handle runs no frames
                refused(L.sgm_get_reprojected(hd, XYZ, ctypes.byref(ptr), ctypes.byref(pitch)), "not in the outputs")
        with pytest.raises(ValueError):
            sgm.set_reproject(q[:15])
        with pytest.raises(ValueError):
            sgm.set_reproject(q, outputs=("cloud",))
        with pytest.raises(ValueError):
            sgm.reproject(np.zeros((H, W + 1), np.float32))
    cam = _capi.Camera(700.0, 700.0, 320.0, 240.0, 0.0, 0.0)
    out = (ctypes.c_double * 16)()
    assert _capi.lib().sgm_camera_q(ctypes.byref(cam), out) == _capi.SGM_ERR_INVALID_ARG   # 1 / baseline
    assert _capi.lib().sgm_camera_q(None, out) == _capi.SGM_ERR_INVALID_ARG
    assert _capi.lib().sgm_camera_q(ctypes.byref(cam), None) == _capi.SGM_ERR_INVALID_ARG
