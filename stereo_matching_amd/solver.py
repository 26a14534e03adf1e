"""Python mirror of the reference's Solver/SGM class surface.

Reference: inc/Solver.h:23-70 and inc/SGM.h:10-26 (constructor SGM(h, w, s, d),
process(l, r[, sky, sky_beta]), get_disp()).  Every call goes through the
C-ABI of libsgm_hip.so; nothing here computes disparities itself.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi
from ._capi import check, lib


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# hipStreamLegacy (hip_runtime_api.h): the legacy default ("null") stream
_HIP_STREAM_LEGACY = 1


def _stream(stream):
    """The hipStream_t the C-ABI gets: None -> NULL, the handle's own stream
    (non-blocking: NOT ordered with the null stream); 0 -> hipStreamLegacy,
    the legacy default stream (torch's default stream reports cuda_stream 0,
    so passing torch.cuda.current_stream().cuda_stream orders the call with
    torch's work either way); anything else is a hipStream_t handle."""
    if stream is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(_HIP_STREAM_LEGACY if stream == 0 else stream)


def _u8(a, shape, what):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape != shape:
        raise ValueError(f"{what}: expected shape {shape}, got {a.shape}")
    return a


_FMT_NAMES = {v: k for k, v in _capi.PIX_FORMATS.items()}


def _fmt_code(fmt) -> int:
    """SGM_PIX_* of a format name; an integer passes through (the library
    refuses one it does not know)."""
    if isinstance(fmt, str):
        if fmt not in _capi.PIX_FORMATS:
            raise ValueError(f"input format must be one of {sorted(_capi.PIX_FORMATS)}, got {fmt!r}")
        return _capi.PIX_FORMATS[fmt]
    if fmt is None:
        return 0
    return int(fmt)


class SGM:
    """Semi-global matcher on one MI355X (HIP device `device`).

    Mirrors ``SGM(int h, int w, int s, int d)`` (src/SGM.cpp:4-29).  The
    reference asserts s in {1, 2} and d in {32, 64, 128} (Solver.cpp:6-10);
    here d = 256 is also accepted and invalid arguments raise SGMError.
    """

    def __init__(self, h: int, w: int, s: int = 1, d: int = 128, *, device: int = 0,
                 blur: bool = True, views: int = 2, p1: int = 10, p2: int = 100,
                 uniqueness: float = 0.7, lr_max_diff: float = 1.0, post_filter: bool = False,
                 lk_refine: bool = False, sky_detect: bool = False,
                 aux_only: bool = False, view: str = "left", paths: int = 8,
                 post_filter_launches: int = 0, confidence: bool = False, min_disp: int = 0,
                 input_size=None, rectify=None, input_format: str = "gray8", reproject=None,
                 cost: str = "census", window=None, volume_filter=None, weighted: bool = False,
                 fill: str = "off", _solver: int = _capi.SGM_SOLVER_SGM):
        self._lib = lib()
        # cost ("census" | "sad" | "ssd" | "ct"): the matching cost of every frame
        # (set_cost): the 7x9 census, or the reference's SAD / SSD window cost or
        # its CT (Solver::build_dsi over cost.cpp:4-96) with no cost filters after it
        if cost not in _capi.COST_KINDS:
            raise ValueError(f"cost must be one of {sorted(_capi.COST_KINDS)}, got {cost!r}")
        # paths (8 | 4): 4 is the reference's USE_8_PATH = false (inc/SGM.h:7):
        # S = ((L1+L2)+L3)+L4 per view, no diagonal paths (SGM.cpp:387-390)
        # (0 means 8, as in a zero-initialised sgm_params)
        if paths not in (0, 4, 8):
            raise ValueError(f"paths must be 4 or 8, got {paths!r}")
        p = _capi.default_params(h, w, s, d)
        p.paths = paths
        p.blur = int(bool(blur))
        p.views = views
        # post_filter: process_device's output is post_filter()ed on the GPU
        # (SGM.cpp:821); process() keeps the LR map and get_disp() filters it
        p.post_filter = int(bool(post_filter))
        # lk_refine: ... then LKRefine (SGM.cpp:824, commented out in the reference)
        p.lk_refine = int(bool(lk_refine))
        # sky_detect: masks from SkyAreaDetector::detect on the GPU (node.cpp:80-93)
        p.sky_detect = int(bool(sky_detect))
        p.solver = _solver
        # aux_only: side stages only (sky, post_filter, LKRefine, colormap, cloud)
        p.aux_only = int(bool(aux_only))
        # view ("left" | "right", views=1 only): the right view alone (SGM.cpp:448-801),
        # for a pair split over two GPUs that meet in lr_check_device
        if view not in ("left", "right"):
            raise ValueError(f"view must be 'left' or 'right', got {view!r}")
        p.view = _capi.SGM_VIEW_RIGHT if view == "right" else _capi.SGM_VIEW_LEFT
        p.p1, p.p2 = p1, p2
        p.uniqueness, p.lr_max_diff = uniqueness, lr_max_diff
        self.params = p
        self.h, self.w, self.scale, self.max_disp = h, w, s, d
        self.rows, self.cols = h // s, w // s
        self.min_disp = int(min_disp)
        handle = ctypes.c_void_p()
        check(self._lib.sgm_create(ctypes.byref(p), device, ctypes.byref(handle)))
        self._h = handle
        # min_disp (sgm_set_min_disp): search disparities [min_disp, min_disp + d)
        # instead of [0, d).  Every map is in true disparity, invalid = d +
        # min_disp + 1 (invalid_disp); a sky pixel reports min_disp.  A multiple
        # of s, >= 0; side-stage handles (aux_only) of such maps take the same value
        try:
            if self.min_disp:
                check(self._lib.sgm_set_min_disp(handle, self.min_disp), handle)
            inv = ctypes.c_int()
            check(self._lib.sgm_get_invalid_disp(handle, ctypes.byref(inv)), handle)
        except Exception:
            self.close()
            raise
        self.invalid_disp = inv.value  # d + min_disp + 1
        self.device = device
        self._lr = np.full((self.rows, self.cols), self.invalid_disp, np.float32)
        self._raw = np.zeros((self.rows, self.cols), np.uint16)
        self._final = None
        self._filled = False  # set_fill: frames return the filled map
        # post_filter_launches: the median fill's fixed launch budget
        # (set_post_filter_launches); 0 = the adaptive, host-synchronised fill
        # confidence: every frame also keeps its per-pixel uniqueness ratio
        # (set_confidence / get_confidence)
        # input_size = (h0, w0): process() takes h0 x w0 images and the frame
        # resizes them to h x w first, as the node does (node.cpp:75-76;
        # set_input_size)
        # rectify = (src_h, src_w, mapx_l, mapy_l, mapx_r, mapy_r): process()
        # takes raw src_h x src_w camera images and the frame remaps them
        # through the h x w float maps first (set_rectify); not with input_size
        # input_format ("gray8" | "bgr8" | "rgb8" | "bgra8" | "rgba8"): process()
        # takes (in_h, in_w, channels) colour images and the frame converts
        # them to grey on the GPU first, inside the resize or the remap when one
        # is set (set_input_format)
        # reproject = Q (16 values, stereoRectify's 4 x 4 matrix row-major): every
        # frame also writes the organized XYZ image and the depth image of its
        # final map (set_reproject; get_xyz(), get_depth())
        self.in_h, self.in_w, self.in_ch = h, w, 1
        try:
            if _fmt_code(input_format):
                self.set_input_format(input_format)
            if post_filter_launches:
                self.set_post_filter_launches(post_filter_launches)
            if confidence:
                self.set_confidence(True)
            if input_size is not None:
                self.set_input_size(*input_size)
            if rectify is not None:
                self.set_rectify(*rectify)
            if reproject is not None:
                self.set_reproject(reproject)
            if cost != "census":
                self.set_cost(cost)
            # window = (win_h, win_w): the census's and the SAD / SSD costs' window, the
            # reference's WIN_H, WIN_W before the division by s (set_window); None: (7, 9)
            if window is not None:
                self.set_window(*window)
            # weighted: the reference's WEIGHTED_COST on that window (set_weighted), applied
            # after it, so that SGM(..., s=2, window=(14, 18), weighted=True) is accepted
            if weighted:
                self.set_weighted(True)
            # volume_filter = (horizontal, vertical): the reference's cost filters on every
            # volume frame (aggregate(), SAD / SSD frames; set_volume_filter); None: off
            if volume_filter is not None:
                self.set_volume_filter(*volume_filter)
            # fill ("off" | "background" | "interpolate"): every frame ends its maps with the
            # occlusion-aware hole filling (set_fill)
            if fill != "off":
                self.set_fill(fill)
        except Exception:
            self.close()
            raise

    # ---------------------------------------------------------- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.sgm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def device_bytes(self) -> int:
        return int(self._lib.sgm_device_bytes(self._h))

    @property
    def stream(self) -> int:
        """The handle's own stream (sgm_get_stream), as an integer hipStream_t
        for torch.cuda.ExternalStream: work on it is ordered with the calls
        made with stream=None, and those calls record no events."""
        return int(self._lib.sgm_get_stream(self._h) or 0)

    # ------------------------------------------------------------ process
    def process(self, img_l, img_r, sky_mask=None, sky_mask_beta=None) -> None:
        """SGM::process (src/SGM.cpp:32-826, sky overload :829-834)."""
        shape = (self.in_h, self.in_w) if self.in_ch == 1 else (self.in_h, self.in_w, self.in_ch)
        l = _u8(img_l, shape, "img_l")
        r = _u8(img_r, shape, "img_r")
        sl = None if sky_mask is None or np.size(sky_mask) == 0 else \
            _u8(sky_mask, (self.rows, self.cols), "sky_mask")
        sr = None if sky_mask_beta is None or np.size(sky_mask_beta) == 0 else \
            _u8(sky_mask_beta, (self.rows, self.cols), "sky_mask_beta")
        # Fresh output maps per frame: the arrays handed out by get_disp() /
        # get_lr_disp() / get_raw_disp() for one frame are never overwritten
        # by the next (the reference's get_disp() reference is valid until the
        # next process(), inc/Solver.h:36; a copy-free handle-owned buffer
        # would alias the previous frame's result).
        out = np.empty((self.rows, self.cols), np.float32)
        raw = np.empty((self.rows, self.cols), np.uint16)
        check(self._lib.sgm_process(self._h, _ptr(l), _ptr(r), self.in_w * self.in_ch, _ptr(sl), _ptr(sr),
                                    self.cols, _ptr(out), self.cols, _ptr(raw)),
              self._h)
        self._raw = raw
        # (with fill set the frame's map is filled, its last map stage: the final map)
        if self.params.post_filter or self.params.lk_refine or self._filled:  # sgm_process returned the final map
            self._final, self._lr = out, None
        else:
            self._final, self._lr = None, out

    def process_device(self, d_left: int, d_right: int, d_out: int, *, pitch: int | None = None,
                       d_sky_l: int = 0, d_sky_r: int = 0, sky_pitch: int | None = None,
                       out_pitch: int | None = None, d_raw: int = 0, stream: int | None = None) -> None:
        """Device-pointer variant (sgm_process_device): enqueue on `stream`
        (None: the handle's own stream; a torch stream's `cuda_stream`,
        including 0 for torch's default stream: that stream).  pitch: bytes per
        image row, by default in_w x the input format's bytes per pixel."""
        check(self._lib.sgm_process_device(
            self._h, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), pitch or self.in_w * self.in_ch,
            ctypes.c_void_p(d_sky_l or None), ctypes.c_void_p(d_sky_r or None),
            sky_pitch or self.cols, ctypes.c_void_p(d_out), out_pitch or self.cols,
            ctypes.c_void_p(d_raw or None), _stream(stream)), self._h)

    # ------------------------------------------------------- input resize
    def set_input_size(self, rows: int, cols: int) -> None:
        """sgm_set_input_size: process() / process_device() take rows x cols
        images, and the frame's first launch resizes them to h x w (the node's
        cv::resize, node.cpp:75-76, in its pinned fixed-point form); (0, 0)
        switches it off.  Not inside stream capture; re-capture graphs."""
        self._set_input(self._lib.sgm_set_input_size, int(rows), int(cols))

    def _set_input(self, setter, *args) -> None:
        """One call of an input stage's setter, then _sync_input_shape(),
        whether or not the call raised."""
        try:
            check(setter(self._h, *args), self._h)
        finally:
            self._sync_input_shape()

    def _input_image(self, stage, view: int) -> np.ndarray:
        """The last frame's full-size grey image of `view` as `stage`
        (sgm_stage_resized, sgm_stage_rectified or sgm_stage_input_gray)
        downloads it: h x w uint8."""
        out = np.empty((self.h, self.w), np.uint8)
        check(stage(self._h, int(view), _ptr(out)), self._h)
        return out

    def _sync_input_shape(self) -> None:
        """in_h, in_w: the shape of the images process() takes, read back from
        the handle -- the input size or the rectification maps' source size,
        whichever is set (never both), else h x w.  After every setter call,
        a failed one included: switching the inactive stage off changes
        nothing, and a failed replacement of maps leaves them off."""
        rows, cols = self.input_size
        if not rows:
            rows, cols = self.rectify_size
        self.in_h, self.in_w = (rows, cols) if rows else (self.h, self.w)
        self.in_ch = _capi.PIX_BYTES[_fmt_code(self.input_format)]

    @property
    def input_size(self):
        """(rows, cols) of the images process() takes; (0, 0): the full size."""
        r, c = ctypes.c_int(), ctypes.c_int()
        check(self._lib.sgm_get_input_size(self._h, ctypes.byref(r), ctypes.byref(c)), self._h)
        return r.value, c.value

    def resize(self, img, pitch: int | None = None) -> np.ndarray:
        """cv::resize(img, Size(w, h)) of a 2-D u8 image of any size on the GPU
        (sgm_stage_resize): h x w uint8.  pitch: bytes per row of `img` when it
        is a padded buffer (its last axis is then the pitch)."""
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError(f"img: expected a 2-D image, got shape {a.shape}")
        out = np.empty((self.h, self.w), np.uint8)
        check(self._lib.sgm_stage_resize(self._h, _ptr(a), a.shape[0], a.shape[1],
                                         pitch or a.shape[1], _ptr(out)), self._h)
        return out

    def resize_device(self, d_src: int, src_rows: int, src_cols: int, d_dst: int, *,
                      src_pitch: int | None = None, dst_pitch: int | None = None,
                      stream: int | None = None) -> None:
        """The same on device buffers (sgm_resize_device: one launch, enqueue
        only, capturable)."""
        check(self._lib.sgm_resize_device(
            self._h, ctypes.c_void_p(d_src or None), int(src_rows), int(src_cols),
            src_cols if src_pitch is None else src_pitch, ctypes.c_void_p(d_dst or None),
            self.w if dst_pitch is None else dst_pitch, _stream(stream)), self._h)

    def get_resized(self, view: int = 0) -> np.ndarray:
        """The last frame's resized image of `view` (0 = left, 1 = right):
        h x w uint8, a host copy (sgm_stage_resized)."""
        return self._input_image(self._lib.sgm_stage_resized, view)

    # ------------------------------------------------------ rectification
    def set_rectify(self, src_rows: int, src_cols: int, mapx_l=None, mapy_l=None,
                    mapx_r=None, mapy_r=None) -> None:
        """sgm_set_rectify: process() / process_device() take raw src_rows x
        src_cols camera images, and the frame's first launch remaps both
        through the h x w float32 maps (cv::initUndistortRectifyMap's CV_32FC1
        outputs; cv::convertMaps + cv::remap INTER_LINEAR, BORDER_CONSTANT 0 in
        their pinned fixed-point form).  (0, 0) with no maps
        switches it off.  Not inside stream capture; re-capture graphs."""
        maps = []
        for name, m in (("mapx_l", mapx_l), ("mapy_l", mapy_l), ("mapx_r", mapx_r), ("mapy_r", mapy_r)):
            if m is not None:
                m = np.ascontiguousarray(m, dtype=np.float32)
                if m.shape != (self.h, self.w):
                    raise ValueError(f"{name}: expected shape {(self.h, self.w)}, got {m.shape}")
            maps.append(m)
        self._set_input(self._lib.sgm_set_rectify, int(src_rows), int(src_cols), *(_ptr(m) for m in maps),
                        self.w)

    @property
    def rectify_size(self):
        """(rows, cols) of the raw images the maps read; (0, 0): no maps set."""
        r, c = ctypes.c_int(), ctypes.c_int()
        check(self._lib.sgm_get_rectify(self._h, ctypes.byref(r), ctypes.byref(c)), self._h)
        return r.value, c.value

    def remap(self, img, view: int = 0, pitch: int | None = None) -> np.ndarray:
        """`view`'s (0 = left, 1 = right) raw image rectified on the GPU
        (sgm_stage_remap): h x w uint8.  pitch: bytes per row of `img` when it
        is a padded buffer (its last axis is then the pitch)."""
        rows, cols = self.rectify_size
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if rows and (a.ndim != 2 or a.shape[0] != rows or a.shape[1] != (pitch or cols)):
            raise ValueError(f"img: expected shape {(rows, pitch or cols)}, got {a.shape}")
        out = np.empty((self.h, self.w), np.uint8)
        check(self._lib.sgm_stage_remap(self._h, int(view), _ptr(a), pitch or cols, _ptr(out)), self._h)
        return out

    def remap_device(self, d_src: int, d_dst: int, view: int = 0, *, src_pitch: int | None = None,
                     dst_pitch: int | None = None, stream: int | None = None) -> None:
        """The same on device buffers (sgm_remap_device: one launch, enqueue
        only, capturable)."""
        check(self._lib.sgm_remap_device(
            self._h, int(view), ctypes.c_void_p(d_src or None),
            self.rectify_size[1] if src_pitch is None else src_pitch, ctypes.c_void_p(d_dst or None),
            self.w if dst_pitch is None else dst_pitch, _stream(stream)), self._h)

    def rectified(self, view: int = 0) -> np.ndarray:
        """The last frame's rectified image of `view` (0 = left, 1 = right):
        h x w uint8, a host copy (sgm_stage_rectified)."""
        return self._input_image(self._lib.sgm_stage_rectified, view)

    def rectify_valid(self, view: int = 0) -> np.ndarray:
        """`view`'s valid mask (sgm_stage_rectify_valid): h x w uint8, 255
        where all four taps of the pixel lie inside the raw image, else 0."""
        out = np.empty((self.h, self.w), np.uint8)
        check(self._lib.sgm_stage_rectify_valid(self._h, int(view), _ptr(out)), self._h)
        return out

    # ------------------------------------------------------- colour input
    def set_input_format(self, fmt: str) -> None:
        """sgm_set_input_format: process() / process_device() take images of
        the pixel format `fmt` ("bgr8", "rgb8", "bgra8", "rgba8": interleaved,
        (in_h, in_w, 3 or 4) arrays; "gray8": off, one channel again).  The
        frame's first launch converts them, Y = (4899 R + 9617 G + 1868 B +
        8192) >> 14: inside the resize or the remap when one is
        set, else as one launch of its own.  Not inside stream capture;
        re-capture graphs."""
        self._set_input(self._lib.sgm_set_input_format, _fmt_code(fmt))

    @property
    def input_format(self) -> str:
        """The pixel format of the images process() takes ("gray8": one channel)."""
        f = ctypes.c_int()
        check(self._lib.sgm_get_input_format(self._h, ctypes.byref(f)), self._h)
        return _FMT_NAMES[f.value]

    def gray(self, img, fmt: str) -> np.ndarray:
        """A colour image of any size as grey on the GPU (sgm_stage_gray):
        (rows, cols, 3 or 4) uint8 -> rows x cols uint8."""
        code = _fmt_code(fmt)
        a = np.ascontiguousarray(img, dtype=np.uint8)
        bpp = _capi.PIX_BYTES[code]
        if a.ndim != 3 or a.shape[2] != bpp:
            raise ValueError(f"img: expected a (rows, cols, {bpp}) image for {fmt!r}, got shape {a.shape}")
        out = np.empty(a.shape[:2], np.uint8)
        check(self._lib.sgm_stage_gray(self._h, code, _ptr(a), a.shape[0], a.shape[1],
                                       a.shape[1] * bpp, _ptr(out)), self._h)
        return out

    def gray_device(self, fmt: str, d_src: int, rows: int, cols: int, d_dst: int, *,
                    src_pitch: int | None = None, dst_pitch: int | None = None,
                    stream: int | None = None) -> None:
        """The same on device buffers (sgm_gray_device: one launch, enqueue
        only, capturable)."""
        code = _fmt_code(fmt)
        check(self._lib.sgm_gray_device(
            self._h, code, ctypes.c_void_p(d_src or None), int(rows), int(cols),
            cols * _capi.PIX_BYTES.get(code, 1) if src_pitch is None else src_pitch,
            ctypes.c_void_p(d_dst or None), cols if dst_pitch is None else dst_pitch,
            _stream(stream)), self._h)

    def input_gray(self, view: int = 0) -> np.ndarray:
        """The last frame's grey image of `view` (0 = left, 1 = right) on a
        handle with a colour format: h x w uint8, a host copy
        (sgm_stage_input_gray).  What the point cloud and show_disp read."""
        return self._input_image(self._lib.sgm_stage_input_gray, view)

    # ------------------------------------------------------- reprojection
    def set_reproject(self, q, outputs=("xyz", "depth"), max_range: float = 0.0,
                      depth_scale: float = 1000.0) -> None:
        """sgm_set_reproject: every later frame ends with one launch more that
        reprojects its final map through Q (16 values, stereoRectify's 4 x 4
        matrix row-major) into the products named in `outputs`
        ("xyz", "depth", "depth16", or the OR of their bits): get_xyz(),
        get_depth(), get_depth16().  max_range > 0: pixels with Z outside
        (0, max_range] are missing; depth16 = rint(Z * depth_scale).
        set_reproject(None) switches it off.  An aux_only handle may pass
        outputs=() and keep Q for reproject() / reproject_device() alone.  Not
        inside stream capture; re-capture graphs."""
        if q is None:
            check(self._lib.sgm_set_reproject(self._h, None), self._h)
            return
        qa = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
        if qa.size != 16:
            raise ValueError(f"q: expected 16 values (a 4 x 4 matrix), got {qa.size}")
        if isinstance(outputs, str):
            outputs = (outputs,)
        bits = 0
        for o in ([outputs] if isinstance(outputs, int) else outputs):
            if isinstance(o, str) and o not in _capi.REPROJECT_OUTPUTS:
                raise ValueError(f"outputs must name {sorted(_capi.REPROJECT_OUTPUTS)}, got {o!r}")
            bits |= _capi.REPROJECT_OUTPUTS[o] if isinstance(o, str) else int(o)
        r = _capi.Reproject((ctypes.c_double * 16)(*qa), bits, max_range, depth_scale)
        check(self._lib.sgm_set_reproject(self._h, ctypes.byref(r)), self._h)

    @property
    def reprojection(self):
        """(Q as a 4 x 4 float64 array, outputs bits, max_range, depth_scale) as
        the handle holds them; None while reprojection is off."""
        r = _capi.Reproject()
        check(self._lib.sgm_get_reproject(self._h, ctypes.byref(r)), self._h)
        if not r.outputs and not any(r.q):
            return None
        return np.array(list(r.q), np.float64).reshape(4, 4), r.outputs, r.max_range, r.depth_scale

    def reproject(self, disp, outputs=("xyz", "depth", "depth16")) -> dict:
        """A rows x cols map reprojected on the GPU through the Q set
        (sgm_stage_reproject; synchronous): {"xyz": rows x cols x 3 float32,
        "depth": rows x cols float32, "depth16": rows x cols uint16} for the
        names in `outputs`.  Missing pixels hold NaN (0 in depth16)."""
        f = np.ascontiguousarray(disp, dtype=np.float32)
        if f.shape != (self.rows, self.cols):
            raise ValueError(f"disp: expected shape {(self.rows, self.cols)}, got {f.shape}")
        shapes = {"xyz": ((self.rows, self.cols, 3), np.float32), "depth": ((self.rows, self.cols), np.float32),
                  "depth16": ((self.rows, self.cols), np.uint16)}
        for o in outputs:
            if o not in shapes:
                raise ValueError(f"outputs must name {sorted(shapes)}, got {o!r}")
        out = {o: np.empty(*shapes[o]) for o in outputs}
        check(self._lib.sgm_stage_reproject(self._h, _ptr(f), _ptr(out.get("xyz")), _ptr(out.get("depth")),
                                            _ptr(out.get("depth16"))), self._h)
        return out

    def reproject_device(self, d_disp: int, *, d_xyz: int = 0, d_depth: int = 0, d_depth16: int = 0,
                         pitch: int | None = None, xyz_pitch: int | None = None,
                         depth_pitch: int | None = None, depth16_pitch: int | None = None,
                         stream: int | None = None) -> None:
        """The same on device buffers (sgm_reproject_device: one launch,
        enqueue only, capturable); a product whose pointer is 0 is skipped;
        pitches in elements of each buffer's type."""
        check(self._lib.sgm_reproject_device(
            self._h, ctypes.c_void_p(d_disp or None), self.cols if pitch is None else pitch,
            ctypes.c_void_p(d_xyz or None), 3 * self.cols if xyz_pitch is None else xyz_pitch,
            ctypes.c_void_p(d_depth or None), self.cols if depth_pitch is None else depth_pitch,
            ctypes.c_void_p(d_depth16 or None), self.cols if depth16_pitch is None else depth16_pitch,
            _stream(stream)), self._h)

    def _reprojected(self, which: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        check(self._lib.sgm_stage_reprojected(self._h, which, _ptr(out)), self._h)
        return out

    def get_xyz(self) -> np.ndarray:
        """The last frame's organized XYZ image: rows x cols x 3 float32, NaN
        where missing; a host copy (sgm_stage_reprojected)."""
        return self._reprojected(_capi.REPROJECT_OUTPUTS["xyz"], (self.rows, self.cols, 3), np.float32)

    def get_depth(self) -> np.ndarray:
        """The last frame's depth image Z: rows x cols float32, NaN where missing."""
        return self._reprojected(_capi.REPROJECT_OUTPUTS["depth"], (self.rows, self.cols), np.float32)

    def get_depth16(self) -> np.ndarray:
        """The last frame's 16-bit depth image rint(Z * depth_scale): rows x
        cols uint16, 0 where missing or outside [1, 65535]."""
        return self._reprojected(_capi.REPROJECT_OUTPUTS["depth16"], (self.rows, self.cols), np.uint16)

    @staticmethod
    def camera_q(fx, fy, cx, cy, baseline) -> np.ndarray:
        """sgm_camera_q: the pinhole Q [1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0
        1/baseline 0] with f = (fx + fy) / 2, as a 4 x 4 float64 array.  Not
        the node's cloud (point_cloud): one focal length and no 1e-6."""
        cam = _capi.Camera(fx, fy, cx, cy, baseline, 0.0)
        q = (ctypes.c_double * 16)()
        check(lib().sgm_camera_q(ctypes.byref(cam), q))
        return np.array(list(q), np.float64).reshape(4, 4)

    # ------------------------------------------------ a caller's cost volume
    def _volume(self, cost, layout):
        """(torch, sgm_volume) of a torch device cost volume: shape
        (rows, cols, D), or (D, rows, cols) with layout="dhw"; strides as the
        tensor has them (nothing is made contiguous)."""
        if isinstance(cost, np.ndarray) or not (hasattr(cost, "data_ptr") and hasattr(cost, "stride")):
            raise TypeError("cost must be a torch device tensor; for a host numpy H x W x D float32 "
                            "volume use stage_aggregate()")
        import torch
        if not cost.is_cuda or cost.device.index != self.device:
            raise ValueError(f"cost must live on the handle's device cuda:{self.device}, got {cost.device}")
        if cost.dtype not in (torch.float32, torch.float16):
            raise TypeError(f"cost must be float32 or float16, got {cost.dtype}")
        hwd, dhw = (self.rows, self.cols, self.max_disp), (self.max_disp, self.rows, self.cols)
        shape = tuple(cost.shape)
        if layout is None:
            if shape == hwd and shape == dhw:
                raise ValueError(f"cost of shape {shape} reads as (rows, cols, D) and as (D, rows, cols): "
                                 "pass layout='hwd' or layout='dhw'")
            layout = "hwd" if shape == hwd else "dhw" if shape == dhw else None
            if layout is None:
                raise ValueError(f"cost: expected shape {hwd} or {dhw}, got {shape}")
        elif layout not in ("hwd", "dhw"):
            raise ValueError(f"layout must be 'hwd', 'dhw' or None, got {layout!r}")
        elif shape != (hwd if layout == "hwd" else dhw):
            raise ValueError(f"cost: expected shape {hwd if layout == 'hwd' else dhw} for layout "
                             f"{layout!r}, got {shape}")
        st = cost.stride()
        sr, sc, sd = st if layout == "hwd" else (st[1], st[2], st[0])
        vol = _capi.Volume(cost.data_ptr(), _capi.SGM_VOL_F16 if cost.dtype == torch.float16 else _capi.SGM_VOL_F32,
                           sr, sc, sd)
        return torch, vol

    def _on_torch_stream(self, torch, tensor, stream, call) -> None:
        """call(stream argument) ordered on torch's work.  stream: a
        hipStream_t handle (e.g. a torch stream's cuda_stream), or None for the
        tensor's device's current torch stream, so that the call is ordered
        after the tensor's producer and before what torch enqueues next.
        torch's default stream has no handle of its own: its cuda_stream is 0,
        the legacy stream, which the two volume entry points refuse
        (sgm_hip.h: a later call on another stream would wait on an event
        recorded on it, and that wait crashed the process).  For it -- current
        or passed as stream=0 -- the call runs on the handle's own stream
        between two stream waits, with the same ordering."""
        if stream is None:
            stream = torch.cuda.current_stream(tensor.device).cuda_stream
        if stream:
            call(_stream(stream))
            return
        cur = torch.cuda.default_stream(tensor.device)
        own = torch.cuda.ExternalStream(self.stream, device=tensor.device)
        own.wait_stream(cur)
        call(_stream(None))
        cur.wait_stream(own)

    def aggregate(self, cost, *, layout=None, out=None, raw=None, stream=None):
        """sgm_aggregate_device: a caller's cost volume (a torch device tensor,
        float32 or float16, of shape (rows, cols, D), or (D, rows, cols) with
        layout="dhw"; any strides with a unit column or disparity stride, e.g.
        one item of a [B, D, H, W] batch) through the frame from the cost
        volume on: path aggregation, WTA, sub-pixel, the LR check (views = 2,
        against the right view's volume derived from this one), post_filter,
        reprojection and confidence as the handle is set up.  Returns `out`, a
        torch float32 (rows, cols) tensor on the same device (allocated when
        None); raw: an optional (rows, cols) int16/uint16 tensor for the left
        raw WTA map.  Enqueued on `stream` (default: the device's current torch
        stream; 0: torch's default stream); get_confidence(), get_xyz(),
        get_depth() and check() work after it as after a frame.  With an
        explicit `stream` other than the one the tensors were allocated on,
        the caller keeps `cost`, `out` and `raw` alive and ordered until the
        call's work is done (tensor.record_stream), as for any torch tensor
        used on a side stream.  Costs: finite, in [0, 999999]."""
        torch, vol = self._volume(cost, layout)
        if out is None:
            out = torch.empty((self.rows, self.cols), dtype=torch.float32, device=cost.device)
        if (out.dtype != torch.float32 or tuple(out.shape) != (self.rows, self.cols) or out.device != cost.device
                or out.stride(1) != 1):
            raise ValueError(f"out must be a float32 {(self.rows, self.cols)} tensor on {cost.device} with unit "
                             "column stride")
        if raw is not None and (raw.element_size() != 2 or tuple(raw.shape) != (self.rows, self.cols)
                                or raw.device != cost.device or not raw.is_contiguous()):
            raise ValueError(f"raw must be a contiguous 16-bit {(self.rows, self.cols)} tensor on {cost.device}")
        self._on_torch_stream(torch, cost, stream, lambda st: check(self._lib.sgm_aggregate_device(
            self._h, ctypes.byref(vol), ctypes.c_void_p(out.data_ptr()), out.stride(0),
            ctypes.c_void_p(raw.data_ptr() if raw is not None else None), st), self._h))
        return out

    def import_volume(self, cost, view: int = 0, *, layout=None, out=None, stream=None):
        """sgm_volume_import_device: the dense float32 (rows, cols, D) volume of
        `view` (0 = left: the re-layout; 1 = right: C_L[i, min(j + (d +
        min_disp) // scale, cols - 1), d]) of a torch device cost volume, as a
        torch tensor on the same device (`out`, allocated when None).  One
        launch on `stream` (default: the device's current torch stream; the
        tensors' lifetime on another stream is the caller's, as for
        aggregate)."""
        torch, vol = self._volume(cost, layout)
        shape = (self.rows, self.cols, self.max_disp)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=cost.device)
        if (out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != cost.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 {shape} tensor on {cost.device}")
        self._on_torch_stream(torch, cost, stream, lambda st: check(self._lib.sgm_volume_import_device(
            self._h, ctypes.byref(vol), int(view), ctypes.c_void_p(out.data_ptr()), st), self._h))
        return out

    # ------------------------------------------------------ the matching cost
    def set_cost(self, kind: str) -> None:
        """sgm_set_cost: "census" (the default), "sad", "ssd" or "ct" (CT,
        build_dsi's own per-disparity census: DESIGN.md 5s).  With a window
        cost every later frame builds the reference's build_dsi volume (one
        launch), derives the right view's from it and runs what aggregate()
        runs; the cost filters run only when set_volume_filter says so, and sky
        masks are refused.  Re-capture graphs afterwards."""
        if kind not in _capi.COST_KINDS:
            raise ValueError(f"cost must be one of {sorted(_capi.COST_KINDS)}, got {kind!r}")
        check(self._lib.sgm_set_cost(self._h, _capi.COST_KINDS[kind]), self._h)

    @property
    def cost(self) -> str:
        """sgm_get_cost, by name."""
        k = ctypes.c_int()
        check(self._lib.sgm_get_cost(self._h, ctypes.byref(k)), self._h)
        return {v: n for n, v in _capi.COST_KINDS.items()}[k.value]

    # --------------------------------- the cost filters on a finished volume
    @staticmethod
    def _filter_bits(horizontal, vertical) -> int:
        return (_capi.SGM_FILTER_H if horizontal else 0) | (_capi.SGM_FILTER_V if vertical else 0)

    def set_volume_filter(self, horizontal: bool = True, vertical: bool = True) -> None:
        """sgm_set_volume_filter: the reference's cost_horizontal_filter(5 // s)
        and cost_vertical_filter(3 // s) (Solver.cpp:296-368) on each view's
        volume in every later volume frame: aggregate() and the frames of
        "sad" / "ssd" handles, after the import or producer launch and after
        the right view's derivation from the raw left volume.  Both False:
        off, the default.  Census frames ignore it (they filter as ever).
        Allocates nothing; call it outside stream capture and re-capture
        graphs afterwards.  BM, aux_only and view="right" handles raise
        SGMError."""
        check(self._lib.sgm_set_volume_filter(self._h, self._filter_bits(horizontal, vertical)), self._h)

    @property
    def volume_filter(self):
        """sgm_get_volume_filter: (horizontal, vertical)."""
        f = ctypes.c_int()
        check(self._lib.sgm_get_volume_filter(self._h, ctypes.byref(f)), self._h)
        return bool(f.value & _capi.SGM_FILTER_H), bool(f.value & _capi.SGM_FILTER_V)

    def filter_volume(self, cost, horizontal: bool = True, vertical: bool = True, stream=None):
        """sgm_filter_volume_device: the cost filters, in place, on a contiguous
        float32 torch device tensor of shape (rows, cols, D), whatever
        set_volume_filter says.  Enqueued on `stream` (default: the device's
        current torch stream; torch's default stream goes through the handle's
        own, as for aggregate).  Returns `cost`.  Filtered this way a volume
        goes into aggregate() of a views=1 handle whose setting is off and
        gives the maps the setting gives."""
        if isinstance(cost, np.ndarray) or not hasattr(cost, "data_ptr"):
            raise TypeError("cost must be a torch device tensor; for a host numpy volume use stage_filter_volume()")
        import torch
        shape = (self.rows, self.cols, self.max_disp)
        if not cost.is_cuda or cost.device.index != self.device:
            raise ValueError(f"cost must live on the handle's device cuda:{self.device}, got {cost.device}")
        if cost.dtype != torch.float32 or tuple(cost.shape) != shape or not cost.is_contiguous():
            raise ValueError(f"cost must be a contiguous float32 {shape} tensor")
        bits = self._filter_bits(horizontal, vertical)
        self._on_torch_stream(torch, cost, stream, lambda st: check(self._lib.sgm_filter_volume_device(
            self._h, ctypes.c_void_p(cost.data_ptr()), bits, st), self._h))
        return cost

    def stage_filter_volume(self, cost, horizontal: bool = True, vertical: bool = True) -> np.ndarray:
        """sgm_stage_filter_volume: the same filters on a host numpy (rows,
        cols, D) float32 volume; returns the filtered copy (tests)."""
        c = np.array(cost, np.float32, order="C", copy=True)
        if c.shape != (self.rows, self.cols, self.max_disp):
            raise ValueError(f"cost: expected shape {(self.rows, self.cols, self.max_disp)}, got {c.shape}")
        check(self._lib.sgm_stage_filter_volume(self._h, _ptr(c), self._filter_bits(horizontal, vertical)), self._h)
        return c

    def set_window(self, win_h: int, win_w: int) -> None:
        """sgm_set_window: the matching window of the census and of the SAD /
        SSD costs, the reference's WIN_H, WIN_W (7, 9) before the division by
        the scale.  Frames, stage_census() and window_cost() of this handle use
        it from the next call on.  Accepted: 1 <= win_h // s, win_w // s <= 9, not
        1 x 1 taps and not 9 x 9 (80 census bits); anything else raises SGMError and
        changes nothing.  Waits for the handle's work; re-capture graphs afterwards."""
        check(self._lib.sgm_set_window(self._h, int(win_h), int(win_w)), self._h)

    @property
    def window(self):
        """sgm_get_window: (win_h, win_w) as set."""
        wh, ww = ctypes.c_int(), ctypes.c_int()
        check(self._lib.sgm_get_window(self._h, ctypes.byref(wh), ctypes.byref(ww)), self._h)
        return wh.value, ww.value

    def set_weighted(self, enable: bool = True) -> None:
        """sgm_set_weighted: the reference's WEIGHTED_COST (inc/Solver.h:15) on
        the handle's window.  SAD and SSD multiply every tap by the Gaussian
        weight exp(-(da^2 + db^2) / 25) of its offset from the centre (fp32
        multiply, then add, in the reference's tap order); the census skips the
        taps whose weight is below 0.5, a disc of da^2 + db^2 <= 17 (7 x 9 keeps
        50 of 62 bits).  Frames, stage_census() and window_cost() follow it from
        the next call on.  Only with win_h // s and win_w // s odd: otherwise,
        and for a later set_window() to such a window, SGMError and nothing
        changes.  Waits for the handle's work; re-capture graphs afterwards."""
        check(self._lib.sgm_set_weighted(self._h, 1 if enable else 0), self._h)

    @property
    def weighted(self) -> bool:
        """sgm_get_weighted."""
        on = ctypes.c_int()
        check(self._lib.sgm_get_weighted(self._h, ctypes.byref(on)), self._h)
        return bool(on.value)

    def window_weights(self):
        """sgm_get_window_weights: the (win_h // s, win_w // s) float32 weight
        table of a weighted handle (Solver.cpp:29-45)."""
        n = ctypes.c_int()
        check(self._lib.sgm_get_window_weights(self._h, None, 0, ctypes.byref(n)), self._h)
        w = np.empty(n.value, np.float32)
        check(self._lib.sgm_get_window_weights(self._h, _ptr(w), n.value, ctypes.byref(n)), self._h)
        wh, ww = self.window
        return w.reshape(wh // self.scale, ww // self.scale)

    def window_cost(self, left, right, kind: str = "sad", out=None, stream=None):
        """sgm_window_cost_device: the float32 (rows, cols, D) SAD, SSD or CT cost
        volume of two torch uint8 device images of shape (h, w) (unit column
        stride; read decimated by the scale, not blurred), as a torch tensor on
        the same device (`out`, allocated when None).  One launch on `stream`
        (default: the device's current torch stream; the tensors' lifetime on
        another stream is the caller's, as for aggregate).  The result goes
        straight into aggregate()."""
        if kind not in ("sad", "ssd", "ct"):
            raise ValueError(f"kind must be 'sad', 'ssd' or 'ct', got {kind!r}")
        import torch
        for name, img in (("left", left), ("right", right)):
            if isinstance(img, np.ndarray) or not hasattr(img, "data_ptr"):
                raise TypeError(f"{name} must be a torch device tensor; for host numpy images use "
                                "stage_window_cost()")
            if not img.is_cuda or img.device.index != self.device:
                raise ValueError(f"{name} must live on the handle's device cuda:{self.device}, got {img.device}")
            if img.dtype != torch.uint8 or tuple(img.shape) != (self.h, self.w) or img.stride(1) != 1:
                raise ValueError(f"{name} must be a uint8 {(self.h, self.w)} tensor with unit column stride")
        if left.stride(0) != right.stride(0):
            raise ValueError("left and right must have the same row stride")
        shape = (self.rows, self.cols, self.max_disp)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=left.device)
        if (out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != left.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 {shape} tensor on {left.device}")
        self._on_torch_stream(torch, left, stream, lambda st: check(self._lib.sgm_window_cost_device(
            self._h, _capi.COST_KINDS[kind], ctypes.c_void_p(left.data_ptr()), ctypes.c_void_p(right.data_ptr()),
            left.stride(0), ctypes.c_void_p(out.data_ptr()), st), self._h))
        return out

    def stage_window_cost(self, left, right, kind: str = "sad") -> np.ndarray:
        """sgm_stage_window_cost: the same volume from host numpy (h, w) uint8
        images, as a numpy (rows, cols, D) float32 array (tests)."""
        if kind not in ("sad", "ssd", "ct"):
            raise ValueError(f"kind must be 'sad', 'ssd' or 'ct', got {kind!r}")
        l, r = _u8(left, (self.h, self.w), "left"), _u8(right, (self.h, self.w), "right")
        cost = np.empty((self.rows, self.cols, self.max_disp), np.float32)
        check(self._lib.sgm_stage_window_cost(self._h, _capi.COST_KINDS[kind], _ptr(l), _ptr(r), self.w,
                                              _ptr(cost)), self._h)
        return cost

    def check(self) -> None:
        """sgm_check: wait for the frames enqueued so far and raise SGMError
        (SGM_ERR_HIP) if a slanted-pass hand-off gave up, or a fixed-budget
        median fill ended unproven, in any of them since the last report
        (their maps are invalid).  Call it after synchronising and before
        gathering or timing device maps."""
        check(self._lib.sgm_check(self._h), self._h)

    def set_post_filter_launches(self, n: int) -> None:
        """sgm_set_post_filter_launches: n = 0, the adaptive median fill (the
        host reads its convergence counter: post-filtered frames block the
        calling thread and cannot be captured into a HIP graph); 1..4096,
        every post filter enqueues exactly n fill launches and returns, and
        check() reports a fill that launch n did not prove
        (ceil(cols / 64) * rows + 1 launches always prove it)."""
        check(self._lib.sgm_set_post_filter_launches(self._h, int(n)), self._h)

    def post_filter_proved_at(self) -> int:
        """sgm_post_filter_proved_at: waits for the last call's work, then the
        1-based index of the first fill launch of the last post filter that
        changed nothing (0: none did)."""
        k = ctypes.c_int()
        check(self._lib.sgm_post_filter_proved_at(self._h, ctypes.byref(k)), self._h)
        return k.value

    # --------------------------------------------------------- confidence
    def set_confidence(self, enable: bool) -> None:
        """sgm_set_confidence: keep (or stop keeping) the per-pixel match
        confidence of every later frame: min_cost / sec_min_cost of the
        aggregated WTA (SGM.cpp:392-409), in [0, 1), lower = more distinctive.
        Not inside stream capture; BM and aux_only handles raise."""
        check(self._lib.sgm_set_confidence(self._h, int(bool(enable))), self._h)

    def get_confidence(self, view: int = 0) -> np.ndarray:
        """The last frame's ratio map of `view` (0 = left, 1 = right; a
        one-view handle serves its own view only): rows x cols float32
        (sgm_stage_confidence; synchronous)."""
        out = np.empty((self.rows, self.cols), np.float32)
        check(self._lib.sgm_stage_confidence(self._h, int(view), _ptr(out)), self._h)
        return out

    def confidence_device(self, d_ratio: int, *, view: int = 0, pitch: int | None = None,
                          stream: int | None = None) -> None:
        """The same map into a row-major device buffer (sgm_confidence_device:
        enqueue only, capturable with the frame)."""
        check(self._lib.sgm_confidence_device(self._h, int(view), ctypes.c_void_p(d_ratio),
                                              pitch or self.cols, _stream(stream)), self._h)

    def confidence_filter_device(self, d_disp: int, d_ratio: int, max_ratio: float, *,
                                 pitch: int | None = None, ratio_pitch: int | None = None,
                                 stream: int | None = None) -> None:
        """In place on a device map: disp = D+1 where ratio > max_ratio
        (sgm_confidence_filter_device)."""
        check(self._lib.sgm_confidence_filter_device(
            self._h, ctypes.c_void_p(d_disp), pitch or self.cols, ctypes.c_void_p(d_ratio),
            ratio_pitch or self.cols, ctypes.c_float(max_ratio), _stream(stream)), self._h)

    def confidence_filter(self, disp, ratio, max_ratio: float) -> np.ndarray:
        """A stricter uniqueness without re-running the frame: a copy of
        `disp` with D+1 where ratio > max_ratio, computed on the GPU.  (The
        WTA's |min_d - sec_d| > 1 clause is not reproduced.)"""
        f = np.array(disp, dtype=np.float32, copy=True, order="C")
        r = np.ascontiguousarray(ratio, dtype=np.float32)
        if f.shape != (self.rows, self.cols) or r.shape != f.shape:
            raise ValueError(f"disp and ratio: expected shape {(self.rows, self.cols)}")
        check(self._lib.sgm_stage_confidence_filter(self._h, _ptr(f), _ptr(r),
                                                    ctypes.c_float(max_ratio)), self._h)
        return f

    def get_disp(self) -> np.ndarray:
        """Post-filtered disparity (inc/Solver.h:36: filtered_disp after
        post_filter, Solver.cpp:600-649), computed on the GPU; invalid = D+1.
        On a handle with fill set: fill(post_filter(lr)), against the last
        frame's right view (right=None)."""
        if self._final is None:
            f = self.post_filter(self._lr)
            self._final = f if self.fill == "off" else self.fill_disp(f)[0]
        return self._final

    # ------------------------------------------------------- hole filling
    @staticmethod
    def _fill_code(mode) -> int:
        if isinstance(mode, str):
            if mode not in _capi.FILL_MODES:
                raise ValueError(f"fill must be one of {sorted(_capi.FILL_MODES)}, got {mode!r}")
            return _capi.FILL_MODES[mode]
        return int(mode)

    def set_fill(self, mode: str) -> None:
        """sgm_set_fill: "off" (the default), "background" or "interpolate":
        every later frame -- process(), process_device(), aggregate(), of any
        cost and schedule -- fills the invalid pixels of its final map as its
        last map stage, after post_filter and LKRefine and before the
        reprojection (Hirschmueller 2008, 2.6).  Each invalid
        pixel takes one of the first valid values of the unfilled map along its
        8 rays: "background" the second lowest; "interpolate" classifies it
        against the frame's right view first, occlusions take the second
        lowest and mismatches the upper median.  get_fill_mask() tells which
        pixels are inferred.  "interpolate" needs a two-view SGM handle; BM
        and one-view handles serve "background"; view="right" handles raise
        SGMError.  Allocates 25 bytes per pixel ("off" frees them); waits for
        the handle's work; not inside stream capture; re-capture graphs."""
        check(self._lib.sgm_set_fill(self._h, self._fill_code(mode)), self._h)
        self._filled = self._fill_code(mode) != 0

    @property
    def fill(self) -> str:
        """sgm_get_fill, by name."""
        m = ctypes.c_int()
        check(self._lib.sgm_get_fill(self._h, ctypes.byref(m)), self._h)
        return {v: n for n, v in _capi.FILL_MODES.items()}[m.value]

    def fill_disp(self, disp, right=None, mode=None):
        """sgm_stage_fill: (filled copy, uint8 fill mask) of a rows x cols
        true-disparity map, on a handle whose fill is set (an aux_only handle
        with the same min_disp included).  mode: "background" or
        "interpolate" (None: the handle's own); right: the right view's rows x
        cols map for "interpolate" (None: this handle's last frame's right
        view, two-view handles only).  Mask: 0 measured, 1 filled as
        occlusion, 2 filled as mismatch, 3 still invalid.  Synchronous."""
        f = np.array(disp, dtype=np.float32, copy=True, order="C")
        if f.shape != (self.rows, self.cols):
            raise ValueError(f"disp: expected shape {(self.rows, self.cols)}, got {f.shape}")
        r = None
        if right is not None:
            r = np.ascontiguousarray(right, dtype=np.float32)
            if r.shape != f.shape:
                raise ValueError(f"right: expected shape {(self.rows, self.cols)}, got {r.shape}")
        mask = np.empty((self.rows, self.cols), np.uint8)
        code = self._fill_code(self.fill if mode is None else mode)
        check(self._lib.sgm_stage_fill(self._h, _ptr(f), _ptr(r), code, _ptr(mask)), self._h)
        return f, mask

    def fill_device(self, d_disp: int, *, d_right: int = 0, mode=None, d_mask: int = 0,
                    pitch: int | None = None, right_pitch: int | None = None,
                    mask_pitch: int | None = None, stream: int | None = None) -> None:
        """In place on a device map (sgm_fill_device: two launches, enqueue
        only, capturable); d_right = 0: this handle's last frame's right view;
        d_mask = 0: the handle's own mask (get_fill_mask()); pitches in
        elements.  hipStreamLegacy (stream=0) is refused."""
        code = self._fill_code(self.fill if mode is None else mode)
        check(self._lib.sgm_fill_device(
            self._h, ctypes.c_void_p(d_disp or None), self.cols if pitch is None else pitch,
            ctypes.c_void_p(d_right or None), self.cols if right_pitch is None else right_pitch, code,
            ctypes.c_void_p(d_mask or None), self.cols if mask_pitch is None else mask_pitch,
            _stream(stream)), self._h)

    def get_fill_mask(self) -> np.ndarray:
        """The fill mask of the last filled frame: rows x cols uint8, a host
        copy (sgm_stage_fill_mask)."""
        out = np.empty((self.rows, self.cols), np.uint8)
        check(self._lib.sgm_stage_fill_mask(self._h, _ptr(out)), self._h)
        return out

    def get_lr_disp(self) -> np.ndarray:
        """Sub-pixel disparity after the LR check (SGM.cpp:803-818)."""
        if self._lr is None:
            raise RuntimeError("constructed with post_filter=True: only get_disp() is kept")
        return self._lr

    def lr_check_device(self, d_fl: int, d_fr: int, d_out: int, *, fl_pitch: int | None = None,
                        fr_pitch: int | None = None, out_pitch: int | None = None,
                        stream: int | None = None) -> None:
        """The LR check (SGM.cpp:803-818) of two device sub-pixel maps, e.g.
        the left and right views computed on two GPUs (sgm_lr_check_device);
        d_out may be d_fl."""
        check(self._lib.sgm_lr_check_device(
            self._h, ctypes.c_void_p(d_fl), fl_pitch or self.cols, ctypes.c_void_p(d_fr),
            fr_pitch or self.cols, ctypes.c_void_p(d_out), out_pitch or self.cols,
            _stream(stream)), self._h)

    def post_filter(self, disp) -> np.ndarray:
        """post_filter() (Solver.cpp:600-649) of a rows x cols map on the GPU
        (sgm_stage_post_filter); returns a filtered copy.  Synchronous: with a
        launch budget, a fill the budget did not prove raises here."""
        f = np.array(disp, dtype=np.float32, copy=True, order="C")
        if f.shape != (self.rows, self.cols):
            raise ValueError(f"disp: expected shape {(self.rows, self.cols)}, got {f.shape}")
        check(self._lib.sgm_stage_post_filter(self._h, _ptr(f)), self._h)
        return f

    def post_filter_device(self, d_disp: int, *, pitch: int | None = None, stream: int | None = None) -> None:
        """In place on a device map (sgm_post_filter_device)."""
        check(self._lib.sgm_post_filter_device(self._h, ctypes.c_void_p(d_disp),
                                               pitch or self.cols,
                                               _stream(stream)), self._h)

    def lk_refine(self, img_l, img_r, disp) -> np.ndarray:
        """LKSubPixel::LKRefine(img_l, img_r, disp_float) (LKSubPixelImpl.cpp:
        13-235) on the GPU: full-size images, working-grid map; returns a
        refined copy (sgm_stage_lk_refine)."""
        l = _u8(img_l, (self.h, self.w), "img_l")
        r = _u8(img_r, (self.h, self.w), "img_r")
        f = np.array(disp, dtype=np.float32, copy=True, order="C")
        if f.shape != (self.rows, self.cols):
            raise ValueError(f"disp: expected shape {(self.rows, self.cols)}, got {f.shape}")
        check(self._lib.sgm_stage_lk_refine(self._h, _ptr(l), _ptr(r), self.w, _ptr(f)), self._h)
        return f

    def lk_refine_device(self, d_left: int, d_right: int, d_disp: int, *, pitch: int | None = None,
                         disp_pitch: int | None = None, stream: int | None = None) -> None:
        """In place on a device map (sgm_lk_refine_device)."""
        check(self._lib.sgm_lk_refine_device(
            self._h, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), pitch or self.w,
            ctypes.c_void_p(d_disp), disp_pitch or self.cols, _stream(stream)),
            self._h)

    def sky_detect(self, img) -> np.ndarray:
        """SkyAreaDetector::detect(img, ..., scale) (imageSkyDetector.cpp:166-208)
        on the GPU: u8 mask on the working grid, 255 = sky."""
        img = _u8(img, (self.h, self.w), "img")
        mask = np.empty((self.rows, self.cols), np.uint8)
        check(self._lib.sgm_stage_sky_detect(self._h, _ptr(img), self.w, _ptr(mask)), self._h)
        return mask

    def sky_detect_device(self, d_img: int, d_mask: int, *, pitch: int | None = None,
                          mask_pitch: int | None = None, stream: int | None = None) -> None:
        check(self._lib.sgm_sky_detect_device(self._h, ctypes.c_void_p(d_img), pitch or self.w,
                                              ctypes.c_void_p(d_mask), mask_pitch or self.cols,
                                              _stream(stream)), self._h)

    def colormap(self, disp) -> np.ndarray:
        """Solver::colormap (Solver.cpp:652-707) on the GPU: rows x cols x 3 BGR."""
        f = np.ascontiguousarray(disp, dtype=np.float32)
        if f.shape != (self.rows, self.cols):
            raise ValueError(f"disp: expected shape {(self.rows, self.cols)}, got {f.shape}")
        out = np.empty((self.rows, self.cols, 3), np.uint8)
        check(self._lib.sgm_stage_colormap(self._h, _ptr(f), _ptr(out)), self._h)
        return out

    def point_cloud(self, disp, img, fx, fy, cx, cy, baseline=0.5, max_range=100.0):
        """node.cpp:119-143 on the GPU: (N x 3 float64 points, N u8 gray values)
        in row-major order; img is the node's full-size image."""
        f = np.ascontiguousarray(disp, dtype=np.float32)
        im = np.ascontiguousarray(img, dtype=np.uint8)
        if f.shape != (self.rows, self.cols) or im.shape[0] < self.rows or im.shape[1] < self.cols:
            raise ValueError("disp must be rows x cols and img at least that large")
        cam = _capi.Camera(fx, fy, cx, cy, baseline, max_range)
        xyz = np.empty((self.rows * self.cols, 3), np.float64)
        pix = np.empty(self.rows * self.cols, np.uint8)
        n = ctypes.c_int()
        check(self._lib.sgm_stage_point_cloud(self._h, _ptr(f), _ptr(im), im.shape[1],
                                              ctypes.byref(cam), _ptr(xyz), _ptr(pix),
                                              ctypes.byref(n)), self._h)
        return xyz[:n.value].copy(), pix[:n.value].copy()

    def get_raw_disp(self) -> np.ndarray:
        """Left WTA disparity (SGM.cpp:411-415; disp_beta, :755-795, for a
        right-view handle), uint16, invalid = D+1."""
        return self._raw

    # ---------------------------------------------------------- profiling
    def set_profiling(self, enable: bool) -> None:
        check(self._lib.sgm_set_profiling(self._h, int(bool(enable))), self._h)

    def get_profile(self) -> dict:
        """{kernel class: (launches, total_ms, elements per launch)}; resets."""
        buf = (_capi.KernelStat * 64)()
        n = ctypes.c_int()
        check(self._lib.sgm_get_profile(self._h, buf, 64, ctypes.byref(n)), self._h)
        return {buf[k].name.decode(): (buf[k].launches, buf[k].total_ms, buf[k].elems)
                for k in range(n.value)}

    # ------------------------------------------------------------- stages
    def stage_census(self, img) -> np.ndarray:
        img = _u8(img, (self.h, self.w), "img")
        out = np.empty((self.rows, self.cols), np.uint64)
        check(self._lib.sgm_stage_census(self._h, _ptr(img), self.w, _ptr(out)), self._h)
        return out

    def stage_cost(self, ctl, ctr, view=0, sky=None, filters=3) -> np.ndarray:
        ctl = np.ascontiguousarray(ctl, np.uint64)
        ctr = np.ascontiguousarray(ctr, np.uint64)
        sky = None if sky is None else _u8(sky, (self.rows, self.cols), "sky")
        out = np.empty((self.rows, self.cols, self.max_disp), np.float32)
        check(self._lib.sgm_stage_cost(self._h, _ptr(ctl), _ptr(ctr), _ptr(sky), view, filters,
                                       _ptr(out)), self._h)
        return out

    def stage_path(self, direction: int, cost):
        cost = np.ascontiguousarray(cost, np.float32)
        L = np.empty_like(cost)
        m = np.empty((self.rows, self.cols), np.float32)
        check(self._lib.sgm_stage_path(self._h, direction, _ptr(cost), _ptr(L), _ptr(m)),
              self._h)
        return L, m

    def stage_aggregate(self, cost):
        cost = np.ascontiguousarray(cost, np.float32)
        d = np.empty((self.rows, self.cols), np.uint16)
        f = np.empty((self.rows, self.cols), np.float32)
        check(self._lib.sgm_stage_aggregate(self._h, _ptr(cost), _ptr(d), _ptr(f)), self._h)
        return d, f

    def stage_lr(self, fl, fr) -> np.ndarray:
        fl = np.ascontiguousarray(fl, np.float32)
        fr = np.ascontiguousarray(fr, np.float32)
        out = np.empty_like(fl)
        check(self._lib.sgm_stage_lr(self._h, _ptr(fl), _ptr(fr), _ptr(out)), self._h)
        return out


class BM(SGM):
    """Block matcher on one MI355X: mirrors ``BM(int h, int w, int s, int d)``
    (inc/BM.h:6-19, src/BM.cpp:4-97): census cost + the two cost filters and a
    winner-take-all on the filtered cost (uniqueness |d1 - d2| > 2), then
    post_filter().  get_disp() is the post-filtered integer disparity (the
    reference's BM never writes filtered_disp); get_raw_disp() the
    WTA result."""

    def __init__(self, h: int, w: int, s: int = 1, d: int = 128, *, device: int = 0,
                 blur: bool = True, uniqueness: float = 0.7, sky_detect: bool = False,
                 post_filter_launches: int = 0, input_size=None, rectify=None,
                 input_format: str = "gray8", reproject=None, window=None, weighted: bool = False,
                 fill: str = "off"):
        super().__init__(h, w, s, d, device=device, blur=blur, views=1, uniqueness=uniqueness,
                         post_filter=True, sky_detect=sky_detect,
                         post_filter_launches=post_filter_launches, input_size=input_size,
                         rectify=rectify, input_format=input_format, reproject=reproject,
                         window=window, weighted=weighted, fill=fill, _solver=_capi.SGM_SOLVER_BM)


class GPU_SGM(SGM):
    """Mirrors the reference's CUDA backend class ``GPU_SGM(int h, int w, int s,
    int d)`` (gpu_sgm/inc/SGM.cuh:23-62; node.cpp:50 holds its commented-out
    call site): process(l, r) runs the LEFT view only -- SGM, WTA, sub-pixel,
    then post_filter (gpu_sgm/src/SGM.cu:105-232) -- and get_disp() returns
    that post-filtered map.  Results follow the reference's CPU path bit for bit
    (src/SGM.cpp:32-443, Solver.cpp:569-649), not the CUDA tree's
    approximations."""

    def __init__(self, h: int, w: int, s: int = 1, d: int = 128, *, device: int = 0,
                 post_filter_launches: int = 0, min_disp: int = 0, input_size=None, rectify=None,
                 input_format: str = "gray8", reproject=None, window=None, weighted: bool = False,
                 fill: str = "off"):
        super().__init__(h, w, s, d, device=device, views=1, post_filter=True,
                         post_filter_launches=post_filter_launches, min_disp=min_disp,
                         input_size=input_size, rectify=rectify, input_format=input_format,
                         reproject=reproject, window=window, weighted=weighted, fill=fill)


# sgm_camera_q without a handle: the pinhole Q of a camera, 4 x 4 float64
camera_q = SGM.camera_q
