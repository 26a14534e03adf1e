"""ctypes front end of the CPU oracle (oracle/sgm_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() (as the
checker) and bench.py's cpu_baseline leg.  The product package
``stereo_matching_amd`` never imports this module.

Parity status (see sgm_oracle.h and DESIGN.md "Oracle and its pinning"):
pinned to the reference's own binaries from the census on.  build_ref()
compiles the reference's src/{Solver,SGM,cost,BM}.cpp unmodified against
stand-in headers (oracle/ref/) into oracle/_ref/; run_ref() runs them; the
recorded outputs are tests/golden/ref_*.npz, and tests/test_reference_parity.py
compares this oracle with them bit for bit.  Not pinned: cv::GaussianBlur's own
arithmetic, LKRefine, and everything the reference does not have.
"""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "liboracle_sgm.so")
_lib = None

L1, L2, L3, L4, L5, L6, L7, L8 = range(8)


def build(force: bool = False) -> str:
    """Compile liboracle_sgm.so with the Makefile next to this file."""
    if force or not os.path.exists(_LIB_PATH) or (
        os.path.getmtime(_LIB_PATH) < max(os.path.getmtime(os.path.join(_HERE, f))
                                          for f in ("sgm_oracle.c", "sgm_oracle.h", "Makefile"))):
        subprocess.run(["make", "-s", "-C", _HERE, "liboracle_sgm.so"], check=True)
    return _LIB_PATH


# ------------------------------------------------------------------ reference
_REF_OUT = os.path.join(_HERE, "_ref")
_REF_DRIVER = os.path.join(_REF_OUT, "ref_driver")
REF_MODES = {"stages": 0, "process": 1, "bm": 2, "post_filter": 3, "subpixel": 4, "colormap": 5}


def reference_dir():
    """The reference checkout (SGM_REFERENCE_DIR, default: `reference` next to
    the repository), or None when it does not hold the four source files."""
    d = os.environ.get("SGM_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(_HERE)),
                                                            "reference")
    ok = all(os.path.isfile(os.path.join(d, "src", f))
             for f in ("Solver.cpp", "SGM.cpp", "cost.cpp", "BM.cpp"))
    return os.path.abspath(d) if ok else None


def build_ref():
    """Compile the reference's own sources and oracle/ref/ref_driver.cpp into
    oracle/_ref/ (Makefile target `ref`).  Returns the driver's path, or None
    when there is no reference to compile."""
    d = reference_dir()
    if d is None:
        return None
    subprocess.run(["make", "-s", "-C", _HERE, "ref", "SGM_REFERENCE_DIR=" + d], check=True,
                   stdout=subprocess.DEVNULL)
    return _REF_DRIVER


def ref_driver():
    """Path of a built driver whose reference is still there, else None."""
    return _REF_DRIVER if reference_dir() and os.access(_REF_DRIVER, os.X_OK) else None


def run_ref(mode, left, right, D, scale=1, sky_l=None, sky_r=None, fmap=None, blur=True,
            threads=1, driver=None):
    """Run the reference through the driver; returns {name: array} in the
    order the driver wrote them (request and record layout: ref_driver.cpp)."""
    driver = driver or ref_driver()
    if driver is None:
        raise RuntimeError("no reference driver: oracle.build_ref() found no reference")
    left = _c(left, np.uint8)
    right = _c(right, np.uint8)
    h, w = left.shape
    H, W = h // scale, w // scale
    has_sky = sky_l is not None
    head = struct.pack("<10i", 0x51524753, REF_MODES[mode], h, w, scale, D, int(bool(blur)),
                       int(has_sky), int(fmap is not None), 0)
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_DYNAMIC="false")
    with tempfile.TemporaryDirectory() as tmp:
        req, res = os.path.join(tmp, "req.bin"), os.path.join(tmp, "out.bin")
        with open(req, "wb") as fh:
            fh.write(head)
            fh.write(left.tobytes())
            fh.write(right.tobytes())
            if has_sky:
                for m in (sky_l, sky_r):
                    m = _c(m, np.uint8)
                    assert m.shape == (H, W)
                    fh.write(m.tobytes())
            if fmap is not None:
                fmap = _c(fmap, np.float32)
                assert fmap.shape == (H, W)
                fh.write(fmap.tobytes())
        subprocess.run([driver, req, res], check=True, env=env, stdout=subprocess.DEVNULL, timeout=300)
        out = {}
        dtypes = (np.uint8, np.float32, np.uint64)
        with open(res, "rb") as fh:
            while True:
                rec = fh.read(32)
                if not rec:
                    break
                name = rec[:16].rstrip(b"\0").decode()
                kind, d0, d1, d2 = struct.unpack("<4i", rec[16:])
                shape = (d0, d1, d2) if d2 else (d0, d1)
                out[name] = np.fromfile(fh, dtypes[kind], int(np.prod(shape))).reshape(shape)
    return out


class _Result(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("disp", "disp_beta", "sub", "sub_beta", "lr", "final_disp")]


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB_PATH)
        P = ctypes.c_void_p
        I = ctypes.c_int
        F = ctypes.c_float
        L.orc_blur.argtypes = [P, P, I, I]
        L.orc_census.argtypes = [P, P, I, I, I]
        L.orc_dsi.argtypes = [P, P, P, P, I, I, I, I, I]
        L.orc_hfilter.argtypes = [P, I, I, I, I]
        L.orc_vfilter.argtypes = [P, I, I, I, I]
        L.orc_path.argtypes = [P, P, P, I, I, I, I, I, I]
        L.orc_aggregate.argtypes = [P, P, I, I, I]
        L.orc_wta.argtypes = [P, P, I, I, I, F]
        L.orc_subpixel.argtypes = [P, P, P, I, I, I]
        L.orc_lr_check.argtypes = [P, P, I, I, I, I, F]
        L.orc_post_filter.argtypes = [P, I, I, I, I]
        L.orc_lk_refine.argtypes = [P, P, P, I, I, I]
        L.orc_sky_detect.argtypes = [P, I, I, I, I, P]
        L.orc_bm_process.argtypes = [P, P, P, I, I, I, I, F, I, P]
        L.orc_bm_process.restype = I
        L.orc_process.argtypes = [P, P, P, P, I, I, I, I, I, I, F, F, I, I, ctypes.POINTER(_Result)]
        L.orc_process.restype = I
        for fn in (L.orc_process_lean, L.orc_process_refplace):
            fn.argtypes = L.orc_process.argtypes
            fn.restype = I
        L.orc_max_threads.restype = I
        L.orc_set_threads.argtypes = [I]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def blur(img):
    img = _c(img, np.uint8)
    out = np.empty_like(img)
    lib().orc_blur(_p(img), _p(out), img.shape[0], img.shape[1])
    return out


def census(img, scale=1):
    img = _c(img, np.uint8)
    out = np.empty(img.shape, np.uint64)
    lib().orc_census(_p(img), _p(out), img.shape[0], img.shape[1], scale)
    return out


def dsi(ctl, ctr, D, scale=1, view=0, sky=None):
    ctl = _c(ctl, np.uint64)
    ctr = _c(ctr, np.uint64)
    H, W = ctl.shape
    sky = None if sky is None else _c(sky, np.uint8)
    out = np.empty((H, W, D), np.float32)
    lib().orc_dsi(_p(ctl), _p(ctr), _p(sky), _p(out), H, W, D, scale, view)
    return out


def hfilter(cost, win):
    c = np.array(cost, dtype=np.float32, copy=True, order="C")
    H, W, D = c.shape
    lib().orc_hfilter(_p(c), H, W, D, win)
    return c


def vfilter(cost, win):
    c = np.array(cost, dtype=np.float32, copy=True, order="C")
    H, W, D = c.shape
    lib().orc_vfilter(_p(c), H, W, D, win)
    return c


def path(cost, direction, P1=10, P2=100):
    cost = _c(cost, np.float32)
    H, W, D = cost.shape
    L = np.empty_like(cost)
    m = np.empty((H, W), np.float32)
    lib().orc_path(_p(cost), _p(L), _p(m), H, W, D, direction, P1, P2)
    return L, m


def aggregate(Ls):
    Ls = [_c(x, np.float32) for x in Ls]
    H, W, D = Ls[0].shape
    arr = (ctypes.c_void_p * 8)(*[x.ctypes.data for x in Ls])
    S = np.empty_like(Ls[0])
    lib().orc_aggregate(ctypes.cast(arr, ctypes.c_void_p), _p(S), H, W, D)
    return S


def wta(S, uniq=0.7):
    S = _c(S, np.float32)
    H, W, D = S.shape
    d = np.empty((H, W), np.int32)
    lib().orc_wta(_p(S), _p(d), H, W, D, uniq)
    return d


def subpixel(disp, S):
    S = _c(S, np.float32)
    disp = _c(disp, np.int32)
    H, W, D = S.shape
    out = np.empty((H, W), np.float32)
    lib().orc_subpixel(_p(disp), _p(S), _p(out), H, W, D)
    return out


def lr_check(FL, FR, D, scale=1, lr_dis=1.0):
    FL = np.array(FL, dtype=np.float32, copy=True, order="C")
    FR = _c(FR, np.float32)
    H, W = FL.shape
    lib().orc_lr_check(_p(FL), _p(FR), H, W, D, scale, lr_dis)
    return FL


def post_filter(F, D, scale=1):
    F = np.array(F, dtype=np.float32, copy=True, order="C")
    H, W = F.shape
    lib().orc_post_filter(_p(F), H, W, D, scale)
    return F


def lk_refine(left, right, disp, D):
    """LKRefine (LKSubPixelImpl.cpp:13-235) on working-grid images; returns a
    refined copy of disp."""
    L = _c(left, np.uint8)
    R = _c(right, np.uint8)
    F = np.array(disp, np.float32, copy=True, order="C")
    H, W = F.shape
    assert L.shape == R.shape == (H, W)
    lib().orc_lk_refine(_p(L), _p(R), _p(F), H, W, D)
    return F


def sky_detect(img, scale=1):
    """SkyAreaDetector::detect (imageSkyDetector.cpp:166-208): u8 mask on the
    working grid, 255 = sky."""
    img = _c(img, np.uint8)
    h, w = img.shape
    mask = np.empty((h // scale, w // scale), np.uint8)
    lib().orc_sky_detect(_p(img), h, w, w, scale, _p(mask))
    return mask


def bm_process(left, right, D, scale=1, sky=None, uniq=0.7, blur=True):
    """BM::process (src/BM.cpp:9-97): raw WTA disparity (int32, invalid D+1)."""
    left = _c(left, np.uint8)
    right = _c(right, np.uint8)
    h, w = left.shape
    sky = None if sky is None else _c(sky, np.uint8)
    disp = np.empty((h // scale, w // scale), np.int32)
    rc = lib().orc_bm_process(_p(left), _p(right), _p(sky), h, w, scale, D, uniq, int(bool(blur)),
                              _p(disp))
    assert rc == 0
    return disp


_SCHEDULES = {"parity": "orc_process", "lean": "orc_process_lean",
              "refplace": "orc_process_refplace"}


def process(left, right, D, scale=1, sky_l=None, sky_r=None, P1=10, P2=100,
            uniq=0.7, lr_dis=1.0, blur=True, views=2, schedule="parity", final=True):
    """Whole SGM::process (src/SGM.cpp:32-826).  Returns a dict of HW arrays.

    schedule: "parity" (10 volumes), "lean" (3 volumes, for 4K256) or
    "refplace" (the reference's OpenMP placement, the timed CPU baseline);
    all three give identical bits.  final=False skips post_filter."""
    left = _c(left, np.uint8)
    right = _c(right, np.uint8)
    h, w = left.shape
    H, W = h // scale, w // scale
    sky_l = None if sky_l is None else _c(sky_l, np.uint8)
    sky_r = None if sky_r is None else _c(sky_r, np.uint8)
    out = {"disp": np.empty((H, W), np.int32), "sub": np.empty((H, W), np.float32)}
    if views >= 2:
        out.update(disp_beta=np.empty((H, W), np.int32), sub_beta=np.empty((H, W), np.float32),
                   lr=np.empty((H, W), np.float32))
        if final:
            out["final"] = np.empty((H, W), np.float32)
    r = _Result(_p(out["disp"]), _p(out.get("disp_beta")), _p(out["sub"]),
                _p(out.get("sub_beta")), _p(out.get("lr")), _p(out.get("final")))
    rc = getattr(lib(), _SCHEDULES[schedule])(_p(left), _p(right), _p(sky_l), _p(sky_r), h, w, scale, D, P1, P2,
                           uniq, lr_dis, int(bool(blur)), views, ctypes.byref(r))
    if rc != 0:
        raise ValueError("orc_process rejected its arguments")
    return out


def max_threads() -> int:
    return lib().orc_max_threads()


def set_threads(n: int) -> None:
    lib().orc_set_threads(n)
