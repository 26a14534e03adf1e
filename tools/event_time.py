"""What the per-call timing tools share (window_time, window_cost_time,
weighted_time, volume_filter_time, ct_cost_time, volume_import_ab): a HIP event
pair around each call with a synchronise after each, milliseconds, median of n
after discarded warm-up runs; the handle's own profile per launch class; and a
device-to-device copy as the yardstick.  (reproject_time.py and its like follow
another protocol -- every launch's events first, one synchronise, microseconds
-- and keep their own.)"""
from __future__ import annotations

import ctypes
import statistics

import torch

from stereo_matching_amd import _capi

DEV = torch.device("cuda", 0)


def timed(stream, fn, n, warm=3):
    """(median, min, max) ms of n calls of fn on stream, after warm discarded ones."""
    ms = []
    for k in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        b.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t, digits=3):
    return f"{t[0]:7.{digits}f} ms ({t[1]:.{digits}f}..{t[2]:.{digits}f})"


def profile_of(s, frame, n, warm=0):
    """The handle's profile over n calls of frame, after warm unprofiled ones:
    {launch class: (launches, total ms, ...)}."""
    for _ in range(warm):
        frame()
    if warm:
        torch.cuda.synchronize(DEV)
    s.set_profiling(True)
    s.get_profile()
    for _ in range(n):
        frame()
    torch.cuda.synchronize(DEV)
    prof = s.get_profile()
    s.set_profiling(False)
    return prof


def class_means(prof):
    """Mean ms per launch class of a profile."""
    return {k: v[1] / v[0] for k, v in prof.items()}


def d2d_copy(hip_stream):
    """copy(dst_ptr, src_ptr, nbytes): a device-to-device hipMemcpyAsync on hip_stream through
    bare ctypes, in the HIP runtime the library shares with PyTorch."""
    _capi.lib()
    hip = ctypes.CDLL(_capi.hip_runtimes()[0])
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return lambda dst, src, nbytes: hip.hipMemcpyAsync(dst, src, nbytes, 3, ctypes.c_void_p(hip_stream))
