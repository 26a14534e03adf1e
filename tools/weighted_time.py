"""Times what weighted windows (sgm_set_weighted) change: the
census launch of both images at 375x1242, masked against unmasked (the frame's
profile classes "census_masked" and "census"), and the weighted SAD / SSD
producer launch against the unweighted one at 375x1242x128 and 1080x1920x256,
beside a device-to-device copy of the volume's bytes.  HIP events, median of N
(min..max); prints the table kept in profiles/weighted_ab.txt.

    python tools/weighted_time.py [N]
"""
from __future__ import annotations

import ctypes
import statistics
import sys

import torch

from stereo_matching_amd import SGM, _capi, synthetic

DEV = torch.device("cuda", 0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 25


def timed(stream, fn, n=N, warm=3):
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


def fmt(t):
    return f"{t[0]:7.4f} ms ({t[1]:.4f}..{t[2]:.4f})"


def census_launch(s, frame, name):
    s.set_profiling(True)
    s.get_profile()
    for _ in range(N):
        frame()
    torch.cuda.synchronize(DEV)
    prof = s.get_profile()
    s.set_profiling(False)
    return prof[name][1] / prof[name][0]


def main():
    _capi.lib()
    hip = ctypes.CDLL(_capi.hip_runtimes()[0])
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    print(f"# median of {N} (min..max), HIP events around the call")
    for h, w, D, frames in ((375, 1242, 128, True), (1080, 1920, 256, False)):
        left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
        d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
        with SGM(h, w, 1, D, views=1, aux_only=not frames) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            out = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
            twin = torch.rand((h, w, D), dtype=torch.float32, device=DEV)
            nvol = h * w * D
            copy = timed(stream, lambda: hip.hipMemcpyAsync(out.data_ptr(), twin.data_ptr(), nvol * 4, 3,
                                                             ctypes.c_void_p(s.stream)))
            print(f"{h}x{w}x{D} memcpy d2d {nvol * 4 / 1e6:.1f} MB out: {fmt(copy)}")
            for weighted in (False, True):
                s.set_weighted(weighted)
                tag = "weighted" if weighted else "unweighted"
                if frames:
                    res = torch.empty((h, w), dtype=torch.float32, device=DEV)

                    def frame():
                        s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream)

                    f = timed(stream, frame)
                    c = census_launch(s, frame, "census_masked" if weighted else "census")
                    print(f"  {tag}: views=1 census frame {fmt(f)}; census launch (both images, {h}x{w}) "
                          f"{c:.4f} ms mean of {N}")
                for kind in ("sad", "ssd"):
                    t = timed(stream, lambda: s.window_cost(d_l, d_r, kind, out=out, stream=s.stream))
                    print(f"  {tag}: window_cost {kind} {h}x{w}x{D} 7x9: {fmt(t)}  {t[0] / copy[0]:5.2f} x the copy, "
                          f"{nvol * 63 / t[0] / 1e9:.1f} G taps/s")
            s.check()


if __name__ == "__main__":
    main()
