"""Times the CT producer launch (window_cost_ct_kernel) beside the
SAD producer, a device-to-device hipMemcpyAsync of one view's bytes and the
census frame's cost_h launch at the same sizes, then the K128 frame on CT with
one view and with two beside the census and the SAD frames.  HIP events around
each call, median of N; prints the table kept in profiles/ct_cost_ab.txt.

What the figures include: every event pair brackets the Python call (argument
checks and ctypes, a few microseconds of host work); the copy goes through bare
ctypes.  cost_h is the census frame's own launch class, as the handle's profile
reports it (mean of N frames).  The share of a CT launch's elements outside the
region where a census-table form would serve is printed from the
element count, not measured.

    python tools/ct_cost_time.py [N]
"""
from __future__ import annotations

import functools
import sys

import torch

import event_time
from event_time import DEV, class_means, fmt, profile_of
from stereo_matching_amd import SGM, _capi, synthetic

N = int(sys.argv[1]) if len(sys.argv) > 1 else 25
timed = functools.partial(event_time.timed, n=N)


def main():
    _capi.lib()
    print(f"# median of {N} (min..max), HIP events around the call")
    for h, w, D in ((375, 1242, 128), (1080, 1920, 256)):
        left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
        d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
        nvol = h * w * D
        with SGM(h, w, 1, D, aux_only=True) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            out = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
            twin = torch.rand((h, w, D), dtype=torch.float32, device=DEV)
            d2d = event_time.d2d_copy(s.stream)
            copy = timed(stream, lambda: d2d(out.data_ptr(), twin.data_ptr(), nvol * 4))
            print(f"{h}x{w}x{D} memcpy d2d {nvol * 4 / 1e6:8.1f} MB out: {fmt(copy)}")
            del twin
            for kind in ("sad", "ct"):
                t = timed(stream, lambda: s.window_cost(d_l, d_r, kind, out=out, stream=s.stream))
                print(f"{h}x{w}x{D} window_cost {kind:3s}: {fmt(t)}  "
                      f"{nvol * 4 / t[0] / 1e9:5.2f} TB/s written  {t[0] / copy[0]:5.2f} x the copy")
            s.set_weighted(True)
            t = timed(stream, lambda: s.window_cost(d_l, d_r, "ct", out=out, stream=s.stream))
            print(f"{h}x{w}x{D} window_cost ct weighted: {fmt(t)}")
            del out
        with SGM(h, w, 1, D, views=1) as s:
            res = torch.empty((h, w), dtype=torch.float32, device=DEV)
            prof = class_means(profile_of(s, n=N, frame=lambda: s.process_device(
                d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream)))
            print(f"{h}x{w}x{D} census frame, per launch class (mean ms): " +
                  ", ".join(f"{k} {v:.3f}" for k, v in prof.items()))
        # elements outside hw <= j <= W - 1 - hw and j - disp >= hw (hw = 4), of a row's W * D
        hw = 4
        outside = sum(min(D, max(0, D - (j - hw + 1))) if hw <= j <= w - 1 - hw else D for j in range(w))
        print(f"{h}x{w}x{D} elements outside the census-table region: {outside / (w * D):.3f} of the volume")
    h, w, D = 375, 1242, 128
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    for views in (1, 2):
        with SGM(h, w, 1, D, views=views) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            res = torch.empty((h, w), dtype=torch.float32, device=DEV)

            def frame():
                s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream)

            for kind in ("census", "sad", "ct"):
                s.set_cost(kind)
                f = timed(stream, frame)
                print(f"K128 views={views} {kind:6s} frame: {fmt(f)}")
                if kind == "ct":
                    print("    per launch class (mean ms): " +
                          ", ".join(f"{k} {v:.3f}" for k, v in class_means(profile_of(s, frame, N)).items()))
            s.check()


if __name__ == "__main__":
    main()
