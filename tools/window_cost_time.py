"""Times the SAD / SSD producer launch (sgm_window_cost.hip) against a
device-to-device hipMemcpyAsync of one view's bytes and against the import
launch's left view at the same sizes, then the K128 SAD frame with one view and
with two against the census frame of the same handle parameters and against
window_cost -> aggregate as two calls.  HIP events around each call, median of
N; prints the table kept in profiles/window_cost_ab.txt.

What the figures include: every event pair brackets the Python call (argument
checks and ctypes, a few microseconds of host work that can show as an idle
gap); the copy goes through bare ctypes.  The producer's required traffic is its
store, so its TB/s counts the bytes written only; the copy's and the import's
count bytes read and written.

    python tools/window_cost_time.py [N]
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
        with SGM(h, w, 1, D, aux_only=True) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            nvol = h * w * D
            d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
            out = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
            twin = torch.rand((h, w, D), dtype=torch.float32, device=DEV)
            d2d = event_time.d2d_copy(s.stream)
            copy = timed(stream, lambda: d2d(out.data_ptr(), twin.data_ptr(), nvol * 4))
            print(f"{h}x{w}x{D} memcpy d2d {nvol * 4 / 1e6:8.1f} MB out: {fmt(copy)}  "
                  f"{2 * nvol * 4 / copy[0] / 1e9:5.2f} TB/s read + written")
            imp = timed(stream, lambda: s.import_volume(twin, 0, layout="hwd", out=out, stream=s.stream))
            print(f"{h}x{w}x{D} import hwd float32 left: {fmt(imp)}  "
                  f"{imp[0] / copy[0]:5.2f} x the copy")
            for kind in ("sad", "ssd"):
                t = timed(stream, lambda: s.window_cost(d_l, d_r, kind, out=out, stream=s.stream))
                print(f"{h}x{w}x{D} window_cost {kind}: {fmt(t)}  "
                      f"{nvol * 4 / t[0] / 1e9:5.2f} TB/s written  {t[0] / copy[0]:5.2f} x the copy  "
                      f"{t[0] / imp[0]:5.2f} x the import")
            del out, twin
    # the K128 frame: census against SAD, and the SAD frame as two calls
    h, w, D = 375, 1242, 128
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    for views in (1, 2):
        with SGM(h, w, 1, D, views=views) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            res = torch.empty((h, w), dtype=torch.float32, device=DEV)
            vol = torch.empty((h, w, D), dtype=torch.float32, device=DEV)

            def frame():
                s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream)

            def two_calls():
                s.window_cost(d_l, d_r, "sad", out=vol, stream=s.stream)
                s.aggregate(vol, layout="hwd", out=res, stream=s.stream)

            c = timed(stream, frame)
            print(f"K128 views={views} census frame:               {fmt(c)}")
            t = timed(stream, two_calls)
            print(f"K128 views={views} window_cost -> aggregate:   {fmt(t)}")
            s.set_cost("sad")
            f = timed(stream, frame)
            print(f"K128 views={views} SAD frame:                  {fmt(f)}")
            print("    per launch class (mean ms): " +
                  ", ".join(f"{k} {v:.3f}" for k, v in class_means(profile_of(s, frame, N)).items()))
            s.check()


if __name__ == "__main__":
    main()
