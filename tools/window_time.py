"""Times what the matching window (sgm_set_window) changes: the
census launch of both images at 375x1242 per window (the frame's profile class
"census"), the SAD / SSD producer launch at 375x1242x128 per window against a
device-to-device copy of one view's bytes, and the K128 one-view census frame
per window.  HIP events, median of N (min..max); prints the table kept in
profiles/window_ab.txt.  A library without sgm_set_window (the parent commit's,
through SGM_HIP_LIB and its own tree) is timed at its fixed 7x9 with
`--default-only`.

    python tools/window_time.py [N] [--default-only]
"""
from __future__ import annotations

import functools
import sys

import torch

import event_time
from event_time import DEV
from stereo_matching_amd import SGM, _capi, synthetic

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(ARGS[0]) if ARGS else 25
DEFAULT_ONLY = "--default-only" in sys.argv
WINDOWS = [(7, 9)] if DEFAULT_ONLY else [(7, 9), (3, 3), (5, 5), (9, 7)]
timed = functools.partial(event_time.timed, n=N)
fmt = functools.partial(event_time.fmt, digits=4)


def main():
    _capi.lib()
    print(f"# median of {N} (min..max), HIP events around the call")
    h, w, D = 375, 1242, 128
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    with SGM(h, w, 1, D, views=1) as s:
        stream = torch.cuda.ExternalStream(s.stream, device=DEV)
        res = torch.empty((h, w), dtype=torch.float32, device=DEV)
        out = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
        twin = torch.rand((h, w, D), dtype=torch.float32, device=DEV)
        nvol = h * w * D
        d2d = event_time.d2d_copy(s.stream)
        copy = timed(stream, lambda: d2d(out.data_ptr(), twin.data_ptr(), nvol * 4))
        print(f"{h}x{w}x{D} memcpy d2d {nvol * 4 / 1e6:.1f} MB out: {fmt(copy)}")

        def frame():
            s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream)

        for win in WINDOWS:
            if not DEFAULT_ONLY:
                s.set_window(*win)
            name = f"{win[0]}x{win[1]}"
            f = timed(stream, frame)
            print(f"K128 views=1 census frame, window {name}: {fmt(f)}")
            c = event_time.profile_of(s, frame, N)["census"]
            print(f"    census launch (both images, {h}x{w}), window {name}: {c[1] / c[0]:.4f} ms mean of {c[0]}")
            for kind in ("sad", "ssd"):
                t = timed(stream, lambda: s.window_cost(d_l, d_r, kind, out=out, stream=s.stream))
                print(f"    window_cost {kind} {h}x{w}x{D}, window {name}: {fmt(t)}  {t[0] / copy[0]:5.2f} x the copy")
        s.check()


if __name__ == "__main__":
    main()
