"""Times what weighted windows (sgm_set_weighted) change: the
census launch of both images at 375x1242, masked against unmasked (the frame's
profile classes "census_masked" and "census"), and the weighted SAD / SSD
producer launch against the unweighted one at 375x1242x128 and 1080x1920x256,
beside a device-to-device copy of the volume's bytes.  HIP events, median of N
(min..max); prints the table kept in profiles/weighted_ab.txt.

    python tools/weighted_time.py [N]
"""
from __future__ import annotations

import functools
import sys

import torch

import event_time
from event_time import DEV, profile_of
from stereo_matching_amd import SGM, _capi, synthetic

N = int(sys.argv[1]) if len(sys.argv) > 1 else 25
timed = functools.partial(event_time.timed, n=N)
fmt = functools.partial(event_time.fmt, digits=4)


def main():
    _capi.lib()
    print(f"# median of {N} (min..max), HIP events around the call")
    for h, w, D, frames in ((375, 1242, 128, True), (1080, 1920, 256, False)):
        left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
        d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
        with SGM(h, w, 1, D, views=1, aux_only=not frames) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            out = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
            twin = torch.rand((h, w, D), dtype=torch.float32, device=DEV)
            nvol = h * w * D
            d2d = event_time.d2d_copy(s.stream)
            copy = timed(stream, lambda: d2d(out.data_ptr(), twin.data_ptr(), nvol * 4))
            print(f"{h}x{w}x{D} memcpy d2d {nvol * 4 / 1e6:.1f} MB out: {fmt(copy)}")
            for weighted in (False, True):
                s.set_weighted(weighted)
                tag = "weighted" if weighted else "unweighted"
                if frames:
                    res = torch.empty((h, w), dtype=torch.float32, device=DEV)

                    def frame():
                        s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream)

                    f = timed(stream, frame)
                    c = profile_of(s, frame, N)["census_masked" if weighted else "census"]
                    print(f"  {tag}: views=1 census frame {fmt(f)}; census launch (both images, {h}x{w}) "
                          f"{c[1] / c[0]:.4f} ms mean of {N}")
                for kind in ("sad", "ssd"):
                    t = timed(stream, lambda: s.window_cost(d_l, d_r, kind, out=out, stream=s.stream))
                    print(f"  {tag}: window_cost {kind} {h}x{w}x{D} 7x9: {fmt(t)}  {t[0] / copy[0]:5.2f} x the copy, "
                          f"{nvol * 63 / t[0] / 1e9:.1f} G taps/s")
            s.check()


if __name__ == "__main__":
    main()
