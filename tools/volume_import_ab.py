"""Times the cost-volume import (sgm_volume.hip) against a device-to-device
hipMemcpyAsync of the same output bytes, and the whole aggregate() call against
the same handle's process_device frame.  HIP events around each launch, median
of N; prints the table kept in profiles/volume_import_ab.txt.

What the figures include: the one-view event pairs bracket the Python call
(SGM.import_volume: argument checks and ctypes, a few microseconds of host work
that can show as an idle gap), while the copy goes through bare ctypes, so the
comparison leans against the import.  "both" (one launch writing both views,
which exists only inside sgm_aggregate_device) is the library's own event pair
(profile class vol_import), a MEAN over N launches, and is taken only below
1 GiB per volume: at 1080x1920x256 it is not measured.

    python tools/volume_import_ab.py [N]
"""
from __future__ import annotations

import functools
import sys

import numpy as np
import torch

import event_time
from event_time import DEV, fmt, profile_of
from stereo_matching_amd import SGM, _capi, synthetic

N = int(sys.argv[1]) if len(sys.argv) > 1 else 25
timed = functools.partial(event_time.timed, n=N)


def main():
    _capi.lib()
    print(f"# median of {N} (min..max), HIP events around the launch; TB/s = (bytes read + written) / time")
    for h, w, D in ((375, 1242, 128), (1080, 1920, 256)):
        with SGM(h, w, 1, D, aux_only=True) as s, SGM(h, w, 1, D, views=2) as s2:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            nvol = h * w * D
            out = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
            twin = torch.empty_like(out)
            d2d = event_time.d2d_copy(s.stream)
            med, lo, hi = timed(stream, lambda: d2d(out.data_ptr(), twin.data_ptr(), nvol * 4))
            print(f"{h}x{w}x{D} memcpy d2d {nvol * 4 / 1e6:8.1f} MB out: {med:7.3f} ms ({lo:.3f}..{hi:.3f})  "
                  f"{2 * nvol * 4 / med / 1e9:5.2f} TB/s")
            for layout in ("hwd", "dhw"):
                for dt in (torch.float32, torch.float16):
                    shape = (h, w, D) if layout == "hwd" else (D, h, w)
                    cost = (torch.rand(shape, device=DEV) * 64).to(dt)
                    eb = cost.element_size()
                    for view, what in ((0, "left"), (1, "right")):
                        med, lo, hi = timed(stream, lambda: s.import_volume(cost, view, layout=layout, out=out,
                                                                            stream=s.stream))
                        moved = nvol * (eb + 4)
                        print(f"{h}x{w}x{D} {layout} {str(dt)[6:]:8s} {what:5s}: {med:7.3f} ms ({lo:.3f}..{hi:.3f})  "
                              f"{moved / 1e6:8.1f} MB  {moved / med / 1e9:5.2f} TB/s")
                    # both views in one launch: the library's own event pair (profile class vol_import)
                    if nvol * 4 < 1 << 30:
                        res = torch.empty((h, w), dtype=torch.float32, device=DEV)
                        n, total, _ = profile_of(s2, lambda: s2.aggregate(cost, layout=layout, out=res,
                                                                          stream=s2.stream), N, warm=1)["vol_import"]
                        moved = nvol * (eb + 8)
                        print(f"{h}x{w}x{D} {layout} {str(dt)[6:]:8s} both : {total / n:7.3f} ms (mean of {n})  "
                              f"{moved / 1e6:8.1f} MB  {moved / (total / n) / 1e9:5.2f} TB/s (source counted once)")
                    del cost
    # the whole call at K128 against the same handle's frame
    h, w, D = 375, 1242, 128
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    for views in (1, 2):
        with SGM(h, w, 1, D, views=views) as s:
            stream = torch.cuda.ExternalStream(s.stream, device=DEV)
            d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
            res = torch.empty((h, w), dtype=torch.float32, device=DEV)
            f = timed(stream, lambda: s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(), stream=s.stream))
            print(f"K128 views={views} process_device frame: {fmt(f)}")
            for layout, dt in (("dhw", torch.float16), ("dhw", torch.float32), ("hwd", torch.float32)):
                shape = (h, w, D) if layout == "hwd" else (D, h, w)
                cost = (torch.rand(shape, device=DEV) * 64).to(dt)
                a = timed(stream, lambda: s.aggregate(cost, layout=layout, out=res, stream=s.stream))
                print(f"K128 views={views} aggregate({layout} {str(dt)[6:]}): {fmt(a)}")
            s.check()


if __name__ == "__main__":
    main()
