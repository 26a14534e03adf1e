"""Times the horizontal cost filter over a finished volume (sgm_volume_filter.hip,
profile class "vol_hfilter") against its two yardsticks of the same session --
cost_h of a census frame of that size (the same chain, raw costs from LDS) and
a device-to-device copy of one view's bytes -- then the whole calls: a K128
aggregate and a K128 SAD frame with both filters against setting 0.  HIP events
around each call, median of N after discarded warm-up runs; prints the table
kept in profiles/volume_filter_ab.txt.

    python tools/volume_filter_time.py [N]
"""
from __future__ import annotations

import functools
import sys

import torch

import event_time
from event_time import DEV, class_means, fmt, profile_of
from stereo_matching_amd import SGM, _capi, synthetic

N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
timed = functools.partial(event_time.timed, n=N)


def classes(s, fn):
    """Mean ms per launch class over N calls of fn, after one unprofiled call."""
    return class_means(profile_of(s, fn, N, warm=1))


def main():
    _capi.lib()
    print(f"# median of {N} (min..max) after 3 discarded runs, HIP events around the call; "
          f"block = {_capi.lib().sgm_volume_filter_block()} steps")
    for h, w, D in ((375, 1242, 128), (1080, 1920, 256)):
        left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
        d_l, d_r = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
        nvol = h * w * D
        for views in (1, 2):
            with SGM(h, w, 1, D, views=views) as s:
                stream = torch.cuda.ExternalStream(s.stream, device=DEV)
                res = torch.empty((h, w), dtype=torch.float32, device=DEV)
                vol = torch.rand((h, w, D), dtype=torch.float32, device=DEV) * 64.0
                twin = torch.empty((h, w, D), dtype=torch.float32, device=DEV)
                tag = f"{h}x{w}x{D} views={views}"
                if views == 1:
                    d2d = event_time.d2d_copy(s.stream)
                    c = timed(stream, lambda: d2d(twin.data_ptr(), vol.data_ptr(), nvol * 4))
                    print(f"{tag} memcpy d2d of one view: {fmt(c)}")
                    f1 = timed(stream, lambda: s.filter_volume(twin, True, False, stream=s.stream))
                    print(f"{tag} filter_volume H in place: {fmt(f1)}")
                census = classes(s, lambda: s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(),
                                                             stream=s.stream))
                print(f"{tag} census frame classes: cost_h {census.get('cost_h', 0):.3f}, vfwd {census.get('vfwd', 0):.3f}")
                agg = lambda: s.aggregate(vol, layout="hwd", out=res, stream=s.stream)  # noqa: E731
                off = timed(stream, agg)
                s.set_volume_filter(True, True)
                on = timed(stream, agg)
                prof = classes(s, agg)
                s.set_volume_filter(False, False)
                print(f"{tag} aggregate setting 0: {fmt(off)}   both filters: {fmt(on)}   diff {on[0] - off[0]:.3f} ms")
                print("    filtered aggregate classes (mean ms): " + ", ".join(f"{k} {v:.3f}" for k, v in prof.items()))
                if (h, D) == (375, 128):
                    s.set_cost("sad")
                    frame = lambda: s.process_device(d_l.data_ptr(), d_r.data_ptr(), res.data_ptr(),  # noqa: E731
                                                     stream=s.stream)
                    off = timed(stream, frame)
                    s.set_volume_filter(True, True)
                    on = timed(stream, frame)
                    print(f"{tag} SAD frame setting 0: {fmt(off)}   both filters: {fmt(on)}   diff {on[0] - off[0]:.3f} ms")
                s.check()
                del vol, twin


if __name__ == "__main__":
    main()
