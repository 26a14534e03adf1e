#!/usr/bin/env python3
"""Event time of the hole filling (sgm_set_fill) and of frames that
end with it.

  launch   sgm_fill_device on an aux_only handle at 375x1242 (D = 128) and
           2160x3840 (D = 256), both modes, on a map with 30% invalid pixels (and a
           right map of the same kind); the handle's own profile splits the call
           into its two launches, fill_march and fill_select, and the march's time
           per row step is reported beside them.  Beside each, a device-to-device
           copy of the bytes the stage moves at most: six planes written and read,
           the map read twice and written once, the mask.
  frame    the K128 two-view frame (375x1242, D = 128) with fill off, background
           and interpolate, the legs in turn on one handle

    python tools/fill_time.py [--out FILE] [--reps 3] [--no-4k]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = ((375, 1242, 128), (2160, 3840, 256))


def launch_legs(H, W, D, lines):
    import numpy as np
    import torch
    import event_time as et
    from stereo_matching_amd import SGM
    rng = np.random.default_rng(1)

    def a_map():
        F = (rng.random((H, W)) * (D - 1)).astype(np.float32)
        F[rng.random((H, W)) < 0.3] = D + 1
        return torch.from_numpy(F).to(et.DEV)

    src, right, work = a_map(), a_map(), torch.empty((H, W), dtype=torch.float32, device=et.DEV)
    mask = torch.empty((H, W), dtype=torch.uint8, device=et.DEV)
    moved = H * W * (6 * 4 * 2 + 3 * 4 + 1)
    a, b = torch.empty(moved // 2, dtype=torch.uint8, device=et.DEV), torch.empty(moved // 2, dtype=torch.uint8, device=et.DEV)
    torch.cuda.synchronize(et.DEV)
    with SGM(H, W, 1, D, aux_only=True, fill="background") as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=et.DEV)
        copy = et.d2d_copy(sgm.stream)
        for mode in ("background", "interpolate"):
            def call():
                copy(work.data_ptr(), src.data_ptr(), H * W * 4)    # (the fill is in place: a fresh map each time)
                sgm.fill_device(work.data_ptr(), d_right=right.data_ptr(), mode=mode, d_mask=mask.data_ptr())
            t = et.timed(stream, call, 20)
            means = et.class_means(et.profile_of(sgm, call, 20, warm=3))
            step = means["fill_march"] / H * 1e3
            lines.append(f"launch {W}x{H} D={D} {mode:11s}: map copy + fill {et.fmt(t)} | fill_march "
                         f"{means['fill_march'] * 1e3:8.1f} us ({step:6.3f} us per row step, {H} steps) | fill_select "
                         f"{means['fill_select'] * 1e3:8.1f} us ({means['fill_select'] / H * 1e3:6.3f} us per row)")
            print(lines[-1], flush=True)
        c = et.timed(stream, lambda: copy(b.data_ptr(), a.data_ptr(), moved // 2), 20)
        lines.append(f"launch {W}x{H} d2d copy moving {moved} B (6 planes written and read, the map twice read and "
                     f"once written, the mask): {et.fmt(c)}  {moved / c[0] / 1e9:6.3f} TB/s")
        print(lines[-1], flush=True)


def frame_legs(H, W, D, reps, lines):
    import torch
    import event_time as et
    from stereo_matching_amd import SGM, synthetic
    left, right = synthetic.stereo_pair(H, W, D, pair_index=0)
    d_left, d_right = torch.from_numpy(left).to(et.DEV), torch.from_numpy(right).to(et.DEV)
    d_out = torch.empty((H, W), dtype=torch.float32, device=et.DEV)
    torch.cuda.synchronize(et.DEV)
    res = {}
    with SGM(H, W, 1, D, views=2) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=et.DEV)
        base = sgm.device_bytes
        for _ in range(reps):
            for mode in ("off", "background", "interpolate"):
                sgm.set_fill(mode)
                t = et.timed(stream, lambda: sgm.process_device(d_left.data_ptr(), d_right.data_ptr(), d_out.data_ptr()),
                             20, warm=5)
                sgm.check()
                res.setdefault(mode, []).append(t[0])
                lines.append(f"frame {W}x{H} D={D} two views, fill {mode:11s}: {et.fmt(t, 4)}  "
                             f"(+{sgm.device_bytes - base} B of scratch)")
                print(lines[-1], flush=True)
        sgm.set_fill("off")
    lines.append("# medians over the rounds")
    for mode, v in res.items():
        lines.append(f"frame {W}x{H} D={D} two views, fill {mode:11s}: {statistics.median(v):8.4f} ms "
                     f"(rounds {min(v):.4f}..{max(v):.4f}; over off {statistics.median(v) - statistics.median(res['off']):+.4f})")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-4k", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    lines = [f"# {torch.cuda.get_device_name(0)}; tools/fill_time.py: HIP events around each call, a synchronise after "
             "each, median (min..max) of 20 after warm-ups; the launches' own times from the handle's profile"]
    for H, W, D in SIZES[:1 if args.no_4k else 2]:
        launch_legs(H, W, D, lines)
    frame_legs(375, 1242, 128, args.reps, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
