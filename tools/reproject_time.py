#!/usr/bin/env python3
"""Event time of the reprojection launch (sgm_set_reproject) and of
frames that end with it.

  launch    sgm_reproject_device on an aux_only handle at 1242x375 and 3840x2160,
            for the product sets XYZ, depth, XYZ + depth and all three, XYZ in
            both store forms of sgm_reproject.hip (SGM_REPROJECT_STORE = 0: one
            12-byte store per lane; 1: through LDS into 16-byte stores); beside
            each, a device-to-device copy that moves the same number of bytes
            (read plus written), timed in the same round on the same stream
  frame     the K128 one-view frame (375x1242, D = 128) and the 4K256 one-view
            frame (2160x3840, D = 256) with reprojection off and with all three
            products on

One process, one device.  REPS rounds over all the legs in turn; each leg: 3
warm-ups, then 20 launches (frames: 10; 4K256: 5) each bracketed by HIP events on
the handle's own stream; the median is reported.

    python tools/reproject_time.py [--out FILE] [--reps 3] [--no-4k]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((375, 1242, 128), (2160, 3840, 256))
SETS = (("xyz", 1), ("depth", 2), ("xyz+depth", 3), ("all three", 7))
BYTES = {1: 12, 2: 4, 4: 2}
WARMUP, LAUNCHES = 3, 20


def timed(torch, stream, fn, n):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    with torch.cuda.stream(stream):
        for _ in range(WARMUP):
            fn()
        for a, b in evs:
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in evs) * 1e3   # us


def launch_legs(torch, dev, H, W, D, res, lines):
    import numpy as np
    import reproject_recipe as rp
    from stereo_matching_amd import SGM, camera_q
    q = camera_q(721.5377, 721.5377, 609.5593, 172.854, 0.54)
    disp = torch.from_numpy(rp.hand_map(H, W, D, 0).astype(np.float32)).to(dev)
    xyz = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    d16 = torch.empty((H, W), dtype=torch.int16, device=dev)
    torch.cuda.synchronize(dev)
    for name, mask in SETS:
        total = H * W * (4 + sum(b for bit, b in BYTES.items() if mask & bit))
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for form in ((0, 1) if mask & 1 else (0,)):
            os.environ["SGM_REPROJECT_STORE"] = str(form)
            with SGM(H, W, 1, D, aux_only=True, device=dev.index) as sgm:
                sgm.set_reproject(q, outputs=(), max_range=80.0)
                stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
                us = timed(torch, stream, lambda: sgm.reproject_device(
                    disp.data_ptr(), d_xyz=xyz.data_ptr() if mask & 1 else 0,
                    d_depth=depth.data_ptr() if mask & 2 else 0, d_depth16=d16.data_ptr() if mask & 4 else 0),
                    LAUNCHES)
                sgm.check()
                cp = timed(torch, stream, lambda: dst.copy_(src, non_blocking=True), LAUNCHES)
            del os.environ["SGM_REPROJECT_STORE"]
            key = (f"{W}x{H}", name, form)
            res.setdefault(key, []).append((us, cp, total))
            lines.append(f"launch {W}x{H} {name:10s} form {form}: {us:8.2f} us  {total / us / 1e6:6.3f} TB/s | "
                         f"copy of {total // 2} B: {cp:8.2f} us  {total / cp / 1e6:6.3f} TB/s")
            print(lines[-1], flush=True)


def frame_legs(torch, dev, H, W, D, frames, res, lines):
    from stereo_matching_amd import SGM, camera_q, synthetic
    q = camera_q(721.5377, 721.5377, 609.5593, 172.854, 0.54)
    left, right = synthetic.stereo_pair(H, W, D, pair_index=0)
    d_left, d_right = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_out = torch.empty((H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    with SGM(H, W, 1, D, views=1, device=dev.index) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
        for on in (False, True, False, True):
            sgm.set_reproject(q if on else None, outputs=("xyz", "depth", "depth16"), max_range=80.0)
            ms = timed(torch, stream, lambda: sgm.process_device(d_left.data_ptr(), d_right.data_ptr(),
                                                                 d_out.data_ptr()), frames) / 1e3
            sgm.check()
            res.setdefault((f"frame {W}x{H} D={D} one view", "on" if on else "off", 0), []).append((ms, 0, 0))
            lines.append(f"frame {W}x{H} D={D} one view, reprojection {'on (all three)' if on else 'off':14s}: "
                         f"{ms:9.4f} ms")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-4k", action="store_true", help="skip the 4K256 frame (its handle holds tens of GB)")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    lines = [f"# {torch.cuda.get_device_name(0)}; {WARMUP} warm-ups, median of {LAUNCHES} launches (frames: 10; "
             f"4K256: 5), HIP events on the handle's stream; {args.reps} rounds over the legs"]
    res = {}
    for _ in range(args.reps):
        for H, W, D in SIZES:
            launch_legs(torch, dev, H, W, D, res, lines)
        frame_legs(torch, dev, 375, 1242, 128, 10, res, lines)
        if not args.no_4k:
            frame_legs(torch, dev, 2160, 3840, 256, 5, res, lines)
    lines.append("")
    lines.append("# medians over the rounds")
    for (size, name, form), v in res.items():
        us = statistics.median(x[0] for x in v)
        if v[0][2]:
            cp, total = statistics.median(x[1] for x in v), v[0][2]
            lines.append(f"launch {size} {name:10s} form {form}: {us:8.2f} us  {total / us / 1e6:6.3f} TB/s | copy "
                         f"{cp:8.2f} us  {total / cp / 1e6:6.3f} TB/s | launch / copy {us / cp:5.2f}")
        else:
            lines.append(f"{size}, reprojection {name:3s}: {us:9.4f} ms "
                         f"(legs {min(x[0] for x in v):.4f}..{max(x[0] for x in v):.4f})")
    print("\n".join(lines[-len(res) - 1:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
