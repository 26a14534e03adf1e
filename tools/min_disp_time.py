#!/usr/bin/env python3
"""Frame times of a minimum disparity (sgm_set_min_disp): its cost, and what it buys.

One process, one device, two views.  Two kinds of measurement:

  cost    m = 0, m = 64, m = 0, m = 64, ... at one (size, D): REPS alternating
          legs each; the m = 0 legs' spread is the pairing's own noise.
  payoff  D = 128 with m = 64 against D = 256 with m = 0 on the SAME pair
          (generated for 256 disparities: rows with ground truth in [64, 192)
          are served by both), alternating REPS times; the frame-time ratio.

Each leg: a fresh handle, 3 warm-up frames, then 20 frames each bracketed by
HIP events on the handle's own stream, median reported, sgm_check after the leg;
then one profiled frame for the per-kernel table (in the --out file).

    python tools/min_disp_time.py [--out FILE] [--reps 3] [--what cost,payoff] [--sizes k128,hd256]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COST = {"k128": (375, 1242, 128), "hd256": (1080, 1920, 256)}
PAYOFF = {"k": (375, 1242), "hd": (1080, 1920)}
WARMUP, FRAMES = 3, 20


def leg(torch, dev, h, w, D, m, dgen, lines, tag):
    from stereo_matching_amd import SGM, synthetic
    left, right = synthetic.stereo_pair(h, w, dgen, pair_index=0)
    d_left = torch.from_numpy(left).to(dev)
    d_right = torch.from_numpy(right).to(dev)
    d_out = torch.empty((h, w), dtype=torch.float32, device=dev)
    with SGM(h, w, 1, D, views=2, device=dev.index, min_disp=m) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)

        def frame():
            sgm.process_device(d_left.data_ptr(), d_right.data_ptr(), d_out.data_ptr())

        with torch.cuda.stream(stream):
            for _ in range(WARMUP):
                frame()
            stream.synchronize()
            sgm.check()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(FRAMES)]
            for a, b in evs:
                a.record(stream)
                frame()
                b.record(stream)
            stream.synchronize()
            sgm.check()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        med = statistics.median(ms)
        sgm.set_profiling(True)
        frame()
        sgm.check()
        prof = sgm.get_profile()
        nbytes = sgm.device_bytes
        valid = float((d_out <= D + m - 1).float().mean().item())
    shift = prof.get("ct_shift", (0, 0.0, 0))[1] * 1e3
    lines.append(f"{tag:8s} {h}x{w} D={D:<3d} m={m:<3d} median {med:8.4f} ms  min {ms[0]:8.4f}  "
                 f"max {ms[-1]:8.4f}  ct_shift {shift:6.1f} us  valid {valid:.3f}  "
                 f"device {nbytes / 2**20:9.1f} MiB")
    print(lines[-1], flush=True)
    for name, (n, total_ms, elems) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"{'':8s}   {name:20s} x{n:<3d} {total_ms * 1e3:10.1f} us")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--what", default="cost,payoff")
    ap.add_argument("--sizes", default=",".join(COST), help="the cost legs' sizes")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    lines = [f"# {torch.cuda.get_device_name(0)}; two views; {WARMUP} warm-ups, median of {FRAMES} frames, "
             f"HIP events on the handle's stream; {args.reps} alternating legs per variant"]
    summary = []
    what = args.what.split(",")
    if "cost" in what:
        for name in args.sizes.split(","):
            h, w, D = COST[name]
            a, b = [], []
            for _ in range(args.reps):
                a.append(leg(torch, dev, h, w, D, 0, D, lines, name))
                b.append(leg(torch, dev, h, w, D, 64, D, lines, name))
            ma, mb = statistics.median(a), statistics.median(b)
            summary.append(f"cost   {name:6s} m=0 {ma:.4f} ms (legs {min(a):.4f}..{max(a):.4f}), "
                           f"m=64 {mb:.4f} ms (legs {min(b):.4f}..{max(b):.4f}): {100 * (mb / ma - 1):+.2f}%, "
                           f"m=0 spread {100 * (max(a) / min(a) - 1):.2f}%")
    if "payoff" in what:
        for name, (h, w) in PAYOFF.items():
            a, b = [], []
            for _ in range(args.reps):
                a.append(leg(torch, dev, h, w, 256, 0, 256, lines, name + "256"))
                b.append(leg(torch, dev, h, w, 128, 64, 256, lines, name + "128m"))
            ma, mb = statistics.median(a), statistics.median(b)
            summary.append(f"payoff {h}x{w} D=256 m=0 {ma:.4f} ms (legs {min(a):.4f}..{max(a):.4f}), "
                           f"D=128 m=64 {mb:.4f} ms (legs {min(b):.4f}..{max(b):.4f}): "
                           f"x{mb / ma:.3f} of the frame time")
    lines.append("")
    lines.extend(summary)
    print("\n".join(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
