#!/usr/bin/env python3
"""Frame time of the rectification remap (sgm_set_rectify): the K128 one-view
frame at the node's sizes, raw 1242x375 camera images remapped to 1240x360
through the test generator's maps (tests/rectify_recipe.py), D = 128, against
the same 1240x360 frame fed full-size images.

One process, one device.  REPS alternating legs per variant (off, on, off, on,
...; --legs off or on: that variant alone, for pairing processes of two
checkouts: the off leg uses nothing the parent commit lacks); the off legs'
spread is the pairing's own noise.  Each leg: a fresh handle, 3 warm-up frames,
then 20 frames each bracketed by HIP events on the handle's own stream, median
reported, sgm_check after the leg; then 20 profiled frames for the `rectify`
class's event time per launch.

    python tools/rectify_time.py [--out FILE] [--reps 3] [--legs both|off|on] [--label NAME]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAW, FULL, D = (375, 1242), (360, 1240), 128
WARMUP, FRAMES = 3, 20


def leg(torch, dev, on, label, lines):
    from stereo_matching_amd import SGM, synthetic
    h, w = RAW if on else FULL
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    d_left = torch.from_numpy(left).to(dev)
    d_right = torch.from_numpy(right).to(dev)
    d_out = torch.empty(FULL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    kw = {}
    if on:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import rectify_recipe as rc
        kw["rectify"] = (*RAW, *rc.maps(*FULL, *RAW, 0), *rc.maps(*FULL, *RAW, 1))
    with SGM(FULL[0], FULL[1], 1, D, views=1, device=dev.index, **kw) as sgm:
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
        for _ in range(FRAMES):
            frame()
        sgm.check()
        prof = sgm.get_profile()
        nbytes = sgm.device_bytes
    n, total_ms, _ = prof.get("rectify", (0, 0.0, 0))
    per = total_ms * 1e3 / n if n else 0.0
    lines.append(f"{label}rectify {'on ' if on else 'off'} {h}x{w} -> {FULL[0]}x{FULL[1]} D={D} one view  "
                 f"median {med:8.4f} ms  min {ms[0]:8.4f}  max {ms[-1]:8.4f}  "
                 f"rectify x{n} {per:5.2f} us per launch  device {nbytes / 2**20:8.1f} MiB")
    print(lines[-1], flush=True)
    return med, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", choices=("both", "off", "on"), default="both")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    label = args.label + " " if args.label else ""
    lines = [f"# {torch.cuda.get_device_name(0)}; {WARMUP} warm-ups, median of {FRAMES} frames, HIP events "
             f"on the handle's stream; {args.reps} legs per variant ({args.legs})"]
    off, on, per = [], [], []
    for _ in range(args.reps):
        if args.legs != "on":
            off.append(leg(torch, dev, False, label, lines)[0])
        if args.legs != "off":
            m, p = leg(torch, dev, True, label, lines)
            on.append(m)
            per.append(p)
    if off and on:
        a, b = statistics.median(off), statistics.median(on)
        lines.append("")
        lines.append(f"off {a:.4f} ms (legs {min(off):.4f}..{max(off):.4f}), on {b:.4f} ms (legs {min(on):.4f}.."
                     f"{max(on):.4f}): {1e3 * (b - a):+.1f} us, {100 * (b / a - 1):+.2f}%; off spread "
                     f"{100 * (max(off) / min(off) - 1):.2f}%; rectify event time {statistics.median(per):.2f} us "
                     f"per launch")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
