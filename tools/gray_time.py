#!/usr/bin/env python3
"""Event time of the colour input's launches (sgm_set_input_format, DESIGN.md
5l) at the node's sizes, one view, D = 128:

  gray      the stand-alone conversion of both 1242x375 images (a 375x1242
            handle with a colour format and no input stage), BGR8 and BGRA8
  resize    375x1242 -> 360x1240: grey images (the launch of DESIGN.md 5j), then
            colour images (the fused launch, which converts its taps)
  rectify   the same through the test generator's maps (tests/rectify_recipe.py)

so that each fused launch stands beside the sum of the conversion and the grey
launch it replaces, measured in one session.

One process, one device.  REPS rounds over all the legs in turn; each leg: a
fresh handle, 3 warm-up frames, 20 frames each bracketed by HIP events on the
handle's own stream (median reported), sgm_check, then 20 profiled frames for
the first launch's class event time per launch (both images, one launch).

    python tools/gray_time.py [--out FILE] [--reps 3]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RAW, FULL, D = (375, 1242), (360, 1240), 128
WARMUP, FRAMES = 3, 20
# (name, handle size, stage, format, the profile class of the frame's first launch)
LEGS = [
    ("gray bgr8", RAW, None, "bgr8", "gray"),
    ("gray bgra8", RAW, None, "bgra8", "gray"),
    ("resize gray8", FULL, "size", "gray8", "resize"),
    ("resize bgr8", FULL, "size", "bgr8", "resize"),
    ("resize bgra8", FULL, "size", "bgra8", "resize"),
    ("rectify gray8", FULL, "rectify", "gray8", "rectify"),
    ("rectify bgr8", FULL, "rectify", "bgr8", "rectify"),
    ("rectify bgra8", FULL, "rectify", "bgra8", "rectify"),
]


def leg(torch, dev, name, size, stage, fmt, cls, lines):
    import gray_recipe as gr
    import rectify_recipe as rc
    from stereo_matching_amd import SGM, synthetic
    left, right = synthetic.stereo_pair(RAW[0], RAW[1], D, pair_index=0)
    if fmt != "gray8":
        left, right = gr.from_gray(left, fmt), gr.from_gray(right, fmt)
    d_left = torch.from_numpy(left).to(dev)
    d_right = torch.from_numpy(right).to(dev)
    d_out = torch.empty(size, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    kw = {}
    if stage == "size":
        kw["input_size"] = RAW
    if stage == "rectify":
        kw["rectify"] = (*RAW, *rc.maps(*FULL, *RAW, 0), *rc.maps(*FULL, *RAW, 1))
    with SGM(size[0], size[1], 1, D, views=1, device=dev.index, input_format=fmt, **kw) as sgm:
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
    n, total_ms, _ = prof.get(cls, (0, 0.0, 0))
    per = total_ms * 1e3 / n if n else 0.0
    lines.append(f"{name:14s} {RAW[0]}x{RAW[1]} -> {size[0]}x{size[1]} D={D} one view  median {med:8.4f} ms  "
                 f"min {ms[0]:8.4f}  max {ms[-1]:8.4f}  {cls} x{n} {per:5.2f} us per launch")
    print(lines[-1], flush=True)
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    lines = [f"# {torch.cuda.get_device_name(0)}; {WARMUP} warm-ups, median of {FRAMES} frames, HIP events on "
             f"the handle's stream; {args.reps} rounds over the legs"]
    per = {name: [] for name, *_ in LEGS}
    for _ in range(args.reps):
        for name, size, stage, fmt, cls in LEGS:
            per[name].append(leg(torch, dev, name, size, stage, fmt, cls, lines))
    med = {k: statistics.median(v) for k, v in per.items()}
    lines.append("")
    for name in per:
        lines.append(f"{name:14s} {med[name]:5.2f} us per launch (rounds {min(per[name]):.2f}..{max(per[name]):.2f})")
    for stage in ("resize", "rectify"):
        for fmt in ("bgr8", "bgra8"):
            two = med[f"gray {fmt}"] + med[f"{stage} gray8"]
            lines.append(f"fused {stage} {fmt}: {med[f'{stage} {fmt}']:.2f} us against gray + grey {stage} = "
                         f"{med[f'gray {fmt}']:.2f} + {med[f'{stage} gray8']:.2f} = {two:.2f} us")
    print("\n".join(lines[-len(per) - 4:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
