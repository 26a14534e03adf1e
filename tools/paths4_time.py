#!/usr/bin/env python3
"""Frame and per-kernel times of the 4-path mode against the 8-path one.

One process, one device.  Per size: paths=8, then paths=4, then paths=8 again
(the two 8-path legs give the run-to-run spread), then both forms of the
4-path schedule's H pair, forced by SGM_P4_HPAIR (read at sgm_create).  Each
leg: 3 warm-up frames, then 20 frames each bracketed by HIP events on the
handle's own stream, median reported, sgm_check after the leg; then one
profiled frame for the per-kernel table.

    python tools/paths4_time.py [--out FILE] [--sizes k128v1,k128v2,k64v2,hd256v2]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    "k128v1": (375, 1242, 128, 1),
    "k128v2": (375, 1242, 128, 2),
    "k64v2": (375, 1242, 64, 2),
    "hd256v2": (1080, 1920, 256, 2),
}
WARMUP, FRAMES = 3, 20


def leg(torch, dev, size, paths, env, lines):
    from stereo_matching_amd import SGM, synthetic
    h, w, D, views = SIZES[size]
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    d_left = torch.from_numpy(left).to(dev)
    d_right = torch.from_numpy(right).to(dev)
    d_out = torch.empty((h, w), dtype=torch.float32, device=dev)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sgm = SGM(h, w, 1, D, views=views, device=dev.index, paths=paths)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    with sgm:
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
        sgm.set_profiling(False)
        nbytes = sgm.device_bytes
    tag = f"paths={paths}" + "".join(f" {k}={v}" for k, v in env.items())
    lines.append(f"{size:8s} {tag:32s} median {med:8.4f} ms  min {ms[0]:8.4f}  max {ms[-1]:8.4f}  "
                 f"device {nbytes / 2**20:9.1f} MiB")
    for name, (n, total_ms, elems) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"{'':8s}   {name:20s} x{n:<3d} {total_ms * 1e3:10.1f} us")
    print("\n".join(lines[-(len(prof) + 1):]), flush=True)
    return med, prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    lines = [f"# {torch.cuda.get_device_name(0)}; {WARMUP} warm-ups, median of {FRAMES} frames, "
             f"HIP events on the handle's stream; one profiled frame per leg"]
    summary = []
    for size in args.sizes.split(","):
        a8, p8 = leg(torch, dev, size, 8, {}, lines)
        m4, p4 = leg(torch, dev, size, 4, {}, lines)
        b8, _ = leg(torch, dev, size, 8, {}, lines)
        alts = {}
        for env in ({"SGM_P4_HPAIR": "0"}, {"SGM_P4_HPAIR": "1"}):
            alts[next(iter(env.items()))] = leg(torch, dev, size, 4, env, lines)[0]
        hp = sum(v[1] for k, v in p4.items() if k.startswith("hpair4"))
        f8 = p8.get("pair_bwd_L4_final", p8.get("slant_up", (0, 0.0, 0)))[1]
        summary.append(
            f"{size:8s} 8-path {a8:.4f} / {b8:.4f} ms (spread {abs(a8 - b8):.4f}), 4-path {m4:.4f} ms: "
            f"x{m4 / a8:.3f} / x{m4 / b8:.3f} of the 8-path frame (bytes 33/74 = x0.446); "
            f"final pass 8-path {f8 * 1e3:.1f} us, 4-path {p4['final4'][1] * 1e3:.1f} us; "
            f"H pair {hp * 1e3:.1f} us; H pair forms "
            + ", ".join(f"{k}={v}: {t:.4f} ms" for (k, v), t in alts.items()))
    lines.append("")
    lines.extend(summary)
    print("\n".join(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
