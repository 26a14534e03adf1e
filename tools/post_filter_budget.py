#!/usr/bin/env python3
"""Sizes the median fill's launch budget (sgm_set_post_filter_launches) and
times what it buys, on bench.py's full-pipeline shapes (sky detector + SGM +
LR check + post_filter + LKRefine, two views).

One process, one device.  Per shape, on PAIRS synthetic pairs:
  1. adaptive fill (budget 0: the host reads the convergence counter), eager:
     sgm_post_filter_proved_at after each of PROBE frames per pair, then
     ms per frame (wall clock over FRAMES frames on the handle's stream, one
     synchronise at the end, as bench.py times its steps);
  2. budget = max proved_at seen + 2, eager: proved_at again, ms per frame,
     sgm_check after the leg (an unproven fill would raise);
  3. the same budget captured once as a HIP graph and replayed: ms per frame,
     sgm_check;
  4. one no-op fill launch (a launch after the proof returns at its first
     instruction): the same legs at budget + EXTRA, difference / EXTRA, eager
     and replayed.
Each timed leg is run REPEATS times; the median and the spread are recorded.

    python tools/post_filter_budget.py [--out FILE.json] [--shapes k128full,4k256full]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # bench.py CONFIGS
    "k128full": (375, 1242, 128),
    "4k256full": (2160, 3840, 256),
}
PAIRS, PROBE, WARMUP, FRAMES, REPEATS, EXTRA = 3, 10, 3, 20, 5, 64


def run_shape(torch, dev, name, frames):
    from stereo_matching_amd import SGM, synthetic
    h, w, D = SHAPES[name]
    pairs = [synthetic.stereo_pair(h, w, D, pair_index=k) for k in range(PAIRS)]
    d_pairs = [(torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)) for l, r in pairs]
    d_l, d_r = torch.empty_like(d_pairs[0][0]), torch.empty_like(d_pairs[0][1])
    d_out = torch.empty((h, w), dtype=torch.float32, device=dev)
    res = {"h": h, "w": w, "D": D, "bound": -(-w // 64) * h + 1, "frames_per_leg": frames,
           "repeats": REPEATS}
    with SGM(h, w, 1, D, views=2, device=dev.index, post_filter=True, lk_refine=True,
             sky_detect=True) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)

        def load(k):
            with torch.cuda.stream(stream):
                d_l.copy_(d_pairs[k][0])
                d_r.copy_(d_pairs[k][1])

        def frame():
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), d_out.data_ptr())

        def probe():
            seen = []
            for k in range(PAIRS):
                load(k)
                for _ in range(PROBE):
                    frame()
                    seen.append(sgm.post_filter_proved_at())   # waits for the frame
            sgm.check()
            return seen

        def timed(step):
            load(0)
            ms = []
            for _ in range(REPEATS):
                for _ in range(WARMUP):
                    step()
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(frames):
                    step()
                stream.synchronize()
                ms.append((time.perf_counter() - t0) / frames * 1e3)
                sgm.check()
            return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                    "max_ms": round(max(ms), 4)}

        def replayed(budget):
            sgm.set_post_filter_launches(budget)
            load(0)
            frame()
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
                frame()
            stream.synchronize()

            def step():
                with torch.cuda.stream(stream):
                    graph.replay()
            out = timed(step)
            out["proved_at_after_replay"] = sgm.post_filter_proved_at()
            del graph
            return out

        sgm.set_post_filter_launches(0)
        seen = probe()
        res["adaptive"] = {"proved_at": seen, **timed(frame)}
        budget = max(seen) + 2
        res["budget"] = budget
        sgm.set_post_filter_launches(budget)
        res["budget_eager"] = {"proved_at": probe(), **timed(frame)}
        res["budget_graph"] = replayed(budget)
        sgm.set_post_filter_launches(budget + EXTRA)
        res["budget_plus_extra_eager"] = timed(frame)
        res["budget_plus_extra_graph"] = replayed(budget + EXTRA)
        res["extra_launches"] = EXTRA
        for kind in ("eager", "graph"):
            d = res[f"budget_plus_extra_{kind}"]["median_ms"] - res[f"budget_{kind}"]["median_ms"]
            res[f"noop_launch_us_{kind}"] = round(d / EXTRA * 1e3, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--frames", type=int, default=FRAMES)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    out = {"device": torch.cuda.get_device_name(0),
           "tree": "every leg, the adaptive one included, runs the library built from the tree "
                   "this file was recorded with (budget 0 = its adaptive fill)",
           "method": "wall clock over frames_per_leg frames on the handle's stream, one "
                     "synchronise at the end; median/min/max of `repeats` such legs"}
    for name in args.shapes.split(","):
        out[name] = run_shape(torch, dev, name, args.frames)
        print(name, json.dumps(out[name]), flush=True)
        if args.out:   # after every shape: a later shape's failure keeps the earlier numbers
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
