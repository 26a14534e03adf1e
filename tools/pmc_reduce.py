"""Reduce rocprofv3 FETCH_SIZE / WRITE_SIZE passes to bytes per launch.

FETCH_SIZE and WRITE_SIZE are reported in KiB.  On gfx950 FETCH_SIZE counts
wide coalesced streaming reads at half their bytes (MI355X_MICROARCH.md,
"HBM"), so it is doubled; WRITE_SIZE is exact for streaming stores.
Usage: python tools/pmc_reduce.py TAG CONFIG  (after tools/pmc.sh)
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel symbol -> name used by the library's in-process profiler (bench.py)
NAMES = [("hpair_kernel", "stage_a_h"), ("stage_a_kernel", "stage_a"), ("stage_b_kernel", "stage_b"),
         ("pair_final_kernel", "pair_bwd_L4_final"),
         ("vfwd_kernel", "vfwd"), ("cost_h_kernel", "cost_h"), ("cost_h2_kernel", "cost_h"),
         ("cost_h_global_kernel", "cost_h"), ("cost_ck_kernel", "cost_ck"), ("vstrip_kernel", "vstrip"),
         ("sky_words_kernel", "sky_words"),
         ("census_kernel", "census"), ("lr_kernel", "lr"), ("lr_cm_kernel", "lr"), ("sweep_kernel<7", "sweep_L8_acc"),
         ("sweep_split_kernel<7", "sweep_L8_acc"),
         ("median_fill_kernel", "post_median"), ("cc_local_kernel", "post_cc_local"),
         ("cc_merge_kernel", "post_cc_merge"), ("cc_count_kernel", "post_cc_count"),
         ("cc_apply_kernel", "post_cc_apply"), ("pf_prep_kernel", "post_prep"),
         ("lk_refine_kernel", "lk_refine"), ("sky_columns_kernel", "sky_columns"),
         ("sky_gray_kernel", "sky_gray"), ("bm_wta_kernel", "bm_wta"),
         # 4-path frames' split H pair
         ("h_fwd_kernel", "hpair4_fwd"), ("h_bwd2_kernel", "hpair4_bwd"),
         # two-view kernels of their own
         ("stage_b2_kernel", "stage_b")]


def targ(name, key, i):
    """Template argument i of kernel `key` in a demangled symbol (None: another kernel, or fewer arguments)."""
    if key not in name:
        return None
    args = name[name.index(key) + len(key):].split(">")[0].split(", ")
    return args[i] if i < len(args) else None


def short(name):
    # (stage A, the finals, the L8 sweep and h_fwd carry the view count NV: one name for both)
    # stage_a_kernel<V, FULL, NV, ROLES>: ROLES 1 the forward bands' diagonal launches
    if targ(name, "stage_a_kernel<", 3) == "1":
        return "stage_a_d"
    # stage_b_kernel<V, FULL, HROWS>: without H rows the banded schedule's
    if targ(name, "stage_b_kernel<", 2) == "false":
        return "stage_b_d2"
    # the slanted passes
    if "slant_kernel<" in name:
        return "slant_up" if name.split("slant_kernel<")[1].startswith("true") else "slant_down"
    # vfwd_kernel<V, FULL, WIN, PF, BAND, L3OUT>, vfwd2_kernel<V, FULL, WIN, PF, L3OUT> (both views in one
    # launch): L3OUT writes the whole L3 volume
    if targ(name, "vfwd_kernel<", 5) == "true" or targ(name, "vfwd2_kernel<", 4) == "true":
        return "vfwd_l3"
    if "vfwd2_kernel<" in name:
        return "vfwd"
    # pair_final_kernel<V, FULL, NV, BAND, NTC, NOT>: NOT the 4-path frames' final
    if targ(name, "pair_final_kernel<", 5) == "true":
        return "final4"
    for key, val in NAMES:
        if key in name:
            return val
    return None


def per_launch(tag, counter):
    files = glob.glob(os.path.join(ROOT, "gpurun_out", f"{tag}_pmc_{counter}", "**",
                                   "*counter_collection.csv"), recursive=True)
    acc = defaultdict(list)
    for f in files:
        for row in csv.DictReader(open(f)):
            k = short(row.get("Kernel_Name", ""))
            if k and row.get("Counter_Name") == counter:
                acc[k].append(float(row["Counter_Value"]))
    return {k: sum(v) / len(v) for k, v in acc.items()}


def main():
    tag, cfg = sys.argv[1], sys.argv[2]
    fetch = per_launch(tag, "FETCH_SIZE")
    write = per_launch(tag, "WRITE_SIZE")
    out = {}
    for k in sorted(set(fetch) | set(write)):
        rd = 2.0 * fetch.get(k, 0.0) * 1024.0
        wr = write.get(k, 0.0) * 1024.0
        out[k] = {"read_bytes": rd, "write_bytes": wr, "bytes": rd + wr}
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    data = {}
    if os.path.exists(path):
        data = json.load(open(path))
    data[cfg] = {k: v["bytes"] for k, v in out.items()}
    data.setdefault("_detail", {})[cfg] = out
    sys.path.insert(0, ROOT)
    from bench import source_sha
    # the run tag, the commit the tree was taken from (GIT_SHA, passed in by
    # the caller: the GPU box has no .git) and the hash of the library's
    # sources, which bench.py compares with the code it runs
    data.setdefault("_tags", {})[cfg] = {"tag": tag, "git": os.environ.get("GIT_SHA", "unknown"),
                                         "src_sha": source_sha()}
    data["_source"] = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes (per config in "
                       "_tags: run tag, git commit, sha of the library sources); FETCH_SIZE "
                       "doubled (gfx950), KiB -> bytes; per-launch means; memory-side bytes "
                       "(Infinity Cache hits included, MI355X_MICROARCH.md 'HBM')")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    for k, v in out.items():
        print(f"  {k:22s} read {v['read_bytes']/1e6:9.1f} MB  write {v['write_bytes']/1e6:9.1f} MB")


if __name__ == "__main__":
    main()
