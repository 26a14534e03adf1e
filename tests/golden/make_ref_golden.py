"""Generate the ref_* fixtures in tests/golden/ from the REFERENCE's own code.

Run from the repo root, after build() (or oracle.build_ref()) has compiled the
reference's sources into oracle/_ref/:

    python tests/golden/make_ref_golden.py

Unlike make_golden.py, nothing here comes from oracle/sgm_oracle.c: every
array is what hilbertw/stereo_matching's src/{Solver,SGM,cost,BM}.cpp computed
when run through oracle/ref/ref_driver.cpp.  The pre-blur is the one stand-in
(the pinned fixed-point formula, or identity for the *_noblur cases).

Per case, ref_<name>.npz holds every H x W output in full (working images,
census words, raw disparities of both views, sub-pixel maps, the LR map, the
post-filtered map, BM's raw disparity, compute_subpixel on drawn disparities)
and, for every volume (cost at three points, L1..L8 and their sum, both
views), the D-vectors of up to 64 seeded pixels that always include the four
corners; ref_<name>_b.npz holds the right view's vectors, and
ref_hashes.json holds each volume's sha256 and the set's statistics.
ref_maps.npz holds post_filter() and colormap() on the arbitrary maps of
tests/postfilter_maps.py.  Inputs are regenerated from seeds (inputs(),
map_inputs()) and not stored.

The SGM stages run with 1 OpenMP thread here; tests/test_reference_parity.py
repeats everything before post_filter with 8 (speckle_filter_new races,
SURVEY.md section 5).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from stereo_matching_amd import synthetic  # noqa: E402
import postfilter_maps  # noqa: E402

# name: (h, w, D, scale, kind, sky, blur, pair_index) -- all inside the
# reference's domain: D in {32, 64, 128}, scale in {1, 2} (Solver.cpp:8-10)
CASES = {
    "min_3x5_D32": (3, 5, 32, 1, "noise", False, True, 0),          # 3s x 5s minimum frame
    "min_s2_6x10_D32": (6, 10, 32, 2, "noise", False, True, 1),     # the same at scale 2
    "narrow_20x40_D128_noblur": (20, 40, 128, 1, "road", False, False, 2),   # W < D
    "edge_24x33_D32": (24, 33, 32, 1, "noise", False, True, 3),     # W = D + 1, noise
    "road_48x96_D32": (48, 96, 32, 1, "road", False, True, 4),      # W = 3 D
    "odd_s2_sky_51x99_D32": (51, 99, 32, 2, "road", True, True, 5),  # odd H and W at scale 2
    "const_16x40_D32": (16, 40, 32, 1, "const", False, True, 7),    # every cost ties
    "road_sky_48x170_D64": (48, 170, 64, 1, "road", True, True, 8),
}
VOLUMES = (["dsi", "hf", "vf"] + [f"L{k}" for k in range(1, 9)] + ["S"]
           + ["dsi_b", "hf_b", "vf_b"] + [f"L{k}_b" for k in range(1, 9)] + ["S_b"])
MAPS = ["img_l", "img_r", "ct_l", "ct_r", "disp", "disp_b", "sub", "sub_b", "lr", "final"]
N_SAMPLES = 64

# post_filter() / colormap() on arbitrary maps: (kind, H, W, D, scale, seed)
PF_CASES = [(k, 44, 100, 64, 1, i) for i, k in enumerate(postfilter_maps.KINDS)] + [
    ("random_holes", 40, 90, 32, 2, 20), ("speckle", 40, 90, 128, 2, 21), ("snake", 33, 77, 32, 2, 22)]
CM_CASES = [("random_holes", 20, 64, 32, 30), ("odd_invalid", 20, 64, 64, 31), ("all_valid", 20, 64, 128, 32)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def save_npz(path, arrays):
    """An .npz that np.load reads, LZMA-compressed: the sampled float vectors
    shrink to about 40% (deflate: 55%), which keeps the set inside its budget."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as zf:
        for k, v in arrays.items():
            zi = zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_LZMA
            with zf.open(zi, "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(v), allow_pickle=False)


def load_case(name):
    """Both fixture files of a case as one dict (meta decoded)."""
    out = {}
    for suffix in ("", "_b"):
        with np.load(os.path.join(HERE, f"ref_{name}{suffix}.npz")) as z:
            out.update({k: z[k] for k in z.files})
    out["meta"] = json.loads(str(out["meta"]))
    return out


def inputs(meta):
    """(left, right, sky_l, sky_r) of a case; the masks differ between the
    views so that swapping them cannot pass."""
    h, w, D, s = meta["h"], meta["w"], meta["D"], meta["scale"]
    if meta["kind"] == "const":
        left = np.full((h, w), 117, np.uint8)
        right = left.copy()
    else:
        left, right = synthetic.stereo_pair(h, w, D, meta["pair_index"], meta["kind"])
    sky_l = sky_r = None
    if meta["sky"]:
        H, W = h // s, w // s
        sky_l = synthetic.sky_mask(H, W)
        sky_r = sky_l.copy()
        sky_r[:, : W // 3] = 0
        sky_r[H // 6, W // 2:] = 255
    return left, right, sky_l, sky_r


def sample_pixels(name, H, W):
    """Flat indices of up to 64 pixels, the four corners first."""
    corners = [0, W - 1, (H - 1) * W, H * W - 1]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rest = [int(i) for i in rng.permutation(H * W) if int(i) not in corners]
    return np.array((corners + rest)[: min(N_SAMPLES, H * W)], np.int64)


def subpixel_input(name, H, W, D):
    """Disparities for compute_subpixel() on the right view's summed volume:
    every branch (0, D-1, interior, invalid D+1)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 0x5B)
    d = rng.integers(0, D, (H, W))
    d[rng.random((H, W)) < 0.1] = D + 1
    d[rng.random((H, W)) < 0.05] = D - 1
    d[rng.random((H, W)) < 0.05] = 0
    return d.astype(np.float32)


def map_inputs():
    """{key: (map, D, scale)} for ref_maps.npz, regenerated from seeds."""
    out = {}
    for kind, H, W, D, s, seed in PF_CASES:
        out[f"pf_{kind}_{H}x{W}_D{D}_s{s}"] = (postfilter_maps.make(kind, H, W, D, seed), D, s)
    for kind, H, W, D, seed in CM_CASES:
        f = postfilter_maps.make(kind, H, W, D, seed)
        # the colour ramp's segment ends (51, 102, 153, 204 after the 256/D
        # scaling) and both ends of the range
        edges = np.array([0, 51, 51.5, 102, 102.25, 153, 153.5, 204, 204.5, 255], np.float32) / (256 // D)
        f[0, : edges.size] = np.minimum(edges, D - 1)
        out[f"cm_{kind}_{H}x{W}_D{D}"] = (f, D, 1)
    return out


def run_case(oracle, name, threads=1, with_post=True):
    """Everything the reference computes for one case: (maps, volumes)."""
    h, w, D, s, kind, sky, blur, idx = CASES[name]
    meta = dict(h=h, w=w, D=D, scale=s, kind=kind, sky=sky, blur=blur, pair_index=idx)
    left, right, sl, sr = inputs(meta)
    kw = dict(sky_l=sl, sky_r=sr, blur=blur, threads=threads)
    proc = oracle.run_ref("process", left, right, D, s, **kw)
    stages = oracle.run_ref("stages", left, right, D, s, **kw)
    for k in ("img_l", "img_r", "ct_l", "ct_r", "dsi", "vf", "dsi_b", "vf_b"):
        assert np.array_equal(stages[k], proc[k]), (name, k, "stages and process modes differ")
    vols = {k: (stages[k] if k.startswith("hf") else proc[k]) for k in VOLUMES}
    maps = {k: proc[k] for k in MAPS}
    if not with_post:
        del maps["final"]
    H, W = h // s, w // s
    bm = oracle.run_ref("bm", left, right, D, s, **kw)
    maps["bm_disp"] = bm["disp"]
    if s > 1:   # BM.cpp:23-24 decimates columns only, so its census differs from SGM's
        maps["bm_ct_l"], maps["bm_ct_r"] = bm["ct_l"], bm["ct_r"]
    else:
        assert np.array_equal(bm["ct_l"], proc["ct_l"]) and np.array_equal(bm["ct_r"], proc["ct_r"])
    din = subpixel_input(name, H, W, D)
    maps["subpixel"] = oracle.run_ref("subpixel", left, right, D, s, fmap=din, **kw)["subpixel"]
    # where compute_subpixel's quotient is +inf (Solver.cpp:593 then clamps it
    # to D-1): classified with numpy, only for the set's statistics
    S, d = vols["S_b"], np.clip(din.astype(np.int64), 1, D - 2)
    c0, cm, cp = (np.take_along_axis(S, (d + o)[..., None], 2)[..., 0] for o in (0, -1, 1))
    with np.errstate(all="ignore"):
        q = (cm - cp) / (np.float32(2) * (cm + cp - np.float32(2) * c0))
    meta["inf_subpixel"] = int(np.sum(np.isposinf(q) & (din >= 1) & (din <= D - 2)
                                      & (maps["subpixel"] == D - 1)))
    return meta, maps, vols


def stats(meta, maps):
    D = meta["D"]
    sub, lr, final = maps["sub"], maps["lr"], maps["final"]
    d = maps["disp"].astype(np.int64)
    inf_sub = meta["inf_subpixel"]
    _, _, sl, _ = inputs(meta)
    return dict(valid_lr=float(np.mean(lr <= D - 1)), valid_final=float(np.mean(final <= D - 1)),
                uniq_rejected=int(np.sum(d == D + 1)),
                lr_rejected=int(np.sum((sub <= D - 1) & (lr > D - 1))),
                inf_subpixel=inf_sub, sky_pixels=0 if sl is None else int(np.sum(sl == 255)))


def check_set(all_stats):
    """The conditions the fixture set must meet, on the reference's output."""
    v = list(all_stats.values())
    assert sum(s["valid_lr"] > 0.5 for s in v) >= 3, "need >= 3 frames with > 50% valid LR pixels"
    assert sum(s["valid_final"] > 0.25 for s in v) >= 2, "need >= 2 frames > 25% valid after post_filter"
    assert any(s["uniq_rejected"] > 0 for s in v), "need a frame with uniqueness rejections"
    assert any(s["lr_rejected"] > 0 for s in v), "need a frame with LR rejections"
    assert any(s["inf_subpixel"] > 0 for s in v), "need a frame with a +inf -> D-1 sub-pixel pixel"
    assert any(s["sky_pixels"] > 0 for s in v), "need a frame with a sky pixel"


def run_maps(oracle):
    out = {}
    for key, (f, D, s) in map_inputs().items():
        H, W = f.shape
        img = np.zeros((H * s, W * s), np.uint8)
        mode = "post_filter" if key.startswith("pf_") else "colormap"
        out[key] = oracle.run_ref(mode, img, img, D, s, fmap=f, threads=1)[mode]
    return out


def main():
    import oracle
    if oracle.build_ref() is None:
        raise SystemExit("no reference checkout found (SGM_REFERENCE_DIR)")
    hashes, all_stats = {}, {}
    for name in CASES:
        meta, maps, vols = run_case(oracle, name)
        H, W = maps["disp"].shape
        idx = sample_pixels(name, H, W)
        smp = {"smp_" + k: v.reshape(H * W, -1)[idx] for k, v in vols.items()}
        all_stats[name] = stats(meta, maps)
        del meta["inf_subpixel"]
        path = os.path.join(HERE, f"ref_{name}.npz")
        left_view = {k: v for k, v in smp.items() if not k.endswith("_b")}
        save_npz(path, dict(meta=np.array(json.dumps(meta)), sample_idx=idx, **maps, **left_view))
        save_npz(path[:-4] + "_b.npz", {k: v for k, v in smp.items() if k.endswith("_b")})
        hashes[name] = {k: sha(v) for k, v in vols.items()}
        print(f"{name}: {os.path.getsize(path)} + {os.path.getsize(path[:-4] + '_b.npz')} bytes",
              all_stats[name])
    check_set(all_stats)
    path = os.path.join(HERE, "ref_maps.npz")
    save_npz(path, run_maps(oracle))
    print("ref_maps:", os.path.getsize(path), "bytes")
    with open(os.path.join(HERE, "ref_hashes.json"), "w") as fh:
        json.dump({"volumes": hashes, "stats": all_stats}, fh, indent=1, sort_keys=True)
    total = sum(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("ref_"))
    print("set:", total, "bytes")


if __name__ == "__main__":
    main()
