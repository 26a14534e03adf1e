"""Seeded random frames over the whole settings surface -- solver, D, scale,
blur, views, paths, min_disp, cost kind, window, weights, volume filters, P1,
P2, uniqueness, the LR threshold, post_filter (adaptive or under a launch
budget), confidence, fill, reprojection, shapes, image kinds and a sky mask per
view -- against tests/frame_recipe.py's composed CPU reference, bit for bit on
every map the handle reports.

CASES: case k is the candidate, of 168 drawn from np.random.default_rng(0x5E77
+ k), that adds most value pairs no earlier case holds (the first of equals).
The draw rejects what frame_recipe.refusal() refuses, and what cannot report a
map with valid and invalid pixels at these sizes (mixed_map_possible).  The
first 56 cases come from strata fixed by k (a cost kind, BM, GPU_SGM, the right
view, a census SGM frame); draw_cases() then goes on until every pair of values
of two axes that some accepted candidate holds is in a case, and until every
forced schedule below keeps two thirds of the SGM-solver cases: 206 cases.
tests/test_frame_recipe_cpu.py asserts all of that, and that every case's map
is mixed.

Sizes.  Census cases start inside tests/test_gpu_fuzz.py's bounds (working grid
up to 48 rows, W up to D + 60); a post-filtered case gets the rows for a
surface of 3.2 speckle sizes (1000 / s pixels) below its noise rows.  A sad /
ssd / ct case keeps H x W x D <= 600000 elements: window_recipe.window_volume
holds (H, e_h, W, D) int64 sums.  Measured on the CPU of the development
machine, one case's reference (frame_recipe.frame): 0.86 s for the first one
computed (case 00, which loads the oracle), 0.55 s for the slowest after it
(case 01, 107 x 51, D = 64, weighted SSD with a filter), all others under 0.5 s.

Forced schedules (SGM-solver cases only; a case whose plan falls back by design
is left out at collection, sgm_plan.h plan_handle and sgm_frame.hip frame_maps):
  SGM_SWEEP_SPLIT=0/1  the L8 sweep's two bodies: 8-path cases (a 4-path handle
                       has no L8); profile class "sweep_L8_acc", which both
                       bodies share: the profile shows that the L8 sweep ran,
                       not which body (nothing the library reports tells them
                       apart; that the switch reaches the launcher is
                       tests/test_gpu_fuzz.py's and the timing tools' matter)
  SGM_BAND_ROWS=16     bands: 8-path census cases of more than 16 rows (volume
                       frames run whole-volume passes; 16 rows or fewer are one
                       band, which the plan turns into none); "stage_b_d2"
  SGM_SLANT=1          slanted tiles: 8-path census cases; "slant_up"
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import frame_recipe
from frame_recipe import Settings, refusal
from support import bits
from stereo_matching_amd import BM, GPU_SGM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

N_DRAWN = 56
N_CANDIDATES = 168
VSTRIP_COLS = 16            # sgm_vstrip_cols(), asserted below
VOLUME_ELEMS = 600000       # H x W x D of a sad / ssd / ct case

# ------------------------------------------------------------------- axes
AXES = {
    "ctor": ("SGM", "BM", "GPU_SGM"),
    "D": (32, 64, 128, 256),
    "s": (1, 2),
    "shape": ("tiny", "narrow", "wide", "strip"),
    "kind": ("road", "noise"),
    "sky": ("none", "same", "differ"),
    "blur": (True, False),
    "views": ("two", "left", "right"),
    "paths": (8, 4),
    "min_disp": (0, 2, 16),
    "cost": ("census", "sad", "ssd", "ct"),
    "window": (None, (5, 5), (9, 7), (14, 18)),
    "weighted": (False, True),
    "volume_filter": ((False, False), (True, False), (False, True), (True, True)),
    "p1": (0, 10, 25),
    "p2": (10, 100, 300),
    "uniqueness": (0.5, 0.7, 1.0),
    "lr_max_diff": (0.0, 1.0, 2.5),
    "post": ("off", "adaptive", "budget"),
    "confidence": (False, True),
    "fill": ("off", "background", "interpolate"),
    "reproject": (False, True),
}


def pinhole_q():
    """reproject_recipe.camera_q's pinhole Q (the library's sgm_camera_q, without loading it)."""
    import reproject_recipe
    return tuple(reproject_recipe.camera_q(500.0, 500.0, 40.0, 20.0, 0.5))


Q = pinhole_q()


def stratum(k):
    """The part of the surface case k is drawn from."""
    if k < 18:
        return ("sad", "ssd", "ct")[k % 3]
    if k < 23:
        return "BM"
    if k < 28:
        return "GPU_SGM"
    if k < 34:
        return "right"
    return "census"


def pick(rng, values, p=None):
    return values[int(rng.choice(len(values), p=p))]


def draw(rng, part, uniform=False):
    """One candidate case (a dict of AXES' values plus the sizes), or None where refusal() refuses
    it.  uniform: every value of an axis equally likely (the universe of accepted pairs)."""
    a = {}
    a["ctor"] = part if part in ("BM", "GPU_SGM") else "SGM"
    sgm = a["ctor"] == "SGM"
    a["cost"] = part if part in ("sad", "ssd", "ct") else "census"
    census = a["cost"] == "census"
    a["D"] = pick(rng, AXES["D"])
    a["s"] = pick(rng, AXES["s"], None if uniform else (0.7, 0.3))
    # (the forced schedules keep 8-path census frames of more than 16 rows: those values are rare there)
    a["shape"] = pick(rng, AXES["shape"], None if uniform else (0.3, 0.25, 0.25, 0.2) if not census or a["ctor"] == "BM"
                      else (0.0, 0.34, 0.36, 0.3))
    a["kind"] = pick(rng, AXES["kind"])
    a["blur"] = pick(rng, AXES["blur"], None if uniform else (0.7, 0.3)) if a["ctor"] != "GPU_SGM" else True
    a["views"] = pick(rng, AXES["views"], None if uniform else (0.7, 0.3, 0.0)) if sgm else "left"
    if part == "right":
        a["views"] = "right"
    a["paths"] = pick(rng, AXES["paths"], None if uniform else (0.5, 0.5) if not census else (0.97, 0.03)) if sgm else 8
    a["min_disp"] = pick(rng, AXES["min_disp"], None if uniform else (0.5, 0.25, 0.25))
    a["window"] = pick(rng, AXES["window"])
    a["weighted"] = pick(rng, AXES["weighted"], None if uniform else (0.65, 0.35))
    a["volume_filter"] = pick(rng, AXES["volume_filter"]) if sgm else (False, False)
    for k in ("p1", "p2", "lr_max_diff"):
        a[k] = pick(rng, AXES[k]) if sgm else Settings.__dataclass_fields__[k].default
    a["uniqueness"] = pick(rng, AXES["uniqueness"]) if a["ctor"] != "GPU_SGM" else 0.7
    a["post"] = pick(rng, AXES["post"]) if sgm else pick(rng, ("adaptive", "budget"))
    a["confidence"] = pick(rng, AXES["confidence"]) if sgm else False
    a["fill"] = pick(rng, AXES["fill"], None if uniform else (0.4, 0.3, 0.3))
    a["reproject"] = pick(rng, AXES["reproject"])
    if a["views"] == "right" and (not uniform or part == "right"):   # (what a right-view handle takes)
        a.update(post="off", fill="off", volume_filter=(False, False), reproject=False)
    if a["views"] != "two" and a["fill"] == "interpolate" and not uniform:
        a["fill"] = "background"
    two_census = census and a["views"] == "two"
    a["sky"] = pick(rng, AXES["sky"], None if uniform else (0.15, 0.15, 0.7) if two_census else (0.5, 0.3, 0.2))
    if a["views"] != "two" and a["sky"] == "differ":
        a["sky"] = "same"      # (one view reads one mask)
    if refusal(settings(a), a["sky"] != "none") or not mixed_map_possible(a):
        return None
    # the working grid
    D, s = a["D"], a["s"]
    if a["shape"] == "tiny":
        H, W = int(rng.integers(3, 9)), int(rng.integers(5, 21))
    elif a["shape"] == "narrow":
        H, W = int(rng.integers(17, 41)), int(rng.integers(max(8, D // 4), D))
    elif a["shape"] == "wide":
        H, W = int(rng.integers(17, 49)), int(rng.integers(D + 1, D + 61))
    else:
        H, W = int(rng.integers(17, 41)), VSTRIP_COLS * int(rng.integers(2, 7)) + int(rng.integers(1, 5))
    # Room for a mixed map (inputs(): true disparities min_disp + s and min_disp + 2 s, the lowest rows
    # of the right image noise): columns the largest disparity can match in, and under
    # post_filter a surface above its speckle size of 1000 / s pixels below the noise rows
    first = a["min_disp"] // s + 3
    tiny = a["shape"] == "tiny"
    W = max(W, first + (4 if tiny else 12))
    if a["cost"] == "ct":   # (CT skips the taps left of the image: at j < d every cost is 0 and the WTA has no say)
        first = (D + a["min_disp"]) // s + 6
        W = max(W, first + 18)
    if a["shape"] == "narrow" and W >= D:
        return None
    band = max(1, H // 2) if tiny else max(6, int(H * (0.5 if a["kind"] == "noise" else 0.2)))
    if settings(a).post_filter:
        H = max(H, band + -(-int(3.2 * (1000 // s)) // (W - first)))
    if not census and H * W * D > VOLUME_ELEMS:
        H = VOLUME_ELEMS // (W * D)
        if settings(a).post_filter or H < band + 3:
            return None
    a["band"] = band
    a["h"], a["w"] = H * s + int(rng.integers(0, s)), W * s + int(rng.integers(0, s))
    return a


def mixed_map_possible(a):
    """Whether a frame of these settings can report a map with valid and invalid pixels at the
    sizes of this file.  post_filter's speckle removal empties a tiny frame (fewer pixels than
    one speckle); a tiny frame is narrower than min_disp = 16 lets anything match; and a
    one-view SGM map with uniqueness 1.0 rejects nothing (min / sec > 1 never holds), and the
    paths smooth what post_filter would remove (BM's WTA on the filtered cost does not); an LR threshold of 0 keeps only pixels whose two sub-pixel values are
    equal, too few for a surface post_filter keeps."""
    post = a["post"] != "off" or a["ctor"] != "SGM"
    if a["shape"] == "tiny" and (post or a["min_disp"] == 16):
        return False
    if a["views"] == "two" and a["lr_max_diff"] == 0.0 and (post or a["shape"] == "tiny"):
        return False
    return not (a["views"] != "two" and a["uniqueness"] == 1.0 and a["ctor"] == "SGM")


def settings(a):
    return Settings(solver="bm" if a["ctor"] == "BM" else "sgm", D=a["D"], s=a["s"], blur=a["blur"], views=a["views"],
                    paths=a["paths"], min_disp=a["min_disp"], cost=a["cost"], window=a["window"],
                    weighted=a["weighted"], volume_filter=a["volume_filter"], p1=a["p1"], p2=a["p2"],
                    uniqueness=a["uniqueness"], lr_max_diff=a["lr_max_diff"],
                    post_filter=a["post"] != "off" or a["ctor"] != "SGM", confidence=a["confidence"], fill=a["fill"],
                    reproject=Q if a["reproject"] else None)


def pairs_of(a):
    names = list(AXES)
    return {(n1, a[n1], n2, a[n2]) for i, n1 in enumerate(names) for n2 in names[i + 1:]}


@functools.lru_cache(maxsize=None)
def accepted_pairs():
    """Every pair of values of two axes that some accepted case holds: 6000 uniform draws over
    every stratum (a pair no draw of those produces is one the library refuses, or that a
    constructor cannot express: GPU_SGM and BM take few of the settings)."""
    rng = np.random.default_rng(0x5E77 - 1)
    out = set()
    for n in range(6000):
        a = draw(rng, ("sad", "ssd", "ct", "BM", "GPU_SGM", "right", "census", "census")[n % 8], uniform=True)
        if a is not None:
            out |= pairs_of(a)
    return frozenset(out)


def sgm_solver(a):
    return a["ctor"] != "BM"


def keeps(a, schedule):
    """Whether the forced schedule runs on the case's handle (the module's docstring)."""
    if not sgm_solver(a) or a["paths"] != 8:
        return False
    if schedule in ("onewave", "split"):
        return True
    if a["cost"] != "census":
        return False
    return schedule == "slant" or a["h"] // a["s"] > 16


SCHEDULES = {"onewave": ({"SGM_SWEEP_SPLIT": "0"}, "sweep_L8_acc"), "split": ({"SGM_SWEEP_SPLIT": "1"}, "sweep_L8_acc"),
             "bands16": ({"SGM_BAND_ROWS": "16"}, "stage_b_d2"), "slant": ({"SGM_SLANT": "1"}, "slant_up")}
PARTS = ("sad", "ssd", "ct", "BM", "GPU_SGM", "right", "census")


def draw_cases():
    """The list: N_DRAWN cases by stratum; then, while an accepted pair is missing, one more case
    from any stratum (every value equally likely: some pairs, a tiny census frame for one, have
    no weight in the strata's draws); then census cases until the forced schedules keep two
    thirds of the SGM-solver cases with two cases to spare."""
    cases, seen = [], set()

    def add(parts, uniform):
        k = len(cases)
        rng = np.random.default_rng(0x5E77 + k)
        best, gain = None, -1
        for part in parts:
            for _ in range(N_CANDIDATES // len(parts)):
                a = draw(rng, part, uniform)
                if a is not None and len(pairs_of(a) - seen) > gain:
                    best, gain = a, len(pairs_of(a) - seen)
        best["seed"] = k
        seen.update(pairs_of(best))
        cases.append(best)

    for k in range(N_DRAWN):
        add((stratum(k),), False)
    while accepted_pairs() - seen:
        assert len(cases) < 2 * N_DRAWN, sorted(accepted_pairs() - seen, key=str)
        add(PARTS, True)

    def short():
        solver = [a for a in cases if sgm_solver(a)]
        return any(3 * (sum(keeps(a, name) for a in solver) - 2) < 2 * len(solver) for name in SCHEDULES)

    while short():
        add(("census",) * 24, False)
    return cases


CASES = draw_cases()


def case_id(a):
    st = settings(a)
    bits_ = [a["ctor"], f"{a['h']}x{a['w']}", f"D{a['D']}", f"s{a['s']}", a["shape"], a["kind"], "sky-" + a["sky"],
             "V" + a["views"], f"p{a['paths']}", f"m{a['min_disp']}", a["cost"]]
    if a["window"]:
        bits_.append("win%dx%d" % a["window"])
    bits_ += [n for n in ("weighted", "confidence", "reproject") if a[n]]
    if not a["blur"]:
        bits_.append("noblur")
    if any(a["volume_filter"]):
        bits_.append("vf" + "".join(c for c, on in zip("hv", a["volume_filter"]) if on))
    bits_ += [f"P{st.p1}-{st.p2}", f"u{st.uniqueness}", f"lr{st.lr_max_diff}", "post-" + a["post"], "fill-" + a["fill"]]
    return f"{a['seed']:02d}_" + "_".join(bits_)


IDS = [case_id(a) for a in CASES]


# ----------------------------------------------------------------- inputs
def blob_mask(rng, H, W):
    """A few random rectangles of sky."""
    m = np.zeros((H, W), np.uint8)
    for _ in range(3):
        i, j = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[i:i + int(rng.integers(1, max(2, H // 5))), j:j + int(rng.integers(1, max(2, W // 5)))] = 255
    return m


def stereo_pair(a):
    """The case's pair: splitmix noise on the left; the right image the left one shifted by a
    step of disparities inside the search window, min_disp + s above and min_disp + 2 s below
    (whole working-grid columns; each level a surface of its own for post_filter), with
    its lowest a["band"] working-grid rows (below any sky mask) replaced by independent noise: pixels the uniqueness test and the
    LR check reject.  kind "noise": half of the rows; "road": a fifth (six at least)."""
    h, w, s = a["h"], a["w"], a["s"]
    seed = synthetic.SEED_BASE + 200 + a["seed"]
    left = synthetic.noise_image(h, w, seed)
    used = h // s if a["ctor"] == "BM" else h
    g = a["min_disp"] + s * (1 + (2 * np.arange(h) >= used - a["band"]))
    right = np.take_along_axis(left, np.minimum(np.arange(w)[None, :] + g[:, None], w - 1), axis=1)
    rows = a["band"] * (1 if a["ctor"] == "BM" else s)      # (BM decimates the columns only, BM.cpp:24-25)
    right[used - rows:] = synthetic.noise_image(h, w, seed ^ 0xA5A5A5A5A5)[used - rows:]
    return left, np.ascontiguousarray(right)


def inputs(a):
    """(left, right, sky_l, sky_r) of a case."""
    left, right = stereo_pair(a)
    H, W = a["h"] // a["s"], a["w"] // a["s"]
    if a["sky"] == "none":
        return left, right, None, None
    if a["sky"] == "same":
        m = synthetic.sky_mask(H, W)
        return left, right, m, m
    rng = np.random.default_rng(0xB10B + a["seed"])
    sky_l, sky_r = blob_mask(rng, H, W), blob_mask(rng, H, W)
    assert not np.array_equal(sky_l, sky_r)
    return left, right, sky_l, sky_r


@functools.lru_cache(maxsize=None)
def expected(k):
    """frame_recipe.frame of CASES[k], computed once per session; read-only."""
    a = CASES[k]
    out = frame_recipe.frame(*inputs(a)[:2], settings(a), *inputs(a)[2:])
    for m in out.values():
        m.setflags(write=False)
    return out


def compared_map(a, want):
    """The expected map get_disp() / get_lr_disp() is compared with."""
    return want["filled"] if a["fill"] != "off" else want["map"]


# ---------------------------------------------------------------- handles
def budget(a):
    rows, cols = a["h"] // a["s"], a["w"] // a["s"]
    return -(-cols // 64) * rows + 1 if a["post"] == "budget" else 0


def create_kwargs(a):
    """What only sgm_create takes."""
    if a["ctor"] == "BM":
        return dict(blur=a["blur"], uniqueness=a["uniqueness"])
    if a["ctor"] == "GPU_SGM":
        return {}
    return dict(blur=a["blur"], views=2 if a["views"] == "two" else 1, view="right" if a["views"] == "right" else "left",
                paths=a["paths"], p1=a["p1"], p2=a["p2"], uniqueness=a["uniqueness"], lr_max_diff=a["lr_max_diff"],
                post_filter=a["post"] != "off")


def setter_kwargs(a):
    """What the setters take, as constructor keywords."""
    kw = dict(post_filter_launches=budget(a), window=a["window"], weighted=a["weighted"], fill=a["fill"],
              reproject=Q if a["reproject"] else None)
    if a["ctor"] != "BM":
        kw["min_disp"] = a["min_disp"]
    if a["ctor"] == "SGM":
        kw.update(confidence=a["confidence"], cost=a["cost"],
                  volume_filter=a["volume_filter"] if any(a["volume_filter"]) else None)
    return kw


def make(a, **kw):
    ctor = {"SGM": SGM, "BM": BM, "GPU_SGM": GPU_SGM}[a["ctor"]]
    return ctor(a["h"], a["w"], a["s"], a["D"], **kw)


def assert_equal(got, want, what):
    g, w = bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(want))
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = int((g != w).sum())
    assert bad == 0, f"{what}: {bad}/{g.size} mismatches"


def frame_map(sgm, post_or_filled):
    """The map process() left: the final map of a post-filtered or filled frame, else the LR /
    sub-pixel map."""
    return sgm.get_disp() if post_or_filled else sgm.get_lr_disp()


def check_maps(sgm, a, want):
    """Every map the handle reports after a frame against frame_recipe.frame's."""
    sgm.check()
    own = 1 if a["views"] == "right" else 0
    assert_equal(sgm.get_raw_disp().astype(np.int64), want["disp"].astype(np.int64), "raw WTA")
    filled, post = a["fill"] != "off", settings(a).post_filter
    assert_equal(frame_map(sgm, filled or post), compared_map(a, want).astype(np.float32), "map")
    if a["confidence"]:
        assert_equal(sgm.get_confidence(own), want["ratio"], "confidence")
        if a["views"] == "two":
            assert_equal(sgm.get_confidence(1), want["ratio_beta"], "confidence of the right view")
    if filled:
        assert_equal(sgm.get_fill_mask(), want["fill_mask"], "fill mask")
    if a["reproject"]:
        assert_equal(sgm.get_xyz(), want["xyz"], "xyz")
        assert_equal(sgm.get_depth(), want["depth"], "depth")
    if not filled and not post and a["views"] != "right":
        assert_equal(sgm.get_disp(), want["final"], "get_disp")


def run_case(k, ran=None):
    a = CASES[k]
    left, right, sky_l, sky_r = inputs(a)
    with make(a, **create_kwargs(a), **setter_kwargs(a)) as sgm:
        sgm.set_profiling(True)
        sgm.process(left, right, sky_l, sky_r)
        profile = sgm.get_profile()
        check_maps(sgm, a, expected(k))
    if ran:
        assert ran in profile, (ran, sorted(profile))


# --------------------------------------------------------------- schedules
FORCED = [pytest.param(k, name, id=f"{name}-{IDS[k]}") for name in SCHEDULES for k, a in enumerate(CASES)
          if keeps(a, name)]


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_frame(k):
    """The library's own schedule."""
    run_case(k)


@pytest.mark.parametrize("k,schedule", FORCED)
def test_frame_forced_schedule(k, schedule, monkeypatch):
    env, ran = SCHEDULES[schedule]
    for name in ("SGM_SWEEP_SPLIT", "SGM_BAND_ROWS", "SGM_SLANT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    run_case(k, ran)


def test_the_strip_width_is_the_librarys():
    assert _capi.lib().sgm_vstrip_cols() == VSTRIP_COLS


# ------------------------------------------------------ setters after a frame
def set_min_disp(sgm, m):
    _capi.check(sgm._lib.sgm_set_min_disp(sgm._h, int(m)), sgm._h)
    sgm.min_disp, sgm.invalid_disp = int(m), sgm.max_disp + int(m) + 1


# setting -> (the Settings fields it changes, their "off" values); the order below is the canonical one
SETTERS = {
    "min_disp": dict(min_disp=0), "cost": dict(cost="census"), "window": dict(window=None),
    "weighted": dict(weighted=False), "volume_filter": dict(volume_filter=(False, False)),
    "confidence": dict(confidence=False), "fill": dict(fill="off"), "reproject": dict(reproject=None),
    "post_filter_launches": {},
}


def apply(sgm, a, name, on):
    if name == "min_disp":
        set_min_disp(sgm, a["min_disp"] if on else 0)
    elif name == "cost":
        sgm.set_cost(a["cost"] if on else "census")
    elif name == "window":
        sgm.set_window(*(a["window"] if on else (7, 9)))
    elif name == "weighted":
        sgm.set_weighted(on)
    elif name == "volume_filter":
        sgm.set_volume_filter(*(a["volume_filter"] if on else (False, False)))
    elif name == "confidence":
        sgm.set_confidence(on)
    elif name == "fill":
        sgm.set_fill(a["fill"] if on else "off")
    elif name == "reproject":
        sgm.set_reproject(Q if on else None)
    else:
        sgm.set_post_filter_launches(budget(a) if on else 0)


def kernels(sgm):
    """The kernel classes launched since the last get_profile() (a class stays listed at 0)."""
    return sorted(n for n, (launches, _, _) in sgm.get_profile().items() if launches)


def moved(a):
    """The setters the case's settings need, in SETTERS' order."""
    st = settings(a)
    out = [n for n, off in SETTERS.items() if any(getattr(st, f) != v for f, v in off.items())]
    return out + (["post_filter_launches"] if budget(a) else [])


def accepted_order(a, names, rng, on):
    """A seeded shuffle of `names` every intermediate state of which refusal() accepts, walking
    from the created handle's settings to the case's (on) or back (off)."""
    st, sky = settings(a), a["sky"] != "none"
    start = st if not on else st.replace(**{f: v for off in SETTERS.values() for f, v in off.items()})
    for _ in range(200):
        order = [names[i] for i in rng.permutation(len(names))]
        cur, ok = start, True
        for n in order:
            cur = cur.replace(**({f: getattr(st, f) for f in SETTERS[n]} if on else SETTERS[n]))
            if refusal(cur, False):     # (masks reach a frame only; no frame runs in between)
                ok = False
                break
        if ok:
            return order
    raise AssertionError("no order of the setters is accepted")


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_setters_after_a_frame(k):
    """A handle that has run a frame takes the case's settings through the setters in a seeded
    shuffled order, reports the case's maps, and after every setting is switched off again runs
    the first frame bit for bit, with a fresh handle's memory and the first frame's kernels."""
    a = CASES[k]
    left, right, sky_l, sky_r = inputs(a)
    names = moved(a)
    rng = np.random.default_rng(0x5E7 + k)
    # (a window cost takes no masks: the plain frames run without them when the case has a cost kind)
    plain_sky = (None, None) if a["cost"] != "census" else (sky_l, sky_r)
    with make(a, **create_kwargs(a)) as fresh:
        fresh_bytes = fresh.device_bytes
    with make(a, **create_kwargs(a)) as sgm:
        sgm.set_profiling(True)
        sgm.process(left, right, *plain_sky)
        post = settings(a).post_filter
        first = (sgm.get_raw_disp().copy(), frame_map(sgm, post).copy())
        first_kernels = kernels(sgm)
        for n in accepted_order(a, names, rng, True):
            apply(sgm, a, n, True)
        sgm.process(left, right, sky_l, sky_r)
        check_maps(sgm, a, expected(k))
        for n in accepted_order(a, names, rng, False):
            apply(sgm, a, n, False)
        sgm.get_profile()       # (the second frame's kernels and its getters': the count restarts)
        sgm.process(left, right, *plain_sky)
        assert_equal(sgm.get_raw_disp(), first[0], "third frame's raw WTA")
        assert_equal(frame_map(sgm, post), first[1], "third frame's map")
        assert kernels(sgm) == first_kernels
        assert sgm.device_bytes == fresh_bytes


# ---------------------------------------------------------------- refusals
def _sgm(**kw):
    return SGM(40, 80, kw.pop("s", 1), 32, **kw)


# rule of frame_recipe.refusal -> (handle, the refused call, what must be unchanged afterwards)
REFUSALS = {
    "weighted: odd effective window sides":   # (tests/test_gpu_weighted.py's own: the default window at scale 2)
        (lambda: _sgm(s=2), lambda g: g.set_weighted(True), lambda g: g.weighted is False),
    "window: 64 bits": (lambda: _sgm(s=2), lambda g: g.set_window(18, 18), lambda g: g.window == (7, 9)),
    "window: 1..9": (lambda: _sgm(s=2), lambda g: g.set_window(20, 18), lambda g: g.window == (7, 9)),
    "window: centre": (lambda: _sgm(s=2), lambda g: g.set_window(3, 3), lambda g: g.window == (7, 9)),
    "min_disp: >= 0, a multiple of the scale, D + m + 1 in 16 bits":
        (lambda: _sgm(s=2), lambda g: set_min_disp(g, 3), lambda g: _invalid(g) == 33),
    "bm: no min_disp": (lambda: BM(40, 80, 1, 32), lambda g: set_min_disp(g, 16), lambda g: _invalid(g) == 33),
    "bm: no cost kind": (lambda: BM(40, 80, 1, 32), lambda g: g.set_cost("sad"), lambda g: g.cost == "census"),
    "bm: no interpolate": (lambda: BM(40, 80, 1, 32), lambda g: g.set_fill("interpolate"), lambda g: g.fill == "off"),
    "bm: no confidence": (lambda: BM(40, 80, 1, 32), lambda g: g.set_confidence(True), lambda g: _no_ratio(g)),
    "bm: no volume filter": (lambda: BM(40, 80, 1, 32), lambda g: g.set_volume_filter(True, True),
                             lambda g: g.volume_filter == (False, False)),
    "interpolate: two views": (lambda: _sgm(views=1), lambda g: g.set_fill("interpolate"), lambda g: g.fill == "off"),
    "right view: no cost kind, volume filter, fill or reprojection":
        (lambda: _sgm(views=1, view="right"), lambda g: g.set_cost("ssd"), lambda g: g.cost == "census"),
    "sky_detect: no cost kind": (lambda: _sgm(sky_detect=True), lambda g: g.set_cost("sad"), lambda g: g.cost == "census"),
    "sky masks: no cost kind":
        (lambda: _sgm(cost="sad"),
         lambda g: g.process(*synthetic.stereo_pair(40, 80, 32), synthetic.sky_mask(40, 80), synthetic.sky_mask(40, 80)),
         lambda g: g.cost == "sad"),
}


def _invalid(g):
    import ctypes
    inv = ctypes.c_int()
    _capi.check(g._lib.sgm_get_invalid_disp(g._h, ctypes.byref(inv)), g._h)
    return inv.value


def _no_ratio(g):
    with pytest.raises(SGMError):
        g.get_confidence(0)
    return True


@pytest.mark.parametrize("rule", list(REFUSALS))
def test_refusals(rule):
    handle, call, unchanged = REFUSALS[rule]
    with handle() as g:
        with pytest.raises(SGMError) as e:
            call(g)
        assert e.value.code == _capi.SGM_ERR_INVALID_ARG
        assert g._lib.sgm_last_error(g._h)      # non-empty
        assert unchanged(g)


# one example per "create: ..." rule of frame_recipe.refusal
CREATE_REFUSALS = {"right_post_filter": dict(views=1, view="right", post_filter=True), "negative_p1": dict(p1=-1),
                   "uniqueness_0": dict(uniqueness=0.0), "scale_3": dict(s=3)}


@pytest.mark.parametrize("kw", list(CREATE_REFUSALS.values()), ids=list(CREATE_REFUSALS))
def test_create_refusals(kw):
    """The rules sgm_create holds (no handle, so no sgm_last_error to read)."""
    with pytest.raises(SGMError) as e:
        _sgm(**kw)
    assert e.value.code == _capi.SGM_ERR_INVALID_ARG
