"""The handle's plan (stereo_matching_amd/csrc/sgm_plan.h) on the CPU: which
schedule sgm_create picks by frame size, views, paths and switches, and which
parameters it refuses.  Every schedule gives bit-identical maps, so nothing else
notices a slip in these rules; the GPU suite pins each schedule's launches only
where a switch forces it (the launch ledgers).  tests/cpp/plan_main.cpp prints
the plans, built under ASan and UBSan and run directly."""
from __future__ import annotations

import os

import pytest

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256  # the MI355X

# (h, w, s, D, views, paths, switches) -> the plan's fields that the row pins.
# At 256 CUs; derived by hand from the rules (the 256 MB Infinity Cache test, 0.5 / 0.9 tiles of 14
# columns per workgroup for the slanted schedule at D = 256 / 128, 192 MB bands on 16-row edges,
# views * H < 4 * CUs for the 4-path H pair's split form).
K, K2, HD, UHD = (375, 1242), (750, 2484), (1080, 1920), (2160, 3840)
TABLE = [
    ((*K, 1, 64, 2, 8, {}), dict(sched="JOINT", band_rows=0, sub_cm=1)),
    ((*K, 1, 64, 1, 8, {}), dict(sched="PER_VIEW", sub_cm=0)),
    ((*K, 1, 128, 1, 8, {}), dict(sched="PER_VIEW")),
    ((*K, 1, 128, 2, 8, {}), dict(sched="PER_VIEW")),
    ((512, 1024, 1, 128, 1, 8, {}), dict(sched="PER_VIEW", band_rows=0)),  # exactly 256 MB
    ((512, 1024, 1, 128, 2, 8, {}), dict(sched="PER_VIEW", band_rows=0)),
    ((513, 1024, 1, 128, 1, 8, {}), dict(sched="BANDS", band_rows=384)),
    ((513, 1024, 1, 128, 2, 8, {}), dict(sched="BANDS", band_rows=384)),
    ((512, 1056, 1, 128, 2, 8, {}), dict(sched="BANDS", band_rows=368)),
    ((512, 1056, 1, 128, 2, 8, {"SGM_BAND_ROWS": "0"}), dict(sched="WHOLE_FINAL2", band_rows=0)),
    ((512, 1056, 1, 128, 1, 8, {"SGM_BAND_ROWS": "0"}), dict(sched="PER_VIEW")),
    ((720, 1280, 1, 128, 2, 8, {}), dict(sched="BANDS", band_rows=304)),
    ((720, 1280, 1, 256, 2, 8, {}), dict(sched="SLANT")),
    ((720, 1280, 1, 256, 1, 8, {}), dict(sched="BANDS", band_rows=144)),
    ((*HD, 1, 128, 1, 8, {}), dict(sched="BANDS", band_rows=192)),
    ((*HD, 1, 128, 2, 8, {}), dict(sched="SLANT")),
    ((*HD, 1, 256, 1, 8, {}), dict(sched="SLANT", vstrip=1)),
    ((*HD, 1, 256, 2, 8, {}), dict(sched="SLANT", vstrip=1)),
    ((*HD, 1, 256, 1, 8, {"SGM_SLANT": "0"}), dict(sched="BANDS", band_rows=96)),
    ((*HD, 1, 256, 2, 8, {"SGM_VSTRIP": "0"}), dict(sched="SLANT", vstrip=0)),
    ((*UHD, 1, 64, 2, 8, {}), dict(sched="BANDS", band_rows=192)),
    ((*UHD, 1, 256, 2, 8, {}), dict(sched="SLANT")),
    ((120, 330, 1, 64, 2, 8, {"SGM_SLANT": "1"}), dict(sched="SLANT", slant_forced=1)),
    ((120, 330, 1, 64, 2, 8, {"SGM_BAND_ROWS": "20"}), dict(sched="BANDS", band_rows=16)),
    ((*K, 1, 128, 2, 4, {}), dict(sched="PATHS4", p4_split=1, slant=0, band_rows=0)),
    ((*K, 1, 128, 2, 4, {"SGM_P4_HPAIR": "0"}), dict(sched="PATHS4", p4_split=0)),
    ((*HD, 1, 256, 2, 4, {}), dict(sched="PATHS4", p4_split=0)),
    # any frame with paths 4 under SGM_SLANT=1
    ((*K, 1, 128, 2, 4, {"SGM_SLANT": "1"}), dict(sched="PATHS4", slant=0, slant_forced=0)),
    ((*HD, 1, 256, 1, 4, {"SGM_SLANT": "1"}), dict(sched="PATHS4", slant=0, slant_forced=0)),
    ((120, 330, 1, 64, 2, 4, {"SGM_SLANT": "1"}), dict(sched="PATHS4", slant=0, slant_forced=0)),
]
# 750x2484 at scale 2 plans as 375x1242 (every field but the scale itself)
SCALED = [((*K2, 2, 128, v, 8, {}), (*K, 1, 128, v, 8, {})) for v in (1, 2)]

# (sgm_default_params(375, 1242, 1, 64) with these fields) -> sgm_create's message, from valid_params
REFUSALS = [
    ((375, 1242, 3, 64), {}, "scale must be 1 or 2 (Solver.cpp:8)"),
    ((375, 1242, 1, 100), {}, "max_disp must be 32, 64, 128 or 256 (Solver.cpp:10, widened)"),
    ((375, 1242, 1, 64), {"views": 3}, "views must be 1 or 2"),
    ((375, 1242, 1, 64), {"paths": 6}, "paths must be 8 (or 0) or 4 (USE_8_PATH, inc/SGM.h:7)"),
    ((375, 1242, 1, 64), {"uniqueness": 0},
     "uniqueness must be > 8*(p2 + 999999)/FLT_MAX (SGM.cpp:392-408 would read the previous pixel's sec_min_d)"),
    ((375, 1242, 1, 64), {"view": 1, "views": 2},
     "SGM_VIEW_RIGHT needs views == 1, the SGM solver and no post_filter/lk_refine"),
    ((375, 4, 1, 64), {}, "working size 375x4 below the 5x3 cost window"),
    ((375, 9, 2, 64), {}, "working size 187x4 below the 5x3 cost window"),
    ((375, 1242, 1, 64), {"p1": -1}, "p1 and p2 must be >= 0"),
]


def plan_arg(row):
    *nums, env = row
    return "plan:" + ",".join([*map(str, nums[:6]), str(CUS), *(f"{k}={v}" for k, v in env.items())])


def parse(half):
    out = {}
    for kv in half.split():
        k, v = kv.split("=")
        out[k] = v if k == "sched" else int(v)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.host_program(tmp_path_factory.mktemp("plan"), os.path.join(ROOT, "tests", "cpp", "plan_main.cpp"))


@pytest.fixture(scope="module")
def plans(exe):
    """row -> (the plan, the plan again without the slanted schedule), for every row of the tables."""
    rows = [r for r, _ in TABLE] + [r for pair in SCALED for r in pair]
    r = support.run(exe, *map(plan_arg, rows))
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == len(rows), r.stdout + r.stderr
    return {plan_arg(row): tuple(map(parse, line.split(" | without_slant: "))) for row, line in zip(rows, lines)}


@pytest.mark.parametrize("row,want", TABLE, ids=[plan_arg(r)[5:] for r, _ in TABLE])
def test_plan_by_size_views_paths_and_switches(plans, row, want):
    got, _ = plans[plan_arg(row)]
    print(got)
    assert {k: got[k] for k in want} == want
    h, w, s, D, views, paths, _env = row
    assert (got["H"], got["W"], got["D"], got["scale"], got["nviews"]) == (h // s, w // s, D, s, views)
    assert got["paths4"] == (paths == 4)


def test_every_plan_is_consistent(plans):
    for arg, both in plans.items():
        for p in both:
            assert not p["slant"] or p["sched"] == "SLANT", arg
            assert (p["sched"] == "SLANT") == bool(p["slant"]), arg
            assert not p["paths4"] or (not p["slant"] and p["band_rows"] == 0 and p["sched"] == "PATHS4"), arg
            assert p["sub_cm"] == (p["nviews"] == 2 and not p["slant"]), arg
            assert p["band_rows"] % 16 == 0 and 0 <= p["band_rows"] < p["H"], arg
            assert not p["slant_forced"] or p["slant"], arg
            assert (p["sched"] == "BANDS") == (p["band_rows"] > 0 and not p["slant"]), arg


def test_scale_two_plans_as_the_working_grid(plans):
    for scaled, plain in SCALED:
        a, b = plans[plan_arg(scaled)][0], plans[plan_arg(plain)][0]
        assert a["scale"] == 2 and b["scale"] == 1
        assert {k: v for k, v in a.items() if k != "scale"} == {k: v for k, v in b.items() if k != "scale"}


def test_replanning_without_slant_is_the_plan_of_slant_off(exe, plans):
    # the memory fallback of sgm_create: what SGM_SLANT=0 gives, whichever way the schedule was chosen
    slanted = [(r, plans[plan_arg(r)]) for r, _ in TABLE if plans[plan_arg(r)][0]["slant"]]
    assert len(slanted) == 7  # six chosen by size, one forced
    off_rows = [(*r[:6], {**r[6], "SGM_SLANT": "0"}) for r, _ in slanted]
    out = support.run(exe, *map(plan_arg, off_rows))
    assert out.returncode == 0, out.stderr
    for (row, (_, without)), line in zip(slanted, out.stdout.splitlines()):
        off = parse(line.split(" | ")[0])
        assert without == off, row
        assert not without["slant"] and not without["slant_forced"] and without["sched"] != "SLANT"
    hd = (*HD, 1, 256, 1, 8, {})
    without = plans[plan_arg(hd)][1]
    assert (without["sched"], without["band_rows"], without["sub_cm"]) == ("BANDS", 96, 0)
    # a plan that never had the schedule is unchanged by it
    for arg, (plan, without) in plans.items():
        if not plan["slant"]:
            assert plan == without, arg


@pytest.mark.parametrize("size,fields,message", REFUSALS, ids=[m[:24] for _, _, m in REFUSALS])
def test_refusals_keep_their_messages(exe, size, fields, message):
    arg = "params:" + ",".join([*map(str, size), *(f"{k}={v}" for k, v in fields.items())])
    r = support.run(exe, arg)
    assert r.returncode == 0 and r.stdout == f"refused: {message}\n", r.stdout + r.stderr


def test_default_params_pass(exe):
    r = support.run(exe, "params:375,1242,1,64", "params:750,2484,2,256", "params:3,5,1,32", "params:375,1242,1,64,paths=0")
    assert r.returncode == 0 and r.stdout == "ok\n" * 4, r.stdout + r.stderr


def test_makefile_lists_the_plan_headers():
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    rules = [line for line in mk.splitlines() if line.startswith(("%.o:", "%.dbg.o:"))]
    assert len(rules) == 2 and all("sgm_plan.h" in r and "sgm_geom.h" in r for r in rules)
