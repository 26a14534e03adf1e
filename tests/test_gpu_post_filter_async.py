"""The median fill with a launch budget (sgm_set_post_filter_launches): a post
filter that enqueues a fixed number of fill launches and returns, with the
device judging whether the last launch proved the fixed point.

Budgets here are the derived bound ceil(W / 64) * H + 1 (DESIGN.md "Post
filter": every launch finalises at least the first not-yet-final row segment
in raster order, and one more launch changes nothing), so no case depends on
how the tiles of a launch happen to interleave.  The deterministic verdict
cases use budget 1: launch 0 runs every tile, so it changes a tile exactly when
the map has a fillable pixel."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import postfilter_maps
from support import f32_bits as bits
from stereo_matching_amd import BM, SGM, SGMError, _capi, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bound(H, W):
    return -(-W // 64) * H + 1


# ------------------------------------------------------------ bit-exactness

# (H, W, SGM_MF_ROWS or "", pitched): every postfilter_maps kind, two seeds each
SHAPES = [(17, 65, "", False), (33, 129, "", False), (48, 96, "", True), (61, 203, "", False),
          (33, 129, "8", False), (33, 129, "16", False)]
D_MAPS = 32

# One child process for all maps (torch's HIP runtime initialises before the
# library's, as in test_gpu_post_filter.py's PITCHED): each map goes through
# post_filter_device in place on a torch device buffer, then check().
CHILD = r"""
import json, os, sys, numpy as np, torch
root, shapes, D = sys.argv[1], json.loads(sys.argv[2]), int(sys.argv[3])
sys.path[:0] = [root, os.path.join(root, "tests")]
dev = torch.device("cuda", 0)
torch.cuda.init()
import oracle, postfilter_maps
from stereo_matching_amd import SGM
out = {}
for H, W, rows, pitched in shapes:
    os.environ.pop("SGM_MF_ROWS", None)
    if rows:
        os.environ["SGM_MF_ROWS"] = rows       # read when the handle is created
    budget = -(-W // 64) * H + 1
    pitch = W + 37 if pitched else W
    bad = []
    with SGM(H, W, 1, D, device=0, post_filter_launches=budget) as sgm:
        for kind in postfilter_maps.KINDS:
            for seed in range(2):
                F = postfilter_maps.make(kind, H, W, D, seed)
                buf = torch.full((H, pitch), -7.0, dtype=torch.float32, device=dev)
                buf[:, :W] = torch.from_numpy(F).to(dev)
                torch.cuda.synchronize(dev)
                sgm.post_filter_device(buf.data_ptr(), pitch=pitch)
                sgm.check()                     # waits; raises if the fill was not proven
                got = buf.cpu().numpy()
                want = oracle.post_filter(F, D, 1)
                n = int(np.count_nonzero(got[:, :W].view(np.uint32) != want.view(np.uint32)))
                if n or not (got[:, W:] == -7.0).all() or sgm.post_filter_proved_at() < 1:
                    bad.append([kind, seed, n, sgm.post_filter_proved_at()])
    out["%dx%d/%s" % (H, W, rows)] = {"budget": budget, "bad": bad,
                                     "maps": 2 * len(postfilter_maps.KINDS)}
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def child_results():
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES), str(D_MAPS)],
                       capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1][7:])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-rows%s%s" % (h, w, r or "auto", "-pitched" if p else "")
                                               for h, w, r, p in SHAPES])
def test_budgeted_fill_is_bit_exact(child_results, shape):
    H, W, rows, _ = shape
    res = child_results["%dx%d/%s" % (H, W, rows)]
    assert res["budget"] == bound(H, W) <= (256 if (H, W) == (61, 203) else 128)
    assert res["maps"] == 24
    assert res["bad"] == [], res["bad"]          # [kind, seed, mismatching pixels, proved_at]


# ------------------------------------------------------- verdict, deterministic

H1, W1, D1 = 48, 200, 64


def one_hole_map():
    F = postfilter_maps.make("all_valid", H1, W1, D1, 1)
    F[20, 100] = D1 + 1            # interior, 24 valid neighbours: launch 0 fills it
    return F


def run_device(sgm, F):
    """post_filter_device in place on a torch buffer; returns the buffer (not synchronised)."""
    buf = torch.from_numpy(F).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    sgm.post_filter_device(buf.data_ptr())
    return buf


def test_unproven_fill_is_reported_once():
    F = one_hole_map()
    with SGM(H1, W1, 1, D1, device=0, post_filter_launches=1) as sgm:
        buf = run_device(sgm, F)               # returns OK: nothing was read back
        with pytest.raises(SGMError, match="median fill") as e:
            sgm.check()
        assert e.value.code == _capi.SGM_ERR_HIP and "1 launches" in str(e.value)
        assert sgm.post_filter_proved_at() == 0
        sgm.check()                            # reported once, then cleared
        # a map with nothing to fill: launch 0 changes nothing and proves it
        G = postfilter_maps.make("all_valid", H1, W1, D1, 2)
        buf = run_device(sgm, G)
        sgm.check()
        assert sgm.post_filter_proved_at() == 1
        assert np.array_equal(bits(buf.cpu().numpy()), bits(oracle.post_filter(G, D1, 1)))
        # the one-hole map again, with room for the proof
        sgm.set_post_filter_launches(8)
        buf = run_device(sgm, F)
        sgm.check()
        assert 2 <= sgm.post_filter_proved_at() <= 8
        assert np.array_equal(bits(buf.cpu().numpy()), bits(oracle.post_filter(F, D1, 1)))


def test_unproven_fill_surfaces_from_the_next_frame():
    F = one_hole_map()
    dev = torch.device("cuda", 0)
    left, right = synthetic.stereo_pair(H1, W1, D1, pair_index=1)
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    out = torch.empty((H1, W1), dtype=torch.float32, device=dev)
    with SGM(H1, W1, 1, D1, device=0, post_filter_launches=1) as sgm:
        run_device(sgm, F)
        torch.cuda.synchronize(dev)            # the verdict is in: no check() in between
        with pytest.raises(SGMError, match="median fill"):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr())
        sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr())   # cleared
        sgm.check()
        want = oracle.process(left, right, D1)["lr"]
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_synchronous_stage_reports_its_own_unproven_fill():
    # sgm_stage_post_filter copies the map back and synchronises: an unproven
    # fill is that call's error, never a map returned as valid
    F = one_hole_map()
    with SGM(H1, W1, 1, D1, device=0, post_filter_launches=1) as sgm:
        with pytest.raises(SGMError, match="median fill"):
            sgm.post_filter(F)
        sgm.check()                            # reported by the call itself, then cleared
        sgm.set_post_filter_launches(bound(H1, W1))
        assert np.array_equal(bits(sgm.post_filter(F)), bits(oracle.post_filter(F, D1, 1)))


def test_get_disp_on_a_budgeted_handle_without_post_filter_param():
    # post_filter=False: process() keeps the LR map and get_disp() filters it
    # through the synchronous stage; an LR map always has fillable pixels, so
    # launch 0 changes a tile and budget 1 cannot prove the fill
    left, right = synthetic.stereo_pair(H1, W1, D1, pair_index=1)
    ref = oracle.process(left, right, D1)
    with SGM(H1, W1, 1, D1, device=0, post_filter=False, post_filter_launches=1) as sgm:
        sgm.process(left, right)
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(ref["lr"]))
        with pytest.raises(SGMError, match="median fill"):
            sgm.get_disp()
        sgm.check()
        sgm.set_post_filter_launches(bound(H1, W1))
        assert np.array_equal(bits(sgm.get_disp()), bits(ref["final"]))


def test_report_names_the_budget_that_was_not_enough():
    # the verdict carries its budget: a later filter or a changed budget does
    # not alter the message
    F = one_hole_map()
    with SGM(H1, W1, 1, D1, device=0, post_filter_launches=1) as sgm:
        run_device(sgm, F)
        torch.cuda.synchronize()
        sgm.set_post_filter_launches(0)
        buf = run_device(sgm, F)               # adaptive: 3 launches, proven
        with pytest.raises(SGMError, match="median fill not proven in 1 launches"):
            sgm.check()
        sgm.check()
        assert np.array_equal(bits(buf.cpu().numpy()), bits(oracle.post_filter(F, D1, 1)))


def test_profiling_with_a_budget_takes_one_event_pair_per_filter():
    F = postfilter_maps.make("diag", H1, W1, D1, 3)
    B = bound(H1, W1)
    with SGM(H1, W1, 1, D1, device=0, post_filter_launches=B) as sgm:
        sgm.set_profiling(True)
        for _ in range(2):
            buf = run_device(sgm, F)
            sgm.check()
        prof = sgm.get_profile()
        assert prof["post_median"][0] == 2 and prof["post_prep"][0] == 2
        assert prof["post_cc_apply"][0] == 2 and prof["post_median"][1] > 0.0
        assert np.array_equal(bits(buf.cpu().numpy()), bits(oracle.post_filter(F, D1, 1)))


def test_adaptive_fill_reports_where_it_was_proven():
    # proved_at after the adaptive path: the one-hole map settles in launch 0
    # (index 1 changes nothing), a map with nothing to fill is proven by launch 0
    with SGM(H1, W1, 1, D1, device=0) as sgm:
        assert sgm.post_filter_proved_at() == 0     # no post filter yet
        sgm.post_filter(one_hole_map())
        assert 2 <= sgm.post_filter_proved_at() <= 3
        sgm.post_filter(postfilter_maps.make("all_valid", H1, W1, D1, 2))
        assert sgm.post_filter_proved_at() == 1


# ---------------------------------------------------------------- arguments

def test_budget_arguments_and_back_to_adaptive():
    h, w, D = 96, 320, 64
    dev = torch.device("cuda", 0)
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    with SGM(h, w, 1, D, views=2, post_filter=True) as sgm:
        for n in (-1, 4097):
            with pytest.raises(SGMError) as e:
                sgm.set_post_filter_launches(n)
            assert e.value.code == _capi.SGM_ERR_INVALID_ARG
        with pytest.raises(SGMError):
            SGM(h, w, 1, D, post_filter_launches=4097)
        sgm.set_post_filter_launches(4096)
        sgm.set_post_filter_launches(bound(h, w))
        sgm.set_post_filter_launches(0)        # adaptive again: the capture is refused again
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
        d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        out = torch.empty((h, w), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)

        def frame():
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(),
                               stream=stream.cuda_stream)

        graph = torch.cuda.CUDAGraph()
        with pytest.raises(SGMError, match="HIP graph"):
            with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
                frame()
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            frame()
        sgm.check()
        want = oracle.process(left, right, D)["final"]
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))


# ----------------------------------------------------------- whole pipeline

HP, WP, DP = 96, 260, 64


@pytest.fixture(scope="module")
def pipeline_refs():
    refs = {}
    for kind in ("noise", "road"):
        left, right = synthetic.stereo_pair(HP, WP, DP, pair_index=2, kind=kind)
        refs[kind] = (left, right, oracle.process(left, right, DP)["final"])
    return refs


@pytest.mark.parametrize("kind", ["noise", "road"])
def test_pipeline_with_budget(pipeline_refs, kind):
    left, right, final = pipeline_refs[kind]
    B = bound(HP, WP)
    with SGM(HP, WP, 1, DP, post_filter=True, post_filter_launches=B) as sgm:
        sgm.process(left, right)
        assert np.array_equal(bits(sgm.get_disp()), bits(final))
        assert 1 <= sgm.post_filter_proved_at() <= B
    with SGM(HP, WP, 1, DP, post_filter=True, lk_refine=True, post_filter_launches=B) as sgm:
        sgm.process(left, right)
        want = oracle.lk_refine(left, right, final, DP)
        assert np.array_equal(bits(sgm.get_disp()), bits(want))


@pytest.mark.parametrize("kind", ["noise", "road", "road+band"])
def test_pipeline_with_budget_and_sky_detect(pipeline_refs, kind):
    left, right, _ = pipeline_refs[kind.split("+")[0]]
    if kind.endswith("band"):   # a bright, smooth band so the detector has something to find
        yy, xx = np.mgrid[0:HP, 0:WP]
        band = yy < (20 + 8 * np.sin(xx / 40.0)).astype(int)
        left = np.where(band, 200 + (yy // 9) % 2, left).astype(np.uint8)
        right = np.where(band, 200 + (yy // 9) % 2, right).astype(np.uint8)
    ml, mr = oracle.sky_detect(left), oracle.sky_detect(right)
    if kind.endswith("band"):
        assert (ml == 255).any()
    final = oracle.process(left, right, DP, sky_l=ml, sky_r=mr)["final"]
    want = oracle.lk_refine(left, right, final, DP)
    with SGM(HP, WP, 1, DP, post_filter=True, lk_refine=True, sky_detect=True,
             post_filter_launches=bound(HP, WP)) as sgm:
        sgm.process(left, right)
        assert np.array_equal(bits(sgm.get_disp()), bits(want))


def test_bm_with_budget(pipeline_refs):
    left, right, _ = pipeline_refs["road"]
    want = oracle.post_filter(oracle.bm_process(left, right, DP, 1).astype(np.float32), DP, 1)
    with BM(HP, WP, 1, DP, device=0, post_filter_launches=bound(HP, WP)) as bm:
        bm.process(left, right)
        assert np.array_equal(bits(bm.get_disp()), bits(want))
