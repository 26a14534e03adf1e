"""The matching window as a handle setting on the GPU (sgm_set_window, DESIGN.md
5p), bit for bit over every pixel and every disparity: the census launch and
the SAD / SSD producer against fixtures written by the reference's own compiled
CT_pts, SAD and SSD, whole frames against tests/window_recipe.py, and the
setter's behaviour."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle
import window_cases as cases
import window_recipe as wr
from stereo_matching_amd import BM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def census_id(c):
    shape, s, win = c
    return f"{shape[0]}x{shape[1]}_s{s}_{cases.wid(win)}"


# ------------------------------------------------------------------ census

@pytest.mark.parametrize("case", cases.census_cases(), ids=census_id)
def test_census_equals_the_reference(case):
    shape, s, win = case
    left, right = cases.census_pair(shape, s)
    h, w = left.shape
    with SGM(h, w, s, 32, views=1, blur=False, window=win) as sgm:
        assert sgm.window == win
        for img, want in zip((left, right), cases.ref_census(shape, s, win)):
            assert np.array_equal(sgm.stage_census(img), want)
    if win == (7, 9):  # the default: what the oracle's census gives
        assert np.array_equal(cases.ref_census(shape, s, win)[0], oracle.census(cases.working(left, s), s))


@pytest.mark.parametrize("case", cases.census_cases(), ids=census_id)
def test_blurred_census_equals_the_recipe(case):
    shape, s, win = case
    left, _ = cases.census_pair(shape, s)
    h, w = left.shape
    with SGM(h, w, s, 32, views=1, blur=True, window=win) as sgm:
        assert np.array_equal(sgm.stage_census(left), wr.frame_census(left, win, s, blur=True))


# ------------------------------------------------------------ window costs

COST_CASES = [(name, s, win, D, m) for name, s, win in cases.cost_fixture_cases()
              for D in cases.COST_D for m in cases.COST_MIN_DISP]


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", COST_CASES, ids=lambda c: f"{c[0]}_s{c[1]}_{cases.wid(c[2])}_D{c[3]}_m{c[4]}")
def test_window_cost_equals_the_reference(case, kind):
    name, s, win, D, m = case
    left, right = cases.cost_pair(name, s)
    h, w = left.shape
    with SGM(h, w, s, D, aux_only=True, min_disp=m, window=win) as sgm:
        got = sgm.stage_window_cost(left, right, kind)
    want = cases.ref_cost(name, s, win, kind)[:, :, m:m + D]
    assert np.array_equal(wr.bits(got), wr.bits(np.ascontiguousarray(want)))


def test_the_largest_numerator_through_the_general_divisions():
    left, right = cases.cost_pair("10x20", 1)
    with SGM(10, 20, 1, 32, aux_only=True, window=(9, 7)) as sgm:  # 63 taps of 255^2, / 9 / 7
        assert (sgm.stage_window_cost(left, right, "ssd") == np.float32(65025)).all()


def test_window_cost_on_device_tensors():
    name, s, win, D = "20x70", 1, (5, 5), 64
    left, right = cases.cost_pair(name, s)
    with SGM(20, 70, 1, D, aux_only=True, window=win) as sgm:
        got = sgm.window_cost(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), "sad")
        torch.cuda.synchronize(DEV)
    assert np.array_equal(wr.bits(got.cpu().numpy()), wr.bits(np.ascontiguousarray(cases.ref_cost(name, s, win, "sad")[:, :, :D])))


# ------------------------------------------------------------------ frames

H, W, D = 48, 96, 32


def pair(h=H, w=W, d=D, index=2):
    return synthetic.stereo_pair(h, w, d, pair_index=index, kind="road")


@functools.lru_cache(maxsize=None)
def expected(window, views=2, paths=8, sky=False, m=0, cost="census", solver="sgm", shape=(H, W, D), index=2):
    h, w, d = shape
    left, right = pair(h, w, d, index)
    mask = synthetic.sky_mask(h, w) if sky else None
    out = wr.recipe(left, right, d, window, 1, mask, paths, m, True, views, cost, solver)
    for a in out.values():
        a.setflags(write=False)
    return out


def check_frame(sgm, want, views, post_filter=False):
    """The handle's maps after process(): the raw WTA map, the sub-pixel map (after the LR check
    with two views) and the post-filtered one."""
    wr.assert_bits_equal(sgm.get_raw_disp(), want["disp"], "disp")
    if not post_filter:
        wr.assert_bits_equal(sgm.get_lr_disp(), want["lr"] if views == 2 else want["sub"], "sub")
    wr.assert_bits_equal(sgm.get_disp(), want["final"], "final")


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("window", [(5, 5), (9, 7)], ids=cases.wid)
def test_frame_equals_the_recipe(window, views, paths):
    left, right = pair()
    with SGM(H, W, 1, D, views=views, paths=paths, window=window) as sgm:
        sgm.process(left, right)
        check_frame(sgm, expected(window, views, paths), views)


def test_frame_with_sky_masks():
    left, right = pair()
    mask = synthetic.sky_mask(H, W)
    with SGM(H, W, 1, D, window=(5, 5)) as sgm:
        sgm.process(left, right, mask, mask)
        check_frame(sgm, expected((5, 5), sky=True), 2)


def test_frame_with_min_disp():
    left, right = pair()
    with SGM(H, W, 1, D, min_disp=16, window=(9, 7)) as sgm:
        sgm.process(left, right)
        check_frame(sgm, expected((9, 7), m=16), 2)


def test_frame_with_post_filter():
    left, right = pair()
    with SGM(H, W, 1, D, post_filter=True, window=(5, 5)) as sgm:
        sgm.process(left, right)
        check_frame(sgm, expected((5, 5)), 2, post_filter=True)


def test_bm_frame():
    left, right = pair()
    want = expected((5, 5), solver="bm")
    with BM(H, W, 1, D, window=(5, 5)) as bm:
        bm.process(left, right)
        wr.assert_bits_equal(bm.get_raw_disp(), want["disp"], "disp")
        wr.assert_bits_equal(bm.get_disp(), want["final"], "final")


def test_slanted_frame(monkeypatch):
    # (33 x 33, D = 64: the smallest frame the slanted schedule's own tests run)
    monkeypatch.setenv("SGM_SLANT", "1")
    shape = (33, 33, 64)
    left, right = pair(*shape, index=3)
    with SGM(33, 33, 1, 64, window=(5, 5)) as sgm:
        sgm.process(left, right)
        sgm.check()
        check_frame(sgm, expected((5, 5), shape=shape, index=3), 2)


def test_sad_frame():
    left, right = pair()
    want = expected((5, 5), cost="sad")
    with SGM(H, W, 1, D, cost="sad", window=(5, 5)) as sgm:
        sgm.process(left, right)
        wr.assert_bits_equal(sgm.get_raw_disp(), want["disp"], "disp")
        wr.assert_bits_equal(sgm.get_lr_disp(), want["lr"], "lr")
        wr.assert_bits_equal(sgm.get_disp(), want["final"], "final")


# ------------------------------------------------------------------ setter

def test_refusals_change_nothing():
    L = _capi.lib()
    with SGM(H, W, 1, D, window=(5, 7)) as sgm, SGM(H, W, 2, D, aux_only=True) as half:
        for bad in ((9, 9), (8, 8), (1, 1), (0, 9), (7, 0), (-7, 9), (10, 9), (7, 11), (20, 20)):
            with pytest.raises(SGMError, match="sgm_set_window") as ei:
                sgm.set_window(*bad)
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
            assert sgm.window == (5, 7)
        assert half.window == (7, 9)
        for bad in ((1, 9), (3, 3), (18, 18), (20, 9), (7, 21)):  # e = 0 x 4, 1 x 1, 9 x 9, 10 x 4, 3 x 10
            assert L.sgm_set_window(half._h, *bad) == _capi.SGM_ERR_INVALID_ARG
            assert b"sgm_set_window" in L.sgm_last_error(half._h)
            assert half.window == (7, 9)
        half.set_window(19, 15)  # 9 x 7
        assert half.window == (19, 15)
    with pytest.raises(SGMError, match="sgm_set_window"):
        SGM(H, W, 1, D, window=(9, 9))


def test_the_default_set_explicitly_is_an_untouched_handle():
    left, right = pair()
    with SGM(H, W, 1, D) as fresh, SGM(H, W, 1, D, window=(7, 9)) as sgm:
        assert fresh.window == sgm.window == (7, 9)
        fresh.process(left, right)
        sgm.process(left, right)
        for get in ("get_raw_disp", "get_lr_disp", "get_disp"):
            wr.assert_bits_equal(getattr(sgm, get)(), getattr(fresh, get)(), get)
        want = oracle.process(left, right, D)
        wr.assert_bits_equal(sgm.get_lr_disp(), want["lr"], "lr")


def test_switching_the_window_between_frames():
    left, right = pair()
    with SGM(H, W, 1, D) as sgm:
        before = sgm.device_bytes
        for window in ((5, 5), (9, 7), (7, 9), (5, 5)):
            sgm.set_window(*window)
            assert sgm.window == window and sgm.device_bytes == before  # (allocates nothing)
            sgm.process(left, right)
            check_frame(sgm, expected(window), 2)


@pytest.mark.timeout(120)
def test_frame_replays_from_a_hip_graph():
    with SGM(H, W, 1, D) as sgm:
        sgm.set_window(5, 5)
        stream = torch.cuda.ExternalStream(sgm.stream, device=DEV)
        d_l = torch.empty((H, W), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_e = torch.empty((H, W), dtype=torch.float32, device=DEV)
        out_g = torch.empty_like(out_e)

        def frame(out):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)

        def load(k):
            left, right = pair(index=k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))

        load(0)
        with torch.cuda.stream(stream):
            frame(out_e)  # warm-up (the capture needs no first-call work)
        torch.cuda.synchronize(DEV)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(out_g)
            with pytest.raises(SGMError, match="outside stream capture"):
                sgm.set_window(9, 7)
            assert sgm.window == (5, 5)
        torch.cuda.synchronize(DEV)
        for k in (1, 2):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
                frame(out_e)
            torch.cuda.synchronize(DEV)
            assert np.array_equal(wr.bits(out_g.cpu().numpy()), wr.bits(out_e.cpu().numpy())), k
        wr.assert_bits_equal(out_g.cpu().numpy(), expected((5, 5))["lr"], "replay")
