"""Weighted windows on the GPU (sgm_set_weighted), bit for bit over
every pixel and every disparity: the masked census launch and the weighted SAD /
SSD producer against tests/weighted_recipe.py (pinned on the CPU to fixtures the
reference's own compiled functions wrote) and against those fixtures themselves,
whole frames against the oracle's stages on the recipe's tables and volumes, the
setter's refusals, a HIP-graph replay and the launches' profile names."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import weighted_recipe as wt
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

CENSUS_CASES = [(shape, s, win) for s in (1, 2) for shape in wt.CENSUS_SHAPES for win in wt.CENSUS_WINDOWS[s]]


@pytest.mark.parametrize("case", CENSUS_CASES, ids=census_id)
def test_masked_census_equals_the_reference(case):
    shape, s, win = case
    left, right = cases.census_pair(shape, s)
    h, w = left.shape
    with SGM(h, w, s, 32, views=1, blur=False, window=win, weighted=True) as sgm:
        assert sgm.weighted and sgm.window == win
        for img, want in zip((left, right), cases.ref_census(shape, s, win, "weighted")):
            assert np.array_equal(sgm.stage_census(img), want)


@pytest.mark.parametrize("case", CENSUS_CASES, ids=census_id)
def test_blurred_masked_census_equals_the_recipe(case):
    shape, s, win = case
    left, _ = cases.census_pair(shape, s)
    h, w = left.shape
    with SGM(h, w, s, 32, views=1, blur=True, window=win, weighted=True) as sgm:
        assert np.array_equal(sgm.stage_census(left), wr.frame_census(left, win, s, blur=True, weighted=True))


# ------------------------------------------------------- weighted producer

COST_CASES = ([(name, 1, win) for name in wt.COST_SHAPES for win in wt.COST_WINDOWS[1]]
              + [(name, 2, win) for name in cases.COST_S2_SHAPES for win in wt.COST_WINDOWS[2]])


@pytest.mark.parametrize("case", COST_CASES, ids=lambda c: f"{c[0]}_s{c[1]}_{cases.wid(c[2])}")
def test_weighted_window_cost_equals_the_recipe(case):
    """D = 32 and 64, min_disp 0 and 16, SAD and SSD; 3x5 and 10x20 are narrower than D."""
    name, s, win = case
    left, right = cases.cost_pair(name, s)
    h, w = left.shape
    for D in cases.COST_D:
        for m in cases.COST_MIN_DISP:
            with SGM(h, w, s, D, aux_only=True, min_disp=m, window=win, weighted=True) as sgm:
                for kind in cases.KINDS:
                    got = sgm.stage_window_cost(left, right, kind)
                    want = wt.volume(left, right, D, kind, win, s, m)
                    assert np.array_equal(wr.bits(got), wr.bits(want)), (D, m, kind)


@pytest.mark.parametrize("case", wt.COST_FIXTURES, ids=lambda c: f"{c[0]}_s{c[1]}_{cases.wid(c[2])}")
def test_weighted_window_cost_equals_the_reference(case):
    name, s, win = case
    left, right = cases.cost_pair(name, s)
    h, w = left.shape
    with SGM(h, w, s, 64, aux_only=True, min_disp=16, window=win, weighted=True) as sgm:
        for kind in cases.KINDS:
            want = np.ascontiguousarray(cases.ref_cost(name, s, win, kind, "weighted")[:, :, 16:80])
            assert np.array_equal(wr.bits(sgm.stage_window_cost(left, right, kind)), wr.bits(want)), kind


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_second_disparity_chunk(kind):
    left, right = cases.cost_pair("20x70", 1)
    with SGM(20, 70, 1, 128, aux_only=True, weighted=True) as sgm:  # (7, 9): 63 taps, shifts up to 127
        got = sgm.stage_window_cost(left, right, kind)
    assert np.array_equal(wr.bits(got), wr.bits(wt.volume(left, right, 128, kind, (7, 9))))


def test_window_cost_on_device_tensors_of_an_aux_only_handle():
    left, right = cases.cost_pair("20x70", 1)
    with SGM(20, 70, 1, 64, aux_only=True, weighted=True) as sgm:
        got = sgm.window_cost(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), "sad")
        torch.cuda.synchronize(DEV)
    want = np.ascontiguousarray(cases.ref_cost("20x70", 1, (7, 9), "sad", "weighted")[:, :, :64])
    assert np.array_equal(wr.bits(got.cpu().numpy()), wr.bits(want))


def test_window_weights_are_the_recorded_table():
    with np.load(wt.WEIGHTS_FIXTURE) as z:
        for s, wins in wt.COST_WINDOWS.items():
            for win in wins:
                with SGM(24 * s, 33 * s, s, 32, aux_only=True, window=win, weighted=True) as sgm:
                    got = sgm.window_weights()
                e = cases.effective(win, s)
                assert got.shape == e and np.array_equal(got.view(np.uint32), z[f"{e[0]}x{e[1]}"].view(np.uint32))


# ------------------------------------------------------------------ frames

H, W, D = 24, 96, 32


def pair(index=2):
    return synthetic.stereo_pair(H, W, D, pair_index=index, kind="road")


@functools.lru_cache(maxsize=None)
def expected(views=2, paths=8, cost="census", solver="sgm", filters=(False, False), index=2):
    left, right = pair(index)
    out = wr.recipe(left, right, D, (7, 9), 1, None, paths, 0, True, views, cost, solver, True, filters)
    for a in out.values():
        a.setflags(write=False)
    return out


def check_frame(sgm, want, views):
    wr.assert_bits_equal(sgm.get_raw_disp(), want["disp"], "disp")
    wr.assert_bits_equal(sgm.get_lr_disp(), want["lr"] if views == 2 else want["sub"], "sub")
    wr.assert_bits_equal(sgm.get_disp(), want["final"], "final")


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("views", [1, 2])
def test_census_frame_equals_the_oracle_on_the_masked_tables(views, paths):
    left, right = pair()
    with SGM(H, W, 1, D, views=views, paths=paths, weighted=True) as sgm:
        sgm.process(left, right)
        check_frame(sgm, expected(views, paths), views)


def frame_maps(s, run):
    """The maps a handle holds after `run` enqueued a frame (or an aggregate call) into a map
    (tests/test_gpu_window_cost.py's path)."""
    out = torch.full((s.rows, s.cols), -77.0, dtype=torch.float32, device=DEV)
    raw = torch.zeros((s.rows, s.cols), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize(DEV)
    run(out, raw)
    s.check()
    torch.cuda.synchronize(DEV)
    return {"out": out.cpu().numpy(), "raw": raw.cpu().numpy()}


def check_volume_frame(kind, **kw):
    """A weighted SAD / SSD frame against an unweighted census handle of the same parameters
    aggregating the recipe's weighted volume (the path the oracle pins)."""
    left, right = pair()
    volume = torch.from_numpy(wt.volume(left, right, D, kind, (7, 9))).to(DEV)
    with SGM(H, W, 1, D, **kw) as ref:
        want = frame_maps(ref, lambda out, raw: ref.aggregate(volume, layout="hwd", out=out, raw=raw))
    with SGM(H, W, 1, D, cost=kind, weighted=True, **kw) as sgm:
        dl, dr = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
        got = frame_maps(sgm, lambda out, raw: sgm.process_device(dl.data_ptr(), dr.data_ptr(), out.data_ptr(),
                                                                  d_raw=raw.data_ptr()))
    for k in want:
        assert np.array_equal(wr.bits(got[k]), wr.bits(want[k])), k
    assert not (want["out"] == -77.0).all()
    return got


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("views", [1, 2])
def test_sad_frame_equals_the_weighted_volume_through_aggregate(views, paths):
    got = check_volume_frame("sad", views=views, paths=paths)
    if views == 2:  # and the CPU oracle's stages on the same volume
        wr.assert_bits_equal(got["out"], expected(2, paths, "sad")["lr"], "lr")


def test_ssd_frame_with_the_cost_filters():
    got = check_volume_frame("ssd", volume_filter=(True, True))
    wr.assert_bits_equal(got["out"], expected(2, 8, "ssd", filters=(True, True))["lr"], "lr")


def test_bm_frame():
    left, right = pair()
    want = expected(solver="bm")
    with BM(H, W, 1, D, weighted=True) as bm:
        assert bm.weighted
        bm.process(left, right)
        wr.assert_bits_equal(bm.get_raw_disp(), want["disp"], "disp")
        wr.assert_bits_equal(bm.get_disp(), want["final"], "final")


def test_right_view_handle_takes_the_setting():
    with SGM(H, W, 1, D, views=1, view="right") as sgm:
        sgm.set_weighted(True)
        assert sgm.weighted
        sgm.set_weighted(False)
        assert not sgm.weighted


def test_set_and_cleared_again_is_an_untouched_handle():
    left, right = pair()
    with SGM(H, W, 1, D) as fresh, SGM(H, W, 1, D, weighted=True) as sgm:
        before = sgm.device_bytes
        sgm.set_weighted(False)
        assert not sgm.weighted and not fresh.weighted and sgm.device_bytes == before == fresh.device_bytes
        fresh.process(left, right)
        sgm.process(left, right)
        for get in ("get_raw_disp", "get_lr_disp", "get_disp"):
            wr.assert_bits_equal(getattr(sgm, get)(), getattr(fresh, get)(), get)
        sgm.set_weighted(True)
        sgm.process(left, right)
        check_frame(sgm, expected(), 2)


# ------------------------------------------------------------------ setter

def test_refusals_carry_their_messages_and_change_nothing():
    L = _capi.lib()
    # the default (7, 9) at scale 2 is 3 x 4: weighting is refused, in either order
    with SGM(H * 2, W * 2, 2, D, aux_only=True) as half:
        assert L.sgm_set_weighted(half._h, 1) == _capi.SGM_ERR_INVALID_ARG
        msg = L.sgm_last_error(half._h)
        assert b"sgm_set_weighted" in msg and b"odd" in msg and b"(7, 9) at scale 2" in msg
        assert not half.weighted
        with pytest.raises(SGMError, match="not weighted"):
            half.window_weights()
        half.set_window(14, 18)
        half.set_weighted(True)
        assert half.weighted and half.window_weights().shape == (7, 9)
        for bad in ((7, 9), (10, 12), (14, 16), (18, 18), (1, 9)):
            assert L.sgm_set_window(half._h, *bad) == _capi.SGM_ERR_INVALID_ARG
            assert b"sgm_set_window" in L.sgm_last_error(half._h)
            assert half.window == (14, 18) and half.weighted
        assert b"odd" in L.sgm_last_error(half._h) or b"1..9" in L.sgm_last_error(half._h)
        half.set_window(10, 18)
        assert half.window_weights().shape == (5, 9)
    with SGM(H, W, 1, D) as sgm:
        sgm.set_window(5, 6)
        with pytest.raises(SGMError, match="sgm_set_weighted.*odd") as ei:
            sgm.set_weighted(True)
        assert ei.value.code == _capi.SGM_ERR_INVALID_ARG and not sgm.weighted and sgm.window == (5, 6)
        sgm.set_window(5, 5)
        sgm.set_weighted(True)
        with pytest.raises(SGMError, match="sgm_set_window.*odd"):
            sgm.set_window(5, 6)
        with pytest.raises(SGMError, match="sgm_set_window.*64 bits"):
            sgm.set_window(9, 9)
        assert sgm.window == (5, 5) and sgm.weighted
        sgm.set_weighted(False)
        sgm.set_window(5, 6)  # (accepted again once weighting is off)
    with pytest.raises(SGMError, match="sgm_set_weighted"):
        SGM(H * 2, W * 2, 2, D, weighted=True)


# ------------------------------------------------------------------ graph

@pytest.mark.timeout(120)
def test_weighted_frame_replays_from_a_hip_graph():
    with SGM(H, W, 1, D, weighted=True) as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=DEV)
        d_l = torch.empty((H, W), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_e = torch.empty((H, W), dtype=torch.float32, device=DEV)
        out_g = torch.empty_like(out_e)

        def frame(out):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)

        def load(k):
            left, right = pair(k)
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
                sgm.set_weighted(False)
            assert sgm.weighted
        torch.cuda.synchronize(DEV)
        for k in (1, 2):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
                frame(out_e)
            torch.cuda.synchronize(DEV)
            assert np.array_equal(wr.bits(out_g.cpu().numpy()), wr.bits(out_e.cpu().numpy())), k
        wr.assert_bits_equal(out_g.cpu().numpy(), expected()["lr"], "replay")


# ---------------------------------------------------------------- launches

def frame_names(sgm):
    left, right = pair()
    sgm.set_profiling(True)
    sgm.process(left, right)
    names = sgm.get_profile()
    sgm.set_profiling(False)
    return {k: v[0] for k, v in names.items()}  # class -> launches


@pytest.mark.parametrize("cost,plain,other", [("census", "census", "census_masked"),
                                              ("sad", "window_cost", "window_cost_weighted")])
def test_only_the_one_launch_changes(cost, plain, other):
    with SGM(H, W, 1, D, cost=cost) as fresh, SGM(H, W, 1, D, cost=cost) as sgm:
        base = frame_names(fresh)
        assert plain in base and other not in base
        sgm.set_weighted(True)
        on = frame_names(sgm)
        sgm.set_weighted(False)
        assert frame_names(sgm) == base  # set and cleared again
        assert other in on and plain not in on
        on[plain] = on.pop(other)
        assert on == base
