"""The reference's CT cost on the GPU (SGM_COST_CT: sgm_window_cost_device,
sgm_set_cost), bit for bit against tests/ct_cost_recipe.py, which
tests/test_ct_cost_cpu.py pins to the reference's own compiled CT: the producer
launch over pitched images into a canary-guarded volume, frames on the cost
against `recipe volume -> SGM.aggregate` on a census handle of the same
parameters and against the CPU oracle's stages on that volume, a HIP graph
replay, the refusals and the launch ledger of a CT frame."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import ct_cost_recipe as ct
import volume_filter_recipe
import volume_recipe
import window_recipe
from stereo_matching_amd import BM, SGM, _capi, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 7.5  # (no CT cost: they are integers)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def produce(s, left, right, pad=13):
    """window_cost(kind="ct") of host images into a canary-guarded buffer; pad: extra bytes per
    image row (pitch > width), filled with a value of its own."""
    h, w = left.shape
    rows, cols, D = s.rows, s.cols, s.max_disp
    imgs = []
    for img in (left, right):
        t = torch.full((h, w + pad), 0xEE, dtype=torch.uint8, device=DEV)
        t[:, :w] = dev(img)
        imgs.append(t[:, :w])
    n = rows * cols * D
    buf = torch.full((n + 512,), CANARY, dtype=torch.float32, device=DEV)
    out = buf[256:256 + n].view(rows, cols, D)
    got = s.window_cost(imgs[0], imgs[1], "ct", out=out)
    torch.cuda.synchronize(DEV)
    assert got is out
    b = buf.cpu().numpy()
    assert (b[:256] == CANARY).all() and (b[256 + n:] == CANARY).all()
    return out.cpu().numpy()


def handle_kw(name):
    _, _, _, _, m, window, weighted = ct.CASES[name]
    return dict(min_disp=m, window=window, weighted=weighted)


@pytest.mark.parametrize("name", list(ct.CASES))
def test_producer_equals_the_recipe(name):
    _, _, D, scale, _, _, _ = ct.CASES[name]
    left, right = ct.inputs(name)
    h, w = left.shape
    with SGM(h, w, scale, D, aux_only=True, **handle_kw(name)) as s:
        got = produce(s, left, right)
    want = ct.expected(name)
    assert np.array_equal(ct.bits(got), ct.bits(want))
    if name in ct.GOLDEN:  # and the reference's compiled CT itself
        assert np.array_equal(ct.bits(got), ct.bits(ct.reference(name)))


def test_tiles_on_either_side_of_the_census_identity():
    """A width from the producer's own column tile: tile 0 holds the first hw columns and the
    triangle j - disp < hw, tile 1 straddles j - disp = hw, tile 2 lies wholly where CT is the
    Hamming distance of two census tables, and the last tile holds the last hw columns."""
    tj = _capi.lib().sgm_window_cost_tile_cols()
    h, w, D, hw = 18, 3 * tj + 5, tj, 4
    assert tj >= 8 and D % 32 == 0
    left, right = synthetic.stereo_pair(h, w, D, pair_index=23, kind="noise")
    with SGM(h, w, 1, D, aux_only=True) as s:
        got = produce(s, left, right)
    assert np.array_equal(ct.bits(got), ct.bits(ct.volume(left, right, D)))
    region = ct.table_region(w, D, 9)
    assert not region[:tj].all() and region[:tj].any()             # tile 0: both kinds of element
    assert not region[tj:2 * tj].all() and region[tj:2 * tj].any()  # tile 1 straddles the edge
    assert region[2 * tj:3 * tj].all() and not region[3 * tj:].all()
    tl, tr = (window_recipe.census(x, 7, 9) for x in (left, right))
    xr = np.maximum(np.arange(w)[:, None] - np.arange(D)[None, :], 0)
    ham = ct.popcount(tl[:, :, None] ^ tr[:, xr]).astype(np.float32)
    assert np.array_equal(got[:, region], ham[:, region])
    assert (got[:, ~region] != ham[:, ~region]).any()


def test_host_twin_and_any_handle_serves():
    name = "edge_24x33_D32"
    left, right = ct.inputs(name)
    for kw in (dict(), dict(aux_only=True), dict(views=1, paths=4), dict(cost="sad")):
        with SGM(24, 33, 1, 32, **kw) as s:
            assert np.array_equal(ct.bits(s.stage_window_cost(left, right, "ct")), ct.bits(ct.expected(name)))


# ------------------------------------------------------------------ frames

# (case, what both handles are built with, what the CT handle alone is built with)
FRAME_CASES = [
    ("edge_24x33_D32", dict(views=1), {}),
    ("road_48x170_D64", dict(views=2), {}),
    ("road_48x170_D64", dict(views=1, paths=4), {}),
    ("m16_48x170_D64", dict(views=2), {}),                                      # min_disp
    ("road_48x170_D64", dict(views=2, volume_filter=(True, True)), {}),
    ("road_48x170_D64", dict(views=2, post_filter=True, post_filter_launches=8), {}),
    ("road_48x170_D64", dict(views=2, confidence=True), {}),
    ("win_9x7", dict(views=2), dict(window=(9, 7))),
    ("weighted_7x9", dict(views=2), dict(window=(7, 9), weighted=True)),
    ("odd_s2_51x99_D32", dict(views=2), {}),                                    # scale 2
]


def frame_maps(s, kw, run):
    """The maps a handle holds after `run` enqueued a frame (or an aggregate call) into a map."""
    out = torch.full((s.rows, s.cols), CANARY, dtype=torch.float32, device=DEV)
    raw = torch.zeros((s.rows, s.cols), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize(DEV)
    run(out, raw)
    s.check()
    torch.cuda.synchronize(DEV)
    maps = {"out": out.cpu().numpy(), "raw": raw.cpu().numpy().astype(np.float32)}
    if kw.get("confidence"):
        for v in range(kw["views"]):
            maps[f"ratio{v}"] = s.get_confidence(v)
    return maps


def oracle_map(C, m, scale, kw):
    """The CPU oracle's stages on the volume: the map a frame without post_filter writes."""
    paths, filters = kw.get("paths", 8), kw.get("volume_filter")
    if filters:
        out = volume_filter_recipe.recipe(C, m, scale, paths, (1 if filters[0] else 0) | (2 if filters[1] else 0))
    else:
        out = volume_recipe.recipe(C, m, scale, paths)
    return out["lr"] if kw["views"] == 2 else out["sub"]


@pytest.mark.parametrize("name,kw,ct_kw", FRAME_CASES)
def test_frame_equals_recipe_volume_through_aggregate_and_the_oracle(name, kw, ct_kw):
    _, _, D, scale, m, _, _ = ct.CASES[name]
    left, right = ct.inputs(name)
    h, w = left.shape
    volume = ct.expected(name)
    with SGM(h, w, scale, D, min_disp=m, **kw) as ref:
        assert ref.cost == "census"
        c = dev(volume)
        want = frame_maps(ref, kw, lambda out, raw: ref.aggregate(c, layout="hwd", out=out, raw=raw))
    with SGM(h, w, scale, D, min_disp=m, cost="ct", **kw, **ct_kw) as s:
        assert s.cost == "ct"
        dl, dr = dev(left), dev(right)
        before = s.device_bytes
        got = frame_maps(s, kw, lambda out, raw: s.process_device(dl.data_ptr(), dr.data_ptr(), out.data_ptr(),
                                                                  d_raw=raw.data_ptr()))
        assert s.device_bytes == before
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(ct.bits(got[k]), ct.bits(want[k])), k
        assert not (want["out"] == CANARY).all()
        # the two calls a frame stands for are window_cost -> aggregate: `want` is aggregate on
        # the recipe's volume, and the handle's own window_cost gives that volume
        vol = s.window_cost(dl, dr, "ct")
        torch.cuda.synchronize(DEV)
        assert np.array_equal(ct.bits(vol.cpu().numpy()), ct.bits(volume))
        # the host API's frame gives the same map
        s.process(left, right)
        host = s.get_disp() if kw.get("post_filter") else s.get_lr_disp()
        assert np.array_equal(ct.bits(host), ct.bits(want["out"]))
    if not kw.get("post_filter"):
        window_recipe.assert_bits_equal(got["out"], oracle_map(volume, m, scale, kw), "oracle")


@pytest.mark.timeout(120)
def test_frame_replays_from_a_hip_graph():
    h, w, D = 48, 170, 64
    with SGM(h, w, 1, D, cost="ct", post_filter=True, post_filter_launches=8) as s:
        stream = torch.cuda.ExternalStream(s.stream, device=DEV)
        d_l = torch.empty((h, w), dtype=torch.uint8, device=DEV)
        d_r = torch.empty_like(d_l)
        out_e = torch.empty((h, w), dtype=torch.float32, device=DEV)
        out_g = torch.empty_like(out_e)

        def frame(out):
            s.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)

        def load(k):
            left, right = synthetic.stereo_pair(h, w, D, pair_index=k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))

        load(0)
        with torch.cuda.stream(stream):
            frame(out_e)  # once eagerly before capturing
        torch.cuda.synchronize(DEV)
        s.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(out_g)
        torch.cuda.synchronize(DEV)
        for k in (1, 2):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
                frame(out_e)
            torch.cuda.synchronize(DEV)
            s.check()
            assert np.array_equal(ct.bits(out_g.cpu().numpy()), ct.bits(out_e.cpu().numpy())), k
    # (and the replayed frame is the recipe's: the last pair's volume through a census handle)
    left, right = synthetic.stereo_pair(h, w, D, pair_index=2)
    kw = dict(views=2, post_filter=True, post_filter_launches=8)
    with SGM(h, w, 1, D, **kw) as ref:
        c = dev(ct.volume(left, right, D))
        want = frame_maps(ref, kw, lambda out, raw: ref.aggregate(c, layout="hwd", out=out, raw=raw))
    assert np.array_equal(ct.bits(out_g.cpu().numpy()), ct.bits(want["out"]))


# ---------------------------------------------------------------- refusals

def test_refusals():
    h, w, D = 24, 80, 32
    L = _capi.lib()
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0)
    mask = synthetic.sky_mask(h, w)
    dl, dr, dm = dev(left), dev(right), dev(mask)
    out = torch.full((h, w), CANARY, dtype=torch.float32, device=DEV)
    vol = torch.full((h, w, D), CANARY, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    with SGM(h, w, 1, D, cost="ct") as s:
        kind = ctypes.c_int(-1)
        assert L.sgm_get_cost(s._h, ctypes.byref(kind)) == 0 and kind.value == 4
        # a non-NULL mask on a frame call, device and host
        for kw in (dict(d_sky_l=dm.data_ptr()), dict(d_sky_r=dm.data_ptr())):
            with pytest.raises(SGMError, match="sky masks") as ei:
                s.process_device(dl.data_ptr(), dr.data_ptr(), out.data_ptr(), **kw)
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
        with pytest.raises(SGMError, match="sky masks"):
            s.process(left, right, mask)
        with pytest.raises(SGMError, match="sky masks"):
            s.process(left, right, None, mask)
        # 3 is still no kind
        for k in (3, -1, 5):
            rc = L.sgm_set_cost(s._h, k)
            assert rc == _capi.SGM_ERR_INVALID_ARG and b"kind" in L.sgm_last_error(s._h)
        assert s.cost == "ct"
        with pytest.raises(ValueError, match="cost"):
            s.set_cost("mi")
        for f in (lambda: s.window_cost(dl, dr, "mi"), lambda: s.stage_window_cost(left, right, "census")):
            with pytest.raises(ValueError, match="kind"):
                f()

        def call(kind=4, l=dl.data_ptr(), r=dr.data_ptr(), pitch=w, dst=vol.data_ptr(), stream=None):
            _capi.check(L.sgm_window_cost_device(s._h, kind, ctypes.c_void_p(l), ctypes.c_void_p(r), pitch,
                                                 ctypes.c_void_p(dst), ctypes.c_void_p(stream)), s._h)

        for word, f in [("kind", lambda: call(kind=0)), ("kind", lambda: call(kind=3)), ("kind", lambda: call(kind=-1)),
                        ("NULL image", lambda: call(l=None)), ("NULL image", lambda: call(r=None)),
                        ("pitch", lambda: call(pitch=w - 1)), ("d_dst", lambda: call(dst=None)),
                        ("float pointer", lambda: call(dst=vol.data_ptr() + 2)),
                        ("hipStreamLegacy", lambda: call(stream=1))]:  # (void *)1: the legacy default stream
            with pytest.raises(SGMError, match=word) as ei:
                f()
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
    for word, make in [("BM", lambda: BM(h, w, 1, D)), ("aux_only", lambda: SGM(h, w, 1, D, aux_only=True)),
                       ("SGM_VIEW_RIGHT", lambda: SGM(h, w, 1, D, views=1, view="right")),
                       ("sky_detect", lambda: SGM(h, w, 1, D, sky_detect=True))]:
        with make() as s:
            with pytest.raises(SGMError, match=word) as ei:
                s.set_cost("ct")
            assert ei.value.code == _capi.SGM_ERR_INVALID_ARG
            assert s.cost == "census"
    with pytest.raises(SGMError, match="sky_detect"):
        SGM(h, w, 1, D, sky_detect=True, cost="ct")
    with pytest.raises(ValueError, match="cost"):
        SGM(h, w, 1, D, cost="mi")
    torch.cuda.synchronize(DEV)
    assert (out.cpu().numpy() == CANARY).all() and (vol.cpu().numpy() == CANARY).all()


def test_back_to_the_census_equals_a_fresh_handle():
    h, w, D = 48, 170, 64
    left, right = ct.inputs("road_48x170_D64")
    with SGM(h, w, 1, D) as fresh:
        fresh.process(left, right)
        want = fresh.get_lr_disp().copy()
    with SGM(h, w, 1, D, cost="ct") as s:
        s.process(left, right)
        on_ct = s.get_lr_disp().copy()
        s.set_cost("census")
        s.process(left, right)
        assert np.array_equal(ct.bits(s.get_lr_disp()), ct.bits(want))
        assert not np.array_equal(ct.bits(on_ct), ct.bits(want))


# ------------------------------------------------------------------ ledger

SWITCHES = ("SGM_BAND_ROWS", "SGM_SLANT", "SGM_VSTRIP", "SGM_P4_HPAIR", "SGM_CONFIDENCE")
# a SAD frame's launches with window_cost_ct in the producer's place, weighted or not
LEDGERS = {
    "ct_v1": (dict(views=1), None, False, {
        "window_cost_ct": (1, 25600.0),
        "pair_fwd_L3": (1, 25600.0),
        "stage_a": (1, 25600.0),
        "stage_b": (1, 25600.0),
        "sweep_L8_acc": (1, 25600.0),
        "pair_bwd_L4_final": (1, 25600.0),
    }),
    "ct_v2_weighted": (dict(), None, True, {
        "window_cost_ct": (1, 25600.0),
        "vol_import": (1, 25600.0),
        "pair_fwd_L3": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    }),
    "ct_v2_hv": (dict(), (True, True), False, {
        "window_cost_ct": (1, 25600.0),
        "vol_import": (1, 25600.0),
        "vol_hfilter": (1, 51200.0),
        "vfwd": (2, 25600.0),
        "stage_a": (2, 25600.0),
        "stage_b": (2, 25600.0),
        "sweep_L8_acc": (2, 25600.0),
        "pair_bwd_L4_final": (2, 25600.0),
        "lr": (1, 800.0),
    }),
}


@pytest.mark.parametrize("name", list(LEDGERS))
def test_ct_frame_ledger(name, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    kw, filt, weighted, want = LEDGERS[name]
    rng = np.random.default_rng(5)
    with SGM(20, 40, 1, 32, **kw) as s:
        s.set_cost("ct")
        if weighted:
            s.set_weighted(True)
        if filt:
            s.set_volume_filter(*filt)
        s.set_profiling(True)
        left, right = rng.integers(0, 256, (2, 20, 40), dtype=np.uint8)
        s.process(left, right)
        prof = s.get_profile()
    got = {k: (v[0], v[2]) for k, v in prof.items()}
    print(name, got)
    assert got == want
