"""The occlusion-aware hole filling (sgm_set_fill) on the GPU
against tests/fill_recipe.py, bit for bit on the map and the mask: the
stand-alone call over geometries, maps, modes and settings; frames of every
schedule small sizes reach; the refusals; off means off; a captured frame."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import fill_recipe
import reproject_recipe as rp
from support import bits
from stereo_matching_amd import BM, SGM, _capi, camera_q, synthetic
from stereo_matching_amd._capi import SGMError

pytestmark = pytest.mark.gpu

# (rows, cols): the smallest handle; rows < cols and rows > cols with cols no multiple of 64
# (diagonal lanes off the image); one segment; one column into a third segment (the carry
# between segments); more rows than two rings of the marches
GEOMS = [(3, 5), (37, 70), (70, 37), (64, 64), (65, 129), (130, 67)]
# (D, min_disp, scale, lr_max_diff)
SETTINGS = {"D32": (32, 0, 1, 1.0), "D32_m16_lr025": (32, 16, 1, 0.25), "D64_s2": (64, 0, 2, 1.0)}


def random_map(rng, rows, cols, share, D, m, nan=False):
    F = (m + rng.random((rows, cols)) * (D - 1)).astype(np.float32)
    F[rng.random((rows, cols)) < share] = D + m + 1
    if nan:
        F[rng.random((rows, cols)) < 0.1] = np.nan
    return F


def maps(rng, rows, cols, D, m):
    """name -> map: the shares, holes at every border and corner, whole rows and
    columns, all and nothing, NaN."""
    inv = np.float32(D + m + 1)
    out = {f"share{s}": random_map(rng, rows, cols, s, D, m) for s in (0.05, 0.5, 0.95)}
    hr, hc = max(1, rows // 3), max(1, cols // 3)
    for name, (rs, cs) in {"top": (slice(0, hr), slice(hc, 2 * hc)), "bottom": (slice(rows - hr, rows), slice(hc, 2 * hc)),
                           "left": (slice(hr, 2 * hr), slice(0, hc)), "right": (slice(hr, 2 * hr), slice(cols - hc, cols)),
                           "tl": (slice(0, hr), slice(0, hc)), "tr": (slice(0, hr), slice(cols - hc, cols)),
                           "bl": (slice(rows - hr, rows), slice(0, hc)),
                           "br": (slice(rows - hr, rows), slice(cols - hc, cols))}.items():
        F = random_map(rng, rows, cols, 0.0, D, m)
        F[rs, cs] = inv
        out["hole_" + name] = F
    F = random_map(rng, rows, cols, 0.1, D, m)
    F[rows // 2] = inv
    F[:, cols // 2] = inv
    F[0] = inv
    F[:, cols - 1] = inv
    out["lines"] = F
    out["none"] = np.full((rows, cols), inv, np.float32)
    out["all"] = random_map(rng, rows, cols, 0.0, D, m)
    out["nan"] = random_map(rng, rows, cols, 0.4, D, m, nan=True)
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("rows,cols", GEOMS)
def test_stand_alone_fill_equals_the_recipe(rows, cols, setting):
    D, m, s, lr = SETTINGS[setting]
    rng = np.random.default_rng(rows * 1000 + cols + D + m)
    with SGM(rows * s, cols * s, s, D, aux_only=True, min_disp=m, lr_max_diff=lr, fill="interpolate") as sgm:
        for name, F in maps(rng, rows, cols, D, m).items():
            R = random_map(rng, rows, cols, 0.3, D, m, nan=name == "nan")
            for mode in ("background", "interpolate"):
                want, wmask = fill_recipe.fill(F, D, m, s, R, mode, lr)
                got, mask = sgm.fill_disp(F, right=R, mode=mode)
                assert np.array_equal(mask, wmask), (name, mode)
                assert np.array_equal(bits(got), bits(want)), (name, mode)
        assert np.array_equal(sgm.get_fill_mask(), wmask)      # the handle's mask: the last fill's


@pytest.mark.parametrize("rows,cols", GEOMS)
def test_pitched_device_buffers(rows, cols):
    """pitch > cols for the map, the right map and the mask; the padding stays."""
    D, m, s, lr = SETTINGS["D32"]
    rng = np.random.default_rng(rows + cols)
    F, R = random_map(rng, rows, cols, 0.5, D, m, nan=True), random_map(rng, rows, cols, 0.3, D, m)
    want, wmask = fill_recipe.fill(F, D, m, s, R, "interpolate", lr)
    dev = torch.device("cuda", 0)
    pad = lambda a, p, v: np.concatenate([a, np.full((rows, p - cols), v, a.dtype)], axis=1)
    pf, pr, pm = cols + 3, cols + 7, cols + 5
    with SGM(rows, cols, s, D, aux_only=True, fill="background") as sgm:
        d_f = torch.from_numpy(pad(F, pf, -7.0)).to(dev)
        d_r = torch.from_numpy(pad(R, pr, 3.0)).to(dev)
        d_m = torch.full((rows, pm), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        sgm.fill_device(d_f.data_ptr(), d_right=d_r.data_ptr(), mode="interpolate", d_mask=d_m.data_ptr(),
                        pitch=pf, right_pitch=pr, mask_pitch=pm)
        sgm.check()
        got, mask = d_f.cpu().numpy(), d_m.cpu().numpy()
    assert np.array_equal(mask[:, :cols], wmask) and (mask[:, cols:] == 9).all()
    assert np.array_equal(bits(got[:, :cols]), bits(want)) and (got[:, cols:] == -7.0).all()


# ------------------------------------------------------------------ frames
H, W, D = 48, 96, 32
Q = camera_q(500.0, 500.0, 48.0, 24.0, 0.5)


def pair():
    return synthetic.stereo_pair(H, W, D, pair_index=3)


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("sched", ["default", "slant", "paths4"])
def test_filled_frame_equals_the_recipe_on_the_unfilled_frame(sched, s, post, monkeypatch):
    """Every schedule small sizes reach (the slanted one keeps d_sub[1] row-major, the others
    column-major); with post_filter under a launch budget; XYZ from the dense map."""
    if sched == "slant":
        monkeypatch.setenv("SGM_SLANT", "1")
    kw = dict(paths=4 if sched == "paths4" else 8)
    left, right = pair()
    rows, cols = H // s, W // s
    budget = -(-cols // 64) * rows + 1
    pkw = dict(post_filter=True, post_filter_launches=budget) if post else {}
    with SGM(H, W, s, D, **kw, **pkw) as off, SGM(H, W, s, D, views=1, view="right", **kw) as rv:
        off.process(left, right)
        base = off.get_disp() if post else off.get_lr_disp()
        rv.process(left, right)
        R = rv.get_lr_disp()
    share = float((base > D - 1).mean())
    print(sched, s, post, "invalid share of the unfilled map", share)
    assert 0.0 < share < 1.0
    for mode in ("interpolate", "background"):
        want, wmask = fill_recipe.fill(base, D, 0, s, R, mode, 1.0)
        with SGM(H, W, s, D, fill=mode, reproject=Q, **kw, **pkw) as sgm:
            assert sgm.fill == mode
            sgm.process(left, right)
            sgm.check()
            got = sgm.get_disp()
            assert np.array_equal(sgm.get_fill_mask(), wmask), mode
            assert np.array_equal(bits(got), bits(want)), mode
            xyz = rp.reproject(want, Q.ravel(), sgm.invalid_disp, s)["xyz"]
            assert np.array_equal(bits(sgm.get_xyz()), bits(xyz)), mode
    assert (wmask == fill_recipe.OCCLUSION).any()


def test_get_disp_fills_after_the_post_filter():
    """A handle without params.post_filter: get_disp() = fill(post_filter(lr)), right = None."""
    left, right = pair()
    with SGM(H, W, 1, D) as off, SGM(H, W, 1, D, views=1, view="right") as rv, SGM(H, W, 1, D) as sgm:
        off.process(left, right)
        rv.process(left, right)
        want, _ = fill_recipe.fill(off.get_disp(), D, 0, 1, rv.get_lr_disp(), "interpolate", 1.0)
        sgm.process(left, right)
        sgm.set_fill("interpolate")          # (after the frame: the map kept is the LR map)
        assert np.array_equal(bits(sgm.get_disp()), bits(want))


@pytest.mark.parametrize("kind", ["sad", "aggregate"])
def test_volume_frames_fill_too(kind):
    left, right = pair()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    # a random volume with a surface in it: the road's disparities cost least, under noise
    g = synthetic.ground_truth(H, D)[:, None, None]
    cost = 10.0 * np.abs(np.arange(D)[None, None, :] - g) + 25.0 * rng.random((H, W, D))
    vol = torch.from_numpy(cost.astype(np.float32)).to(dev)

    def frame(sgm):
        if kind == "sad":
            sgm.process(left, right)
            return sgm.get_disp() if sgm.fill != "off" else sgm.get_lr_disp()
        out = sgm.aggregate(vol)
        torch.cuda.synchronize(dev)
        sgm.check()
        return out.cpu().numpy()

    ckw = dict(cost="sad") if kind == "sad" else {}
    with SGM(H, W, 1, D, **ckw) as off:
        base = frame(off)
    print(kind, "invalid share of the unfilled map", float((base > D - 1).mean()))
    assert 0.0 < float((base > D - 1).mean()) < 1.0
    want, wmask = fill_recipe.fill(base, D, mode="background")
    with SGM(H, W, 1, D, fill="background", **ckw) as sgm:
        got = frame(sgm)
        assert np.array_equal(sgm.get_fill_mask(), wmask)
        assert np.array_equal(bits(got), bits(want))
    # interpolate: the frame's own right view, which the stand-alone call reads with right = None
    with SGM(H, W, 1, D, fill="interpolate", **ckw) as sgm:
        got = frame(sgm)
        mask = sgm.get_fill_mask()
        again, amask = sgm.fill_disp(base, right=None)
        assert np.array_equal(mask, amask) and np.array_equal(bits(got), bits(again))
        assert np.array_equal(mask != 0, wmask != 0) and (mask == fill_recipe.MISMATCH).any()


@pytest.mark.parametrize("make", ["bm", "one_view", "gpu_sgm_post"])
def test_bm_and_one_view_handles_fill_the_background(make):
    left, right = pair()

    def handle(fill):
        if make == "bm":
            return BM(H, W, 1, D, fill=fill)
        return SGM(H, W, 1, D, views=1, fill=fill, post_filter=make == "gpu_sgm_post")

    with handle("off") as off:
        off.process(left, right)
        base = off.get_disp() if make != "one_view" else off.get_lr_disp()
    want, wmask = fill_recipe.fill(base, D, mode="background")
    assert (wmask != 0).any()
    with handle("background") as sgm:
        sgm.process(left, right)
        assert np.array_equal(sgm.get_fill_mask(), wmask)
        assert np.array_equal(bits(sgm.get_disp()), bits(want))


# --------------------------------------------------------------- refusals
def refused(sgm, call):
    with pytest.raises(SGMError) as e:
        call()
    assert e.value.code == _capi.SGM_ERR_INVALID_ARG
    assert _capi.lib().sgm_last_error(sgm._h)


def test_refusals():
    F = np.full((H, W), D + 1, np.float32)
    with SGM(H, W, 1, D, views=1) as one, BM(H, W, 1, D) as bm, SGM(H, W, 1, D, aux_only=True) as aux, \
            SGM(H, W, 1, D, views=1, view="right") as rv, SGM(H, W, 1, D) as two:
        refused(one, lambda: one.set_fill("interpolate"))
        refused(bm, lambda: bm.set_fill("interpolate"))
        for mode in ("background", "interpolate"):
            refused(rv, lambda: rv.set_fill(mode))
        refused(two, lambda: two.set_fill(3))
        refused(two, lambda: two.set_fill(-1))
        refused(aux, lambda: aux.fill_disp(F, mode="background"))        # no scratch yet
        aux.set_fill("background")
        refused(aux, lambda: aux.fill_disp(F, right=None, mode="interpolate"))
        refused(aux, lambda: aux.fill_disp(F, mode="off"))
        refused(aux, lambda: aux.fill_device(1 << 20, mode="background", stream=0))   # hipStreamLegacy
        refused(aux, lambda: aux.get_fill_mask())                         # nothing filled yet
        one.set_fill("background")
        refused(one, lambda: one.fill_disp(F, right=None, mode="interpolate"))
        assert one.fill == "background" and bm.fill == "off" and rv.fill == "off" and two.fill == "off"
        with pytest.raises(ValueError):
            two.set_fill("dense")


# ------------------------------------------------------------ off means off
@pytest.mark.parametrize("views", [1, 2])
def test_off_means_off(views):
    left, right = pair()

    def names(sgm):
        sgm.set_profiling(True)
        sgm.process(left, right)
        prof = sgm.get_profile()
        sgm.set_profiling(False)
        return {k: v[0] for k, v in prof.items()}

    with SGM(H, W, 1, D, views=views) as fresh, SGM(H, W, 1, D, views=views) as sgm:
        want, nbytes = names(fresh), fresh.device_bytes
        assert sgm.device_bytes == nbytes
        assert names(sgm) == want and not any(k.startswith("fill") for k in want)
        lr = sgm.get_lr_disp().copy()
        sgm.set_fill("background")
        assert sgm.device_bytes == nbytes + 25 * H * W        # six fp32 planes and the mask
        on = names(sgm)
        assert on == {**want, "fill_march": 1, "fill_select": 1}
        sgm.set_fill("off")
        assert sgm.device_bytes == nbytes and sgm.fill == "off"
        assert names(sgm) == want
        assert np.array_equal(bits(sgm.get_lr_disp()), bits(lr))


# -------------------------------------------------------------------- graph
@pytest.mark.timeout(120)
def test_filled_frame_replays_from_a_hip_graph():
    dev = torch.device("cuda", 0)
    budget = 8
    with SGM(H, W, 1, D, post_filter=True, post_filter_launches=budget, fill="interpolate") as sgm:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
        d_l = torch.empty((H, W), dtype=torch.uint8, device=dev)
        d_r = torch.empty_like(d_l)
        out_e = torch.empty((H, W), dtype=torch.float32, device=dev)
        out_g = torch.empty_like(out_e)
        d_mask, pitch = ctypes.c_void_p(), ctypes.c_int()

        def frame(out):
            sgm.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)

        def load(k):
            left, right = synthetic.stereo_pair(H, W, D, pair_index=k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))

        load(0)
        frame(out_g)                                   # warm-up
        torch.cuda.synchronize(dev)
        sgm.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(out_g)
            refused(sgm, lambda: sgm.set_fill("off"))          # the setter: outside capture only
            assert "outside stream capture" in sgm._lib.sgm_last_error(sgm._h).decode()
        torch.cuda.synchronize(dev)
        assert sgm.fill == "interpolate"
        for k in (1, 2):
            load(k)
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize(dev)
            sgm.check()
            g, gmask = out_g.cpu().numpy(), sgm.get_fill_mask()
            frame(out_e)                               # the eager frame of the same buffers
            torch.cuda.synchronize(dev)
            sgm.check()
            e, emask = out_e.cpu().numpy(), sgm.get_fill_mask()
            assert np.array_equal(bits(g), bits(e)), k
            assert np.array_equal(gmask, emask), k
            assert (gmask != 0).any() and (gmask == 0).any()
            _capi.check(_capi.lib().sgm_get_fill_mask(sgm._h, ctypes.byref(d_mask), ctypes.byref(pitch)), sgm._h)
            assert d_mask.value and pitch.value == W
