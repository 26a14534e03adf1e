"""examples/stereo_node.cpp with colour images: given two binary PPM files (P6)
it reads them as RGB8, sets the solver's input format and feeds process() the
colour pair; the sky detector, the matcher, the debug view and the point cloud
see the grey pair.  Its outputs equal the oracle's and pyref's on
recipe.gray(raw) (tests/gray_recipe.py), bit for bit; a P5 pair still gives what
it gave."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import gray_recipe as gr
import pyref
import support
from stereo_matching_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "stereo_node.cpp")
CAM = (721.5377, 721.5377, 609.5593, 172.854)   # the example's defaults (KITTI image_0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC, link_hip=False)


def _pnm(path, img):
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P6" if img.ndim == 3 else b"P5", img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def colourise(g):
    """An RGB image whose channels differ, from a grey one."""
    out = np.empty(g.shape + (3,), np.uint8)
    out[..., 0] = g
    out[..., 1] = g.astype(np.int64) * 3 // 4 + 17
    out[..., 2] = 255 - g
    return out


def test_mixed_pairs_are_refused(exe, tmp_path):
    g = np.zeros((4, 6), np.uint8)
    _pnm(tmp_path / "g.pgm", g)
    _pnm(tmp_path / "c.ppm", colourise(g))
    r = subprocess.run([exe, str(tmp_path / "g.pgm"), str(tmp_path / "c.ppm"), str(tmp_path / "o")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "cannot read" in r.stderr


def check_outputs(prefix, stdout, left, want, scale, D):
    """The example's three files against the map `want` and the grey left image."""
    H, W = want.shape
    got = np.fromfile(prefix + "_disp.f32", np.float32).reshape(H, W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with open(prefix + "_debug.ppm", "rb") as f:
        assert f.readline() == b"P6\n" and f.readline() == b"%d %d\n" % (W, 2 * H) and f.readline() == b"255\n"
        view = np.frombuffer(f.read(), np.uint8).reshape(2 * H, W, 3)[..., ::-1]   # RGB -> BGR
    small = left[: H * scale: scale, : W * scale: scale]
    assert np.array_equal(view[: H - 1], np.repeat(small[: H - 1, :, None], 3, axis=2))
    assert np.array_equal(view[H - 1: 2 * H - 1], pyref.colormap(want, D))
    want_xyz, want_pix = pyref.point_cloud(want, left, D, scale, *CAM)
    raw = open(prefix + "_cloud.bin", "rb").read()
    n = len(want_pix)
    assert len(raw) == n * 25
    xyz = np.frombuffer(raw[: n * 24], np.float64).reshape(n, 3)
    assert np.array_equal(xyz.view(np.uint64), want_xyz.view(np.uint64))
    assert np.array_equal(np.frombuffer(raw[n * 24:], np.uint8), want_pix)
    assert f"pointcloud size: {n}, {n}" in stdout


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2])
def test_example_node_takes_a_colour_pair(exe, tmp_path, scale):
    import oracle
    oracle.build()
    D = 64
    h, w = 150 * scale, 420 * scale
    gl, gr_ = synthetic.stereo_pair(h, w, D, pair_index=21, kind="road")
    gl[: h // 5] //= 4             # a darker, flat band on top for the sky detector
    gr_[: h // 5] //= 4
    left, right = colourise(gl), colourise(gr_)
    _pnm(tmp_path / "l.ppm", left)
    _pnm(tmp_path / "r.ppm", right)
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, str(tmp_path / "l.ppm"), str(tmp_path / "r.ppm"), prefix, str(scale), str(D)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    yl, yr = gr.gray(left, "rgb8"), gr.gray(right, "rgb8")
    assert not np.array_equal(yl, gl)        # (the conversion is not a channel pick)
    sky_l, sky_r = oracle.sky_detect(yl, scale), oracle.sky_detect(yr, scale)
    want = oracle.process(yl, yr, D, scale=scale, sky_l=sky_l, sky_r=sky_r)["final"]
    check_outputs(prefix, r.stdout, yl, want, scale, D)
    # the same pair, converted on the host and written as P5, gives the same files
    _pnm(tmp_path / "l.pgm", yl)
    _pnm(tmp_path / "r.pgm", yr)
    prefix5 = str(tmp_path / "out5")
    r = subprocess.run([exe, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), prefix5, str(scale), str(D)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    check_outputs(prefix5, r.stdout, yl, want, scale, D)
    for ext in ("_disp.f32", "_debug.ppm", "_cloud.bin"):
        assert open(prefix + ext, "rb").read() == open(prefix5 + ext, "rb").read(), ext
