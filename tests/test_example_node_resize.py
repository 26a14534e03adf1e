"""examples/stereo_node.cpp with the node's configured size (node.cpp:19-20,
75-78): given img_w img_h it builds the solver at that size and resizes both
camera images to it on the GPU before the sky detector, the matcher and the
point cloud see them.  Its three outputs equal the oracle's on
recipe(raw) (tests/resize_recipe.py), bit for bit."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import pyref
import resize_recipe as rr
import support
from stereo_matching_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "stereo_node.cpp")
CAM = (721.5377, 721.5377, 609.5593, 172.854)   # the example's defaults (KITTI image_0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC, link_hip=False)


def test_usage_names_the_size_arguments_and_twelve_arguments_are_refused(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "img_w img_h" in r.stderr
    r = subprocess.run([exe] + ["x"] * 11, capture_output=True, text=True)   # img_w without img_h
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("scale,raw,size", [(1, (157, 431), (150, 420)), (2, (375, 621), (300, 840))])
def test_example_node_resizes_to_the_configured_size(exe, tmp_path, scale, raw, size):
    import oracle
    oracle.build()
    D = 64
    (sh, sw), (h, w) = raw, size
    left, right = synthetic.stereo_pair(sh, sw, D, pair_index=21, kind="road")
    left[: sh // 5] //= 4          # a darker, flat band on top for the sky detector
    right[: sh // 5] //= 4
    support.write_pgm(tmp_path / "l.pgm", left)
    support.write_pgm(tmp_path / "r.pgm", right)
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), prefix, str(scale), str(D)]
                       + [repr(c) for c in CAM] + ["0", str(w), str(h)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"left size: {sh}, {sw}" in r.stdout and f"resized left size: {h}, {w}" in r.stdout
    assert f"resized right size: {h}, {w}" in r.stdout
    left, right = rr.resize(left, h, w), rr.resize(right, h, w)      # node.cpp:75-76
    H, W = h // scale, w // scale
    sky_l, sky_r = oracle.sky_detect(left, scale), oracle.sky_detect(right, scale)
    want = oracle.process(left, right, D, scale=scale, sky_l=sky_l, sky_r=sky_r)["final"]
    got = np.fromfile(prefix + "_disp.f32", np.float32).reshape(H, W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # show_disp (Solver.cpp:55-93): the resized gray left image on top, the colormap from row H-1
    with open(prefix + "_debug.ppm", "rb") as f:
        assert f.readline() == b"P6\n" and f.readline() == b"%d %d\n" % (W, 2 * H) and f.readline() == b"255\n"
        view = np.frombuffer(f.read(), np.uint8).reshape(2 * H, W, 3)[..., ::-1]   # RGB -> BGR
    small = left[: H * scale: scale, : W * scale: scale]
    assert np.array_equal(view[: H - 1], np.repeat(small[: H - 1, :, None], 3, axis=2))
    assert np.array_equal(view[H - 1: 2 * H - 1], pyref.colormap(want, D))
    # the point cloud (node.cpp:113-143) reads the resized img_l
    want_xyz, want_pix = pyref.point_cloud(want, left, D, scale, *CAM)
    raw_bytes = open(prefix + "_cloud.bin", "rb").read()
    n = len(want_pix)
    assert len(raw_bytes) == n * 25
    xyz = np.frombuffer(raw_bytes[: n * 24], np.float64).reshape(n, 3)
    assert np.array_equal(xyz.view(np.uint64), want_xyz.view(np.uint64))
    assert np.array_equal(np.frombuffer(raw_bytes[n * 24:], np.uint8), want_pix)
