"""examples/stereo_node.cpp with rectification maps: given img_w img_h and
MAPS.f32 it builds the solver at that size, sets the maps and feeds process()
the raw camera images; the sky detector, the matcher and the point cloud see
the rectified pair.  Its outputs equal the Python class's on the same raw
images and maps, and the recipe's rectified images (tests/rectify_recipe.py),
bit for bit."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import pyref
import rectify_recipe as rc
import support
from stereo_matching_amd import SGM, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "stereo_node.cpp")
CAM = (721.5377, 721.5377, 609.5593, 172.854)   # the example's defaults (KITTI image_0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC, link_hip=False)


def test_usage_names_the_maps_argument(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "MAPS.f32" in r.stderr
    r = subprocess.run([exe] + ["x"] * 14, capture_output=True, text=True)   # one argument too many
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_example_node_rectifies_raw_images(exe, tmp_path):
    D = 64
    (sh, sw), (h, w) = (157, 431), (150, 420)
    left, right = synthetic.stereo_pair(sh, sw, D, pair_index=21, kind="road")
    left[: sh // 5] //= 4          # a darker, flat band on top for the sky detector
    right[: sh // 5] //= 4
    ml, mr = rc.maps(h, w, sh, sw, 0), rc.maps(h, w, sh, sw, 1)
    support.write_pgm(tmp_path / "l.pgm", left)
    support.write_pgm(tmp_path / "r.pgm", right)
    np.stack([*ml, *mr]).astype(np.float32).tofile(tmp_path / "maps.f32")
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), prefix, "1", str(D)]
                       + [repr(c) for c in CAM] + ["0", str(w), str(h), str(tmp_path / "maps.f32")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"left size: {sh}, {sw}" in r.stdout and f"rectified left size: {h}, {w}" in r.stdout
    assert f"rectified right size: {h}, {w}" in r.stdout
    # the Python class on the same raw pair and maps; the masks from the recipe's rectified images
    rl, rr = rc.remap(left, *ml), rc.remap(right, *mr)
    with SGM(h, w, 1, D, post_filter=True, rectify=(sh, sw, *ml, *mr)) as sgm:
        sky_l, sky_r = sgm.sky_detect(rl), sgm.sky_detect(rr)     # (the stage calls take full-size images)
        sgm.process(left, right, sky_l, sky_r)
        want = sgm.get_disp()
        assert np.array_equal(sgm.rectified(0), rl)
    got = np.fromfile(prefix + "_disp.f32", np.float32).reshape(h, w)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # show_disp (Solver.cpp:55-93): the rectified gray left image on top, the colormap from row h-1
    with open(prefix + "_debug.ppm", "rb") as f:
        assert f.readline() == b"P6\n" and f.readline() == b"%d %d\n" % (w, 2 * h) and f.readline() == b"255\n"
        view = np.frombuffer(f.read(), np.uint8).reshape(2 * h, w, 3)[..., ::-1]   # RGB -> BGR
    assert np.array_equal(view[: h - 1], np.repeat(rl[: h - 1, :, None], 3, axis=2))
    assert np.array_equal(view[h - 1: 2 * h - 1], pyref.colormap(want, D))
    # the point cloud reads the rectified left image
    want_xyz, want_pix = pyref.point_cloud(want, rl, D, 1, *CAM)
    raw_bytes = open(prefix + "_cloud.bin", "rb").read()
    n = len(want_pix)
    assert len(raw_bytes) == n * 25
    xyz = np.frombuffer(raw_bytes[: n * 24], np.float64).reshape(n, 3)
    assert np.array_equal(xyz.view(np.uint64), want_xyz.view(np.uint64))
    assert np.array_equal(np.frombuffer(raw_bytes[n * 24:], np.uint8), want_pix)
