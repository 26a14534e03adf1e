"""The C++ class surface's input resize (include/sgm_amd/SGM.h): set_input_size,
process() on camera-size Mats, resize() and get_resized() compile with g++
against the C-ABI library and -- on the GPU -- give the map the Python pipeline
computes on recipe(raw) (tests/resize_recipe.py) and the recipe's images."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import resize_recipe as rr
import support
from stereo_matching_amd import SGM, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sgm_resize_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_bad_sizes_and_wrong_size_images_are_refused(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 4, r.stdout + r.stderr


@pytest.mark.gpu
def test_input_size_class_matches_the_python_pipeline(exe, tmp_path):
    (sh, sw), (h, w, D) = (37, 53), (24, 80, 32)
    left, right = synthetic.stereo_pair(sh, sw, D, pair_index=5, kind="road")
    rl, rright = rr.resize(left, h, w), rr.resize(right, h, w)
    with SGM(h, w, 1, D, post_filter=True) as sgm:
        sgm.process(rl, rright)
        want = sgm.get_disp()
    fl, fr, fo = (str(tmp_path / n) for n in ("l.raw", "r.raw", "out"))
    left.tofile(fl)
    right.tofile(fr)
    r = subprocess.run([exe, "run", fl, fr, str(sh), str(sw), str(h), str(w), str(D), fo],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"resized {h} {w} and {h} {w}" in r.stdout, r.stdout
    got = np.fromfile(fo + ".disp", dtype=np.float32).reshape(h, w)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.fromfile(fo + ".left", np.uint8).reshape(h, w), rl)
    assert np.array_equal(np.fromfile(fo + ".right", np.uint8).reshape(h, w), rright)
