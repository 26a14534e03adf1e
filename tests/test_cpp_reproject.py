"""The reprojection's C++ side: the class surface (include/sgm_amd/SGM.h:
set_reproject, clear_reproject, reproject(), xyz(), depth(), depth16(), the Mat
shim's CV_32FC3 and CV_16UC1) compiles with g++ against the C-ABI library and --
on the GPU -- gives the recipe's products (tests/reproject_recipe.py) of the map
the oracle computes."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import reproject_recipe as rp
import support
from stereo_matching_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_reproject_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_the_refusals_throw(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 11, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("q", ["camera_q", "skewed"])
def test_class_products_equal_the_recipe_on_the_oracles_map(exe, tmp_path, q):
    import oracle
    oracle.build()
    h, w, D = 24, 80, 32
    left, right = synthetic.stereo_pair(h, w, D, pair_index=0, kind="road")
    ref = oracle.process(left, right, D, views=2)["final"]
    invalid = float((ref == np.float32(D + 1)).mean())
    assert invalid >= 0.05 and 1.0 - invalid >= 0.50
    qv = rp.camera_q(700.5, 699.25, 31.5, 8.25, 0.12) if q == "camera_q" else rp.skewed_q()
    free = rp.reproject(ref, qv, D + 1)
    mr = float(np.float32(np.median(free["depth"][~free["missing"]])))
    want = rp.reproject(ref, qv, D + 1, 1, mr, 1000.0)
    assert (want["missing"] & ~free["missing"]).any() and (~want["missing"]).any()
    fl, fr, fq, fo = (str(tmp_path / n) for n in ("l.raw", "r.raw", "q.f64", "out"))
    left.tofile(fl)
    right.tofile(fr)
    qv.tofile(fq)
    r = subprocess.run([exe, "run", fl, fr, str(h), str(w), str(D), fq, repr(mr), fo],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"xyz {h} {w} x 3 type 21, depth16 type 2" in r.stdout, r.stdout
    got = np.fromfile(fo + ".disp", dtype=np.float32).reshape(h, w)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(np.fromfile(fo + ".xyz", np.uint32).reshape(h, w, 3), rp.bits(want["xyz"]))
    assert np.array_equal(np.fromfile(fo + ".depth", np.uint32).reshape(h, w), rp.bits(want["depth"]))
    assert np.array_equal(np.fromfile(fo + ".depth2", np.uint32).reshape(h, w), rp.bits(want["depth"]))
    assert np.array_equal(np.fromfile(fo + ".depth16", np.uint16).reshape(h, w), want["depth16"])
