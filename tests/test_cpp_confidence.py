"""The C++ class surface's match confidence (include/sgm_amd/SGM.h):
set_confidence(true); process(l, r); get_confidence() compiles with g++ against
the C-ABI library and -- on the GPU -- returns the left view's ratio map, equal
bit for bit to the C-ABI's (sgm_stage_confidence) and to the recipe
(tests/confidence_recipe.py); BM refuses it."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import confidence_recipe as cr
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sgm_confidence_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC)


def test_surface_compiles(exe):
    assert os.access(exe, os.X_OK)


@pytest.mark.gpu
def test_bm_refuses_confidence(exe):
    r = subprocess.run([exe, "bm"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "threw as expected" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_get_confidence_matches_capi_and_recipe(exe, tmp_path):
    shape = cr.SHAPES[1]
    h, w, D, s, kind, sky = shape
    assert (s, sky) == (1, False)       # process(l, r): no sky masks
    left, right, _ = cr.make_inputs(*shape)
    fl, fr, fo, fc = (str(tmp_path / n) for n in ("l.raw", "r.raw", "out.raw", "capi.raw"))
    left.tofile(fl)
    right.tofile(fr)
    r = subprocess.run([exe, "run", fl, fr, str(h), str(w), str(D), fo, fc],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fo, dtype=np.float32).reshape(h, w)
    capi = np.fromfile(fc, dtype=np.float32).reshape(h, w)
    cr.assert_bits_equal(got, capi, "get_confidence() vs the C-ABI map")
    cr.assert_bits_equal(got, cr.expected(shape, 8)[0], "get_confidence() vs the recipe")
