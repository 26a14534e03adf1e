"""The C++ class surface's min_disp constructor (include/sgm_amd/SGM.h):
SGM(h, w, s, d, paths, min_disp) compiles with g++ against the C-ABI library,
refuses a bad min_disp before any device work, and -- on the GPU -- a two-view
frame with min_disp = 16 returns get_disp() bit-identical to the recipe's
post-filtered map (tests/min_disp_recipe.py) and reports invalid = D + 17."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import min_disp_recipe as md
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sgm_min_disp_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC)


def test_bad_min_disp_is_refused(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 3, r.stdout + r.stderr


@pytest.mark.gpu
def test_min_disp_class_matches_recipe(exe, tmp_path):
    shape = md.RECOVERY
    h, w, D, m, s, kind, sky = shape
    assert (h, w, D, m, s) == (37, 150, 32, 16, 1)
    left, right, _ = md.make_inputs(shape)
    fl, fr, fo = (str(tmp_path / n) for n in ("l.raw", "r.raw", "out.raw"))
    left.tofile(fl)
    right.tofile(fr)
    r = subprocess.run([exe, "run", fl, fr, str(h), str(w), str(D), str(m), fo],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"invalid {D + 17} min_disp {m}" in r.stdout, r.stdout
    got = np.fromfile(fo, dtype=np.float32).reshape(h, w)
    md.assert_bits_equal(got, md.expected(shape)["final"], "get_disp()")
