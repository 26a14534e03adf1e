"""The C++ class surface's 4-path constructor (include/sgm_amd/SGM.h):
SGM(h, w, s, d, paths) compiles with g++ against the C-ABI library, refuses a
path count other than 4 or 8, and -- on the GPU -- SGM(h, w, 1, 64, 4) returns
get_disp() bit-identical to the 4-path recipe's post-filtered map
(tests/paths4_recipe.py)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import paths4_recipe as p4
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sgm_paths4_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC)


def test_other_path_counts_are_refused(exe):
    r = subprocess.run([exe, "badpaths"], capture_output=True, text=True)
    assert r.returncode == 0 and "threw as expected" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_four_path_class_matches_recipe(exe, tmp_path):
    shape = p4.SHAPES[3]
    h, w, D, s, kind, sky = shape
    assert (h, w, D, s) == (48, 150, 64, 1)
    left, right, _ = p4.make_inputs(*shape)
    fl, fr, fo = (str(tmp_path / n) for n in ("l.raw", "r.raw", "out.raw"))
    left.tofile(fl)
    right.tofile(fr)
    r = subprocess.run([exe, "run", fl, fr, str(h), str(w), str(D), fo],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fo, dtype=np.float32).reshape(h, w)
    want = p4.recipe(left, right, D, 1, None, paths=4)["final"]   # process(l, r): no sky masks
    p4.assert_bits_equal(got, want, "get_disp()")
