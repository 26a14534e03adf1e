"""The cost filters' C++ side: the class surface (include/sgm_amd/SGM.h:
set_volume_filter, volume_filter, filter_volume_device) compiled with g++
against the C-ABI library; its refusals throw, and a filtered aggregate_device
equals tests/volume_filter_recipe.py bit for bit."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_volume_filter_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC, hip_headers=True)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_filtered_aggregate_equals_the_recipe(exe, tmp_path):
    import oracle
    import volume_filter_recipe as fr
    oracle.build()
    h, w, D = 12, 37, 32
    C = fr.frame_volume(h, w, D)
    vol, maps = str(tmp_path / "volume.f32"), str(tmp_path / "maps.f32")
    np.ascontiguousarray(C).tofile(vol)
    r = subprocess.run([exe, "run", vol, maps, str(h), str(w), str(D)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 4, r.stdout + r.stderr
    got = np.fromfile(maps, np.float32).reshape(2, h, w)
    # (the class's handles run two views and end with post_filter, as SGM::process does)
    assert np.array_equal(fr.bits(got[0]), fr.bits(fr.expected(h, w, D)["final"]))
    # a caller-side filter of the left volume is the other order: the right view derived from it
    assert np.array_equal(fr.bits(got[1]), fr.bits(fr.caller_side(C)["final"]))
