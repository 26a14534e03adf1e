"""The matching window's C++ side: the accept / refuse rule, the
divisions for every divisor 1 .. 9 and the staged-row index helpers
(csrc/sgm_window_cost_args.h) as a stand-alone program under sanitizers, and the
class surface (include/sgm_amd/SGM.h: set_window, get_window) compiled with g++
against the C-ABI library: its refusals throw, and a frame with a 5 x 5 window
equals the recipe."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np
import pytest

import window_recipe as wr
import support
from stereo_matching_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_window_surface.cpp")


def test_rule_divisions_and_indices_run_clean_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "window_args_main.cpp"),
                               fp_contract_off=True)
    r = support.run(exe, timeout=300)
    assert r.returncode == 0 and "window args ok" in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC, hip_headers=True)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_the_refusals_throw_and_change_nothing(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 7, r.stdout + r.stderr


@pytest.mark.gpu
def test_get_disp_with_a_5x5_window_equals_the_recipe(exe, tmp_path):
    h, w, D = 24, 80, 32
    left, right = synthetic.stereo_pair(h, w, D, pair_index=1, kind="road")
    req, res = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<5i", h, w, D, 5, 5))
        f.write(left.tobytes())
        f.write(right.tobytes())
    r = subprocess.run([exe, "frame", req, res], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(res, np.float32).reshape(h, w)
    wr.assert_bits_equal(got, wr.recipe(left, right, D, (5, 5))["final"], "get_disp")
