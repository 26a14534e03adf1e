"""The window costs' C++ side: the two divisions, the staged-column index and
the argument checks (csrc/sgm_window_cost_args.h) as a stand-alone program under
sanitizers, and the class surface (include/sgm_amd/SGM.h: set_cost, cost,
window_cost_device) compiled with g++ against the C-ABI library, whose refusals
throw."""
from __future__ import annotations

import os
import subprocess

import pytest

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_window_cost_surface.cpp")


def test_divisions_and_indices_run_clean_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "window_cost_args_main.cpp"),
                               fp_contract_off=True)
    r = support.run(exe, timeout=120)
    assert r.returncode == 0 and "window cost args ok" in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC, hip_headers=True)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_the_refusals_throw_and_a_frame_runs(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 7, r.stdout + r.stderr
