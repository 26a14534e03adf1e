"""The CT cost's class surface (include/sgm_amd/SGM.h: set_cost, cost,
window_cost_device with SGM_COST_CT) compiled with g++ against the C-ABI
library: kind 3 still throws, a constant pair gives an all-zero volume, a frame
on the cost runs."""
from __future__ import annotations

import os
import subprocess

import pytest

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_ct_cost_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC, hip_headers=True)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_kind_3_throws_a_constant_pair_is_zero_and_a_frame_runs(exe):
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 5, r.stdout + r.stderr
    assert "cost[0] = 0" in r.stdout
