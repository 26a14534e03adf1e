"""The caller's cost volume's C++ side: the host-side stride rule
(csrc/sgm_volume_args.h) as a stand-alone program under sanitizers, and the
class surface (include/sgm_amd/SGM.h: aggregate_device, import_volume_device)
compiled with g++ against the C-ABI library, whose refusals throw."""
from __future__ import annotations

import os
import subprocess

import pytest

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_volume_surface.cpp")


def test_stride_rule_runs_clean_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "volume_args_main.cpp"))
    r = support.run(exe)
    assert r.returncode == 0 and "volume args ok" in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC, hip_headers=True)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_the_refusals_throw(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 11, r.stdout + r.stderr
