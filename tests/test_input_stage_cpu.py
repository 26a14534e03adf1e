"""The handle's input stage (csrc/sgm_input_stage.h, DESIGN.md "The input slot"): which launch
a frame begins with, the shape of the images it takes and whether the handle
stages them, checked against written-out values by a stand-alone CPU program
under sanitizers; the build list carries the new source file and header."""
from __future__ import annotations

import os

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_input_stage_runs_clean_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "input_stage_main.cpp"))
    r = support.run(exe)
    assert r.returncode == 0 and "input stage ok" in r.stdout, r.stdout + r.stderr


def test_build_list_carries_the_input_stage():
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    assert "sgm_input.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    rules = [line for line in mk.splitlines() if line.startswith("%.")]
    assert len(rules) == 2 and all("sgm_input_stage.h" in line for line in rules)
