"""The handle's memory ledger (stereo_matching_amd/csrc/sgm_ledger.h) on the
CPU: sizes remembered per buffer, and the rollback of a group of allocations
under an allocator that fails at every position -- the setters' failure paths,
which running out of device memory cannot be asked to show.
tests/cpp/ledger_main.cpp holds the checks; it is built under ASan and UBSan
(no leak, no double free) and run directly."""
from __future__ import annotations

import os
import re

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_matching_amd", "csrc")


def test_ledger_and_group_rollback_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "ledger_main.cpp"))
    r = support.run(exe)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout) and not r.stderr, r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 20
    nested = support.run(exe, "nest")        # groups do not nest: the constructor's assert aborts
    assert nested.returncode == -6 and "!l.open" in nested.stderr, nested.stdout + nested.stderr


def test_the_ledger_header_is_host_pure_and_built_into_the_library():
    src = open(os.path.join(CSRC, "sgm_ledger.h")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()        # (comments may name hipMalloc)
    assert "sgm_ledger.h" in open(os.path.join(CSRC, "Makefile")).read()
    assert '#include "sgm_ledger.h"' in open(os.path.join(CSRC, "sgm_handle.h")).read()
