"""The weighted windows' host side (csrc/sgm_window_cost_args.h):
the weight table, the census's disc, the refusal rule and the weighted producer's
indices as a stand-alone program under sanitizers."""
from __future__ import annotations

import os

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_mask_rule_and_indices_run_clean_under_sanitizers(tmp_path):
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "weighted_args_main.cpp"),
                               fp_contract_off=True)
    r = support.run(exe, timeout=300)
    assert r.returncode == 0 and "weighted args ok" in r.stdout, r.stdout + r.stderr
