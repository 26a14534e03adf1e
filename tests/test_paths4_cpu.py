"""The 4-path mode's CPU-side contract: the field in the ABI structs, and the
recipe the GPU tests compare against (tests/paths4_recipe.py).

The recipe composes oracle stage functions with S = ((L1+L2)+L3)+L4; run with
all eight paths it must equal oracle.process bit for bit, which pins the
composition (decimation, blur, census, DSI, filters, WTA, sub-pixel, LR check,
post_filter) independently of the path count."""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess

import pytest

import oracle
import paths4_recipe as p4
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_params_paths():
    # sgm_default_params: USE_8_PATH = true (inc/SGM.h:7)
    assert _capi.default_params(48, 96, 1, 32).paths == 8


def test_params_layout_matches_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "sgm_hip.h"\n'
                   'int main(void) { printf("%zu %zu %d\\n", sizeof(sgm_params), '
                   'offsetof(sgm_params, paths), SGM_HIP_VERSION); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off, version = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                 text=True).stdout.split())
    assert ctypes.sizeof(_capi.Params) == size
    assert _capi.Params.paths.offset == off
    # the last field
    assert off + ctypes.sizeof(ctypes.c_int) == size
    assert version == 2


@pytest.mark.parametrize("shape", [p4.SHAPES[2], p4.SHAPES[6]], ids=[p4.IDS[2], p4.IDS[6]])
def test_recipe_with_eight_paths_is_oracle_process(shape):
    h, w, D, s, kind, sky = shape
    assert (h, w, D, s) in ((37, 75, 32, 1), (96, 300, 64, 2))
    left, right, mask = p4.make_inputs(*shape)
    want = oracle.process(left, right, D, s, mask, mask)
    got = p4.recipe(left, right, D, s, mask, paths=8)
    for key in ("disp", "sub", "disp_beta", "sub_beta", "lr", "final"):
        p4.assert_bits_equal(got[key], want[key], key)
    # and the 4-path maps are other maps (a 4-path result cannot pass by accident)
    four = p4.expected(shape)
    assert (p4.bits(four["lr"]) != p4.bits(want["lr"])).mean() > 0.2
