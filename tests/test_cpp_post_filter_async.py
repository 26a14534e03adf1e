"""The median fill's launch budget through the C++ class surface:
sgm_amd::SGM::set_post_filter_launches and BatchSGM's constructor argument
(include/sgm_amd/SGM.h, BatchSGM.h) compile with g++ against the C-ABI library
and return get_disp() bit-identical to the oracle's SGM::process."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import support
from stereo_matching_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "post_filter_async.cpp")

H, W, D = 72, 200, 64
# ceil(W / 64) * H + 1 fill launches always prove the fixed point (DESIGN.md "Post filter")
BUDGET = -(-W // 64) * H + 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC, hip_headers=True, pthread=True)


def test_program_compiles_against_the_headers(exe):
    # the usage error path runs without a device
    assert subprocess.run([exe], capture_output=True).returncode == 64


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    import oracle
    oracle.build()
    prefix = str(tmp_path_factory.mktemp("pairs") / "pair")
    want = []
    for k in range(2):
        left, right = synthetic.stereo_pair(H, W, D, pair_index=70 + k, kind=("noise" if k else "road"))
        left.tofile(f"{prefix}_l{k}.raw")
        right.tofile(f"{prefix}_r{k}.raw")
        want.append(oracle.process(left, right, D)["final"])
    return prefix, want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["run", "batch"])
def test_budgeted_frames_match_oracle(exe, pairs, tmp_path, mode):
    prefix, want = pairs
    fo = str(tmp_path / "out.raw")
    r = subprocess.run([exe, mode, prefix, "2", str(H), str(W), str(D), str(BUDGET), fo],
                       capture_output=True, text=True, timeout=120,
                       env={**os.environ, "SGM_AMD_DEVICES": "0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"with a budget of {BUDGET}" in r.stdout
    if mode == "run":
        assert r.stdout.count("refused") == 2
    got = np.fromfile(fo, dtype=np.float32).reshape(2, H, W)
    for k in range(2):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
