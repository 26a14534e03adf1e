"""The C++ class surface's hole filling (include/sgm_amd/SGM.h, GPU_SGM.h):
set_fill(mode); process(l, r); get_disp(); get_fill_mask() compiles with g++
against the C-ABI library and -- on the GPU -- returns the filled map and the
fill mask, equal bit for bit to the recipe (tests/fill_recipe.py) applied to
the same pair's unfilled map; BM refuses the interpolate mode."""
from __future__ import annotations

import os

import numpy as np
import pytest

import fill_recipe
import support
from support import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sgm_fill_surface.cpp")
H, W, D = 48, 96, 32
MODES = {"background": 1, "interpolate": 2}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SRC)


def test_surface_compiles(exe):
    assert os.access(exe, os.X_OK)


@pytest.mark.gpu
def test_bm_refuses_interpolate(exe):
    r = support.run(exe, "refuse", timeout=120)
    assert r.returncode == 0 and "threw as expected" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode", [("sgm", "interpolate"), ("sgm", "background"), ("bm", "background"),
                                       ("gpu_sgm", "background")])
def test_filled_map_and_mask_equal_the_recipe(exe, tmp_path, kind, mode):
    from stereo_matching_amd import BM, GPU_SGM, SGM, synthetic
    left, right = synthetic.stereo_pair(H, W, D, pair_index=3)
    make = {"sgm": lambda: SGM(H, W, 1, D, post_filter=True), "bm": lambda: BM(H, W, 1, D),
            "gpu_sgm": lambda: GPU_SGM(H, W, 1, D)}[kind]
    with make() as off, SGM(H, W, 1, D, views=1, view="right") as rv:
        off.process(left, right)
        rv.process(left, right)
        want, wmask = fill_recipe.fill(off.get_disp(), D, 0, 1, rv.get_lr_disp(), mode, 1.0)
    assert (wmask != 0).any()
    fl, fr, fo, fm = (str(tmp_path / n) for n in ("l.raw", "r.raw", "disp.raw", "mask.raw"))
    left.tofile(fl)
    right.tofile(fr)
    r = support.run(exe, "run", kind, fl, fr, H, W, D, MODES[mode], fo, fm, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fo, dtype=np.float32).reshape(H, W)
    mask = np.fromfile(fm, dtype=np.uint8).reshape(H, W)
    assert np.array_equal(mask, wmask)
    assert np.array_equal(bits(got), bits(want))
