"""The colour input's C++ side: the class surface (include/sgm_amd/SGM.h:
set_input_format, process() on CV_8UC3 and CV_8UC4 Mats, gray(), input_gray())
compiles with g++ against the C-ABI library and -- on the GPU -- gives the map
the oracle computes on recipe.gray(raw) (tests/gray_recipe.py)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import gray_recipe as gr
import support
from stereo_matching_amd import _capi, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE_SRC = os.path.join(ROOT, "tests", "cpp", "sgm_gray_surface.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return support.library_program(tmp_path_factory, SURFACE_SRC)


def test_surface_compiles_and_checks_its_arguments(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 64 and "usage" in r.stderr


@pytest.mark.gpu
def test_bad_formats_and_wrong_type_images_are_refused(exe):
    r = subprocess.run([exe, "bad"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("threw as expected") == 7, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", gr.FORMATS)
def test_colour_class_matches_the_oracle(exe, tmp_path, fmt):
    import oracle
    oracle.build()
    h, w, D = 24, 80, 32
    ch = gr.bytes_per_pixel(fmt)
    gl, gr_ = synthetic.stereo_pair(h, w, D, pair_index=5, kind="road")
    pair = []
    for k, g in enumerate((gl, gr_)):
        img = np.empty((h, w, ch), np.uint8)
        img[..., 0] = g
        img[..., 1] = g.astype(np.int64) * 3 // 4 + 17
        img[..., 2] = 255 - g
        if ch == 4:
            img[..., 3] = np.random.default_rng(k).integers(0, 256, (h, w), dtype=np.uint8)
        pair.append(img)
    yl, yr = gr.gray(pair[0], fmt), gr.gray(pair[1], fmt)
    want = oracle.process(yl, yr, D, views=2)["final"]
    fl, fr, fo = (str(tmp_path / n) for n in ("l.raw", "r.raw", "out"))
    pair[0].tofile(fl)
    pair[1].tofile(fr)
    r = subprocess.run([exe, "run", str(_capi.PIX_FORMATS[fmt]), fl, fr, str(h), str(w), str(D), fo],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"grey {h} {w} and {h} {w}" in r.stdout, r.stdout
    got = np.fromfile(fo + ".disp", dtype=np.float32).reshape(h, w)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.fromfile(fo + ".left", np.uint8).reshape(h, w), yl)
    assert np.array_equal(np.fromfile(fo + ".right", np.uint8).reshape(h, w), yr)
