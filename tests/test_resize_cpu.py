"""CPU checks of the input resize's pinned definition (tests/resize_recipe.py,
DESIGN.md 5j): the worked case, the identity, the half-size path, constants and
monotone ramps; the header, the binding and the build list name the feature."""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np
import pytest

import resize_recipe as rr
import support
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_worked_case_1x2_to_1x4():
    s, a0, a1 = rr.coefficients(4, 2)
    assert s.tolist() == [0, 0, 0, 1]                 # dx = 0 clamps low, dx = 3 clamps high
    assert a0.tolist() == [2048, 1536, 512, 2048] and a1.tolist() == [0, 512, 1536, 0]
    assert 0 * 1536 + 255 * 512 == 130560 and (2048 * (130560 >> 4)) >> 16 == 255
    got = rr.resize(np.array([[0, 255]], np.uint8), 1, 4)
    assert got.tolist() == [[0, 64, 191, 255]]


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (24, 80), (37, 53)])
def test_equal_sizes_are_the_identity(h, w):
    img = rr.random_image(h, w, 1)
    assert np.array_equal(rr.resize(img, h, w), img)


def test_exact_half_is_the_2x2_mean():
    img = rr.random_image(48, 160, 2)
    want = np.empty((24, 80), np.uint8)
    for i in range(24):
        for j in range(80):
            blk = img[2 * i: 2 * i + 2, 2 * j: 2 * j + 2].astype(int)
            want[i, j] = (blk.sum() + 2) >> 2
    assert np.array_equal(rr.resize(img, 24, 80), want)
    # half in one axis only is the general path: columns are sampled, not averaged
    one_axis = rr.resize(img, 48, 80)
    assert not np.array_equal(one_axis[::2], want)


RATIOS = [Fraction(3, 2), Fraction(2, 3), Fraction(7, 3), Fraction(1, 5), Fraction(8)]


@pytest.mark.parametrize("ry", RATIOS)
@pytest.mark.parametrize("rx", RATIOS)
@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_a_constant_image_stays_constant(rx, ry, value):
    sh, sw = 30, 45                                   # multiples of 3 and 5: every ratio is exact
    dh, dw = int(sh * ry), int(sw * rx)
    got = rr.resize(np.full((sh, sw), value, np.uint8), dh, dw)
    assert got.shape == (dh, dw) and (got == value).all()


@pytest.mark.parametrize("sw,dw", [(2, 4), (16, 24), (53, 80), (64, 512), (100, 233)])
def test_upscaled_ramp_is_monotone(sw, dw):
    ramp = np.round(np.linspace(0, 255, sw)).astype(np.uint8)
    got = rr.resize(np.tile(ramp, (3, 1)), 3, dw).astype(int)
    assert (np.diff(got, axis=1) >= 0).all()
    assert got[0, 0] == 0 and got[0, -1] == 255


def test_more_than_2x_down_skips_pixels():
    # 1 x 10 -> 1 x 2: fx = 2.0 and 7.0, so the taps are columns 2 and 7 alone; a spike elsewhere is not seen
    img = np.zeros((1, 10), np.uint8)
    img[0, 0] = img[0, 5] = 255
    assert rr.resize(img, 1, 2).tolist() == [[0, 0]]


def test_header_binding_and_build_list_carry_the_feature():
    header = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    for name in ("sgm_resize_device", "sgm_stage_resize", "sgm_set_input_size", "sgm_get_input_size",
                 "sgm_get_resized"):
        assert name + "(" in header and name in _capi.EXPORTS
    assert "#define SGM_HIP_VERSION 2 " in header     # the struct and the version stay
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    assert "sgm_resize.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]


def test_host_side_checks_run_clean_under_sanitizers(tmp_path):
    # the size checks and scale factors (csrc/sgm_resize_args.h) as a stand-alone CPU program
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "resize_args_main.cpp"))
    r = support.run(exe)
    assert r.returncode == 0 and "resize args ok" in r.stdout, r.stdout + r.stderr
