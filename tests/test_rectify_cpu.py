"""CPU checks of the rectification remap's pinned definition
(tests/rectify_recipe.py) against hand-computed values: the
identity, an integer shift, the largest fractions, every border, the rounding
ties and the non-finite coordinates; the header, the binding and the build list
name the feature."""
from __future__ import annotations

import os

import numpy as np
import pytest

import rectify_recipe as rc
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(src, x, y):
    """The remap of one destination pixel sampling (x, y)."""
    return int(rc.remap(np.asarray(src, np.uint8), np.array([[x]], np.float32), np.array([[y]], np.float32))[0, 0])


def valid(shape, x, y):
    return int(rc.convert(np.array([[x]], np.float32), np.array([[y]], np.float32), *shape)[4][0, 0])


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (24, 80), (37, 53)])
def test_the_identity_map_returns_the_source(h, w):
    img = rc.random_image(h, w, 1)
    mx, my = rc.identity_maps(h, w)
    assert np.array_equal(rc.remap(img, mx, my), img)
    # the last row and column have their second taps outside the source: not valid
    want = np.zeros((h, w), np.uint8)
    want[: h - 1, : w - 1] = 255
    assert np.array_equal(rc.convert(mx, my, h, w)[4], want)


def test_an_integer_shift_moves_the_image_and_fills_with_zero():
    img = rc.random_image(9, 14, 2)
    mx, my = rc.identity_maps(9, 14)
    got = rc.remap(img, mx + 3, my - 2)             # dst(i, j) = src(i - 2, j + 3)
    want = np.zeros_like(img)
    want[2:, :11] = img[:7, 3:]
    assert np.array_equal(got, want)


def test_the_largest_fractions():
    src = [[10, 20], [30, 250]]
    # a = 31, b = 0: (1 * 32 * 10 + 31 * 32 * 20 + 512) >> 10
    assert (32 * 10 + 31 * 32 * 20 + 512) >> 10 == 20 and one(src, 31 / 32, 0) == 20
    # a = 0, b = 31: (32 * 1 * 10 + 32 * 31 * 30 + 512) >> 10
    assert (32 * 10 + 32 * 31 * 30 + 512) >> 10 == 29 and one(src, 0, 31 / 32) == 29
    # a = b = 31: (1 * 10 + 31 * 20 + 31 * 30 + 961 * 250 + 512) >> 10
    assert (10 + 31 * 20 + 31 * 30 + 961 * 250 + 512) >> 10 == 236 and one(src, 31 / 32, 31 / 32) == 236
    # a = b = 16: the plain mean, (256 * 310 + 512) >> 10
    assert one(src, 0.5, 0.5) == (256 * 310 + 512) >> 10 == 78
    assert one([[255, 255], [255, 255]], 0.3, 0.7) == 255       # the weights sum to 1024


def test_taps_straddling_each_border_count_the_outside_as_zero():
    src = np.full((4, 6), 200, np.uint8)
    # left: x0 = -1, a = 16: half of the pixel at column 0
    assert one(src, -0.5, 1) == (16 * 32 * 200 + 512) >> 10 == 100 and valid((4, 6), -0.5, 1) == 0
    # right: x0 = 5 (the last column), a = 16: its right neighbour is outside
    assert one(src, 5.5, 1) == 100 and valid((4, 6), 5.5, 1) == 0
    # top: y0 = -1, b = 8: a quarter
    assert one(src, 2, -0.75) == (32 * 8 * 200 + 512) >> 10 == 50 and valid((4, 6), 2, -0.75) == 0
    # bottom: y0 = 3 (the last row), b = 24
    assert one(src, 2, 3.75) == (32 * 8 * 200 + 512) >> 10 == 50 and valid((4, 6), 2, 3.75) == 0
    # a corner: one tap of four inside, weight 16 * 16
    assert one(src, -0.5, -0.5) == (256 * 200 + 512) >> 10 == 50
    # the last pixel itself is exact although not "valid": the zero taps have zero weight
    assert one(src, 5, 3) == 200 and valid((4, 6), 5, 3) == 0
    assert valid((4, 6), 4, 2) == 255 and valid((4, 6), 4.97, 2.97) == 255
    # wholly outside
    for x, y in ((-1, 1), (6, 1), (2, -1), (2, 4), (-7.3, 99)):
        assert one(src, x, y) == 0 and valid((4, 6), x, y) == 0


def test_rounding_ties_go_to_even():
    # x * 32 = k + 0.5: k even rounds down to k, k odd rounds up to k + 1
    ks = np.array([0, 1, 2, 3, 4, 5, 30, 31, 32, 33, 1000, 1001])
    q = rc.fix(((ks + 0.5) / 32).astype(np.float32))
    assert q.tolist() == [0, 2, 2, 4, 4, 6, 30, 32, 32, 34, 1000, 1002]
    q = rc.fix((-(ks + 0.5) / 32).astype(np.float32))
    assert q.tolist() == [0, -2, -2, -4, -4, -6, -30, -32, -32, -34, -1000, -1002]
    # the integer part floors, the fraction is what is left: -2/32 is (-1, 30)
    x0, _, a, _, _ = rc.convert(np.float32([[-1.5 / 32]]), np.float32([[0]]), 4, 4)
    assert (int(x0[0, 0]), int(a[0, 0])) == (-1, 30)
    src = [[100, 0], [0, 0]]
    assert one(src, 0.5 / 32, 0) == 100                       # q = 0: the pixel itself
    assert one(src, 1.5 / 32, 0) == (30 * 32 * 100 + 512) >> 10 == 94   # q = 2


@pytest.mark.parametrize("bad", rc.SPECIALS)
def test_non_finite_and_huge_coordinates_give_zero(bad):
    src = np.full((5, 5), 255, np.uint8)
    for x, y in ((bad, 2.0), (2.0, bad), (bad, bad)):
        assert one(src, x, y) == 0 and valid((5, 5), x, y) == 0
    q = int(rc.fix(np.float32(bad)))
    assert q == (rc.FIX_MAX if bad > 0 else rc.FIX_MIN)       # (NaN: the lower clamp)
    # the clamped integer parts lie outside every allowed source (at most 32767 wide)
    assert rc.FIX_MIN >> 5 == -32768 and rc.FIX_MAX >> 5 == 32767 and rc.FIX_MAX & 31 == 0
    big = np.full((1, 32767), 255, np.uint8)
    assert one(big, 32766, 0) == 255 and one(big, 32767, 0) == 0 and one(big, np.float32(bad), 0) == 0


def test_the_generator_samples_outside_on_every_side_and_differs_per_view():
    for shape in ((1, 1), (2, 3), (37, 53), (129, 200)):
        for h, w in ((24, 80), (17, 65)):
            l, r = rc.maps(h, w, *shape, 0), rc.maps(h, w, *shape, 1)
            assert not np.array_equal(l[0], r[0], equal_nan=True)
            for mx, my in (l, r):
                x0, y0, a, b, ok = rc.convert(mx, my, *shape)
                assert (x0[:, 0] < 0).any() and (x0[:, -1] + 1 >= shape[1]).any()
                assert (y0[0] < 0).any() and (y0[-1] + 1 >= shape[0]).any()
                assert np.isnan(mx).any() and np.isinf(my).any()
                assert (a[h // 2] == 0).all() and (b[:, w - 1 - w // 3] == 0).all()   # the integer row and column


def test_header_binding_and_build_list_carry_the_feature():
    header = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    for name in ("sgm_set_rectify", "sgm_get_rectify", "sgm_remap_device", "sgm_stage_remap",
                 "sgm_get_rectified", "sgm_stage_rectified", "sgm_stage_rectify_valid"):
        assert name + "(" in header and name in _capi.EXPORTS
    assert "#define SGM_HIP_VERSION 2 " in header     # the struct and the version stay
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    assert "sgm_rectify.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
