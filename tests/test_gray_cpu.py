"""CPU checks of the colour input's pinned grey conversion (tests/gray_recipe.py,
DESIGN.md 5l): the worked values, the identity on grey pixels, the channel
orders, the ignored alpha, the distance to the real-valued weights; the header,
the binding and the build list name the feature; the host-side checks run under
sanitizers as a stand-alone program."""
from __future__ import annotations

import os

import numpy as np
import pytest

import gray_recipe as gr
import support
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def px(r, g, b, fmt):
    p = {"rgb8": [r, g, b], "bgr8": [b, g, r], "rgba8": [r, g, b, 9], "bgra8": [b, g, r, 9]}[fmt]
    return np.array([[p]], np.uint8)


@pytest.mark.parametrize("fmt", gr.FORMATS)
def test_worked_values(fmt):
    assert gr.gray(px(255, 0, 0, fmt), fmt)[0, 0] == 76
    assert gr.gray(px(0, 255, 0, fmt), fmt)[0, 0] == 150
    assert gr.gray(px(0, 0, 255, fmt), fmt)[0, 0] == 29
    assert 4899 + 9617 + 1868 == 16384


@pytest.mark.parametrize("fmt", gr.FORMATS)
def test_grey_pixels_keep_their_value(fmt):
    v = np.arange(256, dtype=np.uint8).reshape(1, 256)
    assert np.array_equal(gr.gray(gr.from_gray(v, fmt), fmt), v)


def test_channel_orders_mirror_each_other():
    x = gr.random_image(9, 31, 3, 1)
    assert np.array_equal(gr.gray(x, "bgr8"), gr.gray(np.ascontiguousarray(x[..., ::-1]), "rgb8"))
    assert not np.array_equal(gr.gray(x, "bgr8"), gr.gray(x, "rgb8"))


@pytest.mark.parametrize("fmt4,fmt3", [("bgra8", "bgr8"), ("rgba8", "rgb8")])
def test_alpha_is_ignored(fmt4, fmt3):
    x = gr.random_image(9, 31, 4, 2)
    want = gr.gray(np.ascontiguousarray(x[..., :3]), fmt3)
    for alpha in (0, 1, 255):
        y = x.copy()
        y[..., 3] = alpha
        assert np.array_equal(gr.gray(y, fmt4), want)


def test_within_rounding_of_the_real_weights_over_the_lattice():
    # each 14-bit coefficient is within 1 / 16384 of its real weight, so the weighted sum is within
    # 3 * 255 / 16384 of the real one, and the final rounding adds at most 0.5
    v = np.arange(0, 256, 17)
    r, g, b = (a.ravel() for a in np.meshgrid(v, v, v, indexing="ij"))
    assert r.size == 16 ** 3
    img = np.stack([r, g, b], axis=1).astype(np.uint8)[None]
    y = gr.gray(img, "rgb8")[0].astype(np.float64)
    err = np.abs(y - (0.299 * r + 0.587 * g + 0.114 * b))
    assert err.max() <= 0.5 + 3 * 255 / 16384, err.max()
    assert y.min() >= 0 and y.max() <= 255


def test_bytes_per_pixel_agree_with_the_binding():
    for name, code in _capi.PIX_FORMATS.items():
        assert gr.bytes_per_pixel(name) == _capi.PIX_BYTES[code]
    assert _capi.PIX_FORMATS == {"gray8": 0, "bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4}


def test_header_binding_and_build_list_carry_the_feature():
    header = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    for name in ("sgm_set_input_format", "sgm_get_input_format", "sgm_gray_device", "sgm_stage_gray",
                 "sgm_get_input_gray", "sgm_stage_input_gray"):
        assert name + "(" in header and name in _capi.EXPORTS
    for k, name in enumerate(("SGM_PIX_GRAY8", "SGM_PIX_BGR8", "SGM_PIX_RGB8", "SGM_PIX_BGRA8", "SGM_PIX_RGBA8")):
        assert f"{name} = {k}" in header
    assert "#define SGM_HIP_VERSION 2 " in header     # the struct and the version stay
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    assert "sgm_gray.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]


def test_host_side_checks_run_clean_under_sanitizers(tmp_path):
    # the format table and the pitch checks (csrc/sgm_gray_args.h) as a stand-alone CPU program
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "gray_args_main.cpp"))
    r = support.run(exe)
    assert r.returncode == 0 and "gray args ok" in r.stdout, r.stdout + r.stderr
