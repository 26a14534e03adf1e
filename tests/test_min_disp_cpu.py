"""The min_disp recipe (tests/min_disp_recipe.py) pinned on the CPU: with m = 0
it is oracle.process, its shifted-table cost volumes are the definition's
formulas computed directly, and the map it defines finds the disparities that
lie inside the window.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import min_disp_recipe as md
import oracle


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(-1)


def _direct_dsi(ctl, ctr, D, m, s, view):
    """Step 2 of the definition, no shifted tables:
    left  C[i, j, d] = ham(ctL[i, j], ctR[i, max(j - (d + m)/s, 0)])
    right C[i, j, d] = ham(ctL[i, min(j + (d + m)/s, W-1)], ctR[i, j])"""
    H, W = ctl.shape
    j = np.arange(W)
    out = np.empty((H, W, D), np.float32)
    for d in range(D):
        k = (d + m) // s
        if view == 0:
            out[:, :, d] = _popcount(ctl ^ ctr[:, np.maximum(j - k, 0)])
        else:
            out[:, :, d] = _popcount(ctl[:, np.minimum(j + k, W - 1)] ^ ctr)
    return out


@pytest.mark.parametrize("shape", md.SHAPES + md.STRIP_SHAPES[:1], ids=md.IDS + md.STRIP_IDS[:1])
def test_shifted_tables_give_the_defined_dsi(shape):
    h, w, D, m, s, kind, sky = shape
    left, right, _ = md.make_inputs(shape)
    ctl, ctr = md.census(left, s), md.census(right, s)
    ctl_s, ctr_s = md.shift_tables(ctl, ctr, m // s)
    md.assert_bits_equal(oracle.dsi(ctl, ctr_s, D, s, 0), _direct_dsi(ctl, ctr, D, m, s, 0), "left DSI")
    md.assert_bits_equal(oracle.dsi(ctl_s, ctr, D, s, 1), _direct_dsi(ctl, ctr, D, m, s, 1), "right DSI")


@pytest.mark.parametrize("shape", [md.SHAPES[1], md.SHAPES[3], md.SHAPES[4]],
                         ids=[md.IDS[1], md.IDS[3], md.IDS[4]])
def test_recipe_without_min_disp_is_oracle_process(shape):
    h, w, D, m, s, kind, sky = shape
    left, right, mask = md.make_inputs(shape)
    got = md.recipe(left, right, D, 0, s, mask)
    ref = oracle.process(left, right, D, s, mask, mask)
    for key in ("disp", "disp_beta", "sub", "sub_beta", "lr", "final"):
        md.assert_bits_equal(got[key], ref[key], key)


def test_invalid_marker_and_sky():
    shape = md.SHAPES[4]
    h, w, D, m, s, kind, sky = shape
    want = md.expected(shape)
    _, _, mask = md.make_inputs(shape)
    for key in ("sub", "sub_beta", "lr", "final"):
        a = want[key]
        assert ((a <= D + m - 1) | (a == D + m + 1)).all(), key
        assert a.min() >= m, key
    # the sky override stays in index space: a sky pixel wins index 0 = disparity m
    assert (want["disp"][mask == 255] == m).all()
    assert (want["sub"][mask == 255] == np.float32(m)).all()


def test_recovery():
    """Rows of the (37, 150) road pair (generated for 64 disparities) whose
    ground truth lies in [16, 48): at least half of their pixels survive the
    LR check and the median error of those is at most 2."""
    frac, med = md.recovery_figures(md.expected(md.RECOVERY)["lr"])
    print(f"valid fraction {frac:.3f}, median |lr - gt| {med:.3f}")
    assert frac >= 0.5
    assert med <= 2.0


def test_the_setter_is_declared_and_the_struct_is_unchanged():
    """min_disp is a property of the handle: sgm_params keeps its fields."""
    import ctypes
    import os
    import re

    from stereo_matching_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sgm_hip.h")).read()
    assert re.search(r"^int sgm_set_min_disp\(sgm_handle \*h, int m\);", text, re.M)
    assert re.search(r"^int sgm_get_invalid_disp\(const sgm_handle \*h, int \*invalid\);", text, re.M)
    body = text[text.index("typedef struct sgm_params {"):text.index("} sgm_params;")]
    assert "min_disp" not in body
    assert not hasattr(_capi.Params, "min_disp")
    lib = _capi.lib()
    assert lib.sgm_set_min_disp.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.sgm_set_min_disp(None, 16) == _capi.SGM_ERR_INVALID_ARG
    assert lib.sgm_get_invalid_disp(None, None) == _capi.SGM_ERR_INVALID_ARG
