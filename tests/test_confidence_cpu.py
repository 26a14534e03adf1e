"""The confidence recipe (tests/confidence_recipe.py) tied to the oracle: the
quotient it computes is the one oracle.wta's uniqueness test decides on
(SGM.cpp:392-409).  No GPU: this validates the GPU tests' expectation, not the
feature."""
from __future__ import annotations

import numpy as np
import pytest

import confidence_recipe as cr
import oracle

UNIQ = np.float32(0.7)


def _first_index(S, x):
    """First d with S[i, j, d] == x[i, j] (0 where none)."""
    return np.argmax(S == x[..., None], axis=-1)


def _invalid_by_ratio(S):
    m, sec = cr.min_sec(S)
    ratio = cr.ratio_of(S)
    return (ratio > UNIQ) & (np.abs(_first_index(S, m) - _first_index(S, sec)) > 1)


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("shape", cr.SHAPES, ids=cr.IDS)
def test_ratio_decides_the_oracles_invalidations(shape, paths):
    D = shape[2]
    for view, S in enumerate(cr.volumes(shape, paths)):
        ratio = cr.expected(shape, paths)[view]
        assert ratio.dtype == np.float32 and ratio.shape == S.shape[:2]
        if not shape[5]:
            # [0, 1) wherever the costs are non-negative; next to a sky mask's
            # 999999 override a path cost C + min(...) - minL_prev goes
            # negative, and the quotient leaves the range with it
            assert (ratio >= 0).all() and (ratio < 1).all(), (view, ratio.min(), ratio.max())
        invalid = oracle.wta(S) == D + 1
        assert np.array_equal(invalid, _invalid_by_ratio(S)), (view, int(invalid.sum()))


def test_all_equal_costs_divide_by_flt_max():
    shape = cr.SHAPES[1]
    D = shape[2]
    S = np.array(cr.volumes(shape, 8)[0], copy=True)
    S[0, :, :] = np.float32(123.0)      # a whole row of pixels without a second value
    S[5, 7, :] = np.float32(4.5e6)
    ratio = cr.ratio_of(S)
    assert np.array_equal(ratio[0].view(np.uint32),
                          np.full(S.shape[1], np.float32(123.0) / cr.FLT_MAX, np.float32).view(np.uint32))
    assert ratio[5, 7] == np.float32(4.5e6) / cr.FLT_MAX
    assert (ratio[0] > 0).all() and (ratio[0] < np.float32(1e-30)).all()
    # the oracle keeps those pixels (their quotient is far below 0.7) ...
    disp = oracle.wta(S)
    assert (disp[0] == 0).all() and disp[5, 7] == 0
    # ... and the rest of the map still follows the quotient
    assert np.array_equal(disp == D + 1, _invalid_by_ratio(S))
