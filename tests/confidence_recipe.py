"""Expected match-confidence maps (sgm_set_confidence), composed from the
oracle's stage functions.

ratio = min_cost / sec_min_cost, the uniqueness test's own quotient
(SGM.cpp:392-409): min_cost = min_d S, sec_min_cost the smallest S != min_cost,
or FLT_MAX (SGM.cpp:399's initial value) where every cost of a pixel is equal;
one numpy float32 division.  S is paths4_recipe.aggregate's volume (the
reference's association order, 8 or 4 paths); tests/test_confidence_cpu.py
ties the quotient to oracle.wta's invalidations.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools

import numpy as np

from paths4_recipe import (IDS, SHAPES, aggregate, assert_bits_equal, census, cost_volume,  # noqa: F401
                           make_inputs, masks)
from stereo_matching_amd import synthetic

FLT_MAX = np.float32(np.finfo(np.float32).max)

# the schedule tests' frames (tests/test_gpu_schedules.py's two small masked
# shapes): (h, w, D), scale 1, road pair 5, the same sky mask for both views
SCHEDULE_SHAPES = [(96, 260, 128), (80, 240, 256)]


def min_sec(S):
    """(m, sec) of an aggregated volume: float32 rows x cols each."""
    assert S.dtype == np.float32
    m = S.min(-1)
    sec = np.where(S != m[..., None], S, FLT_MAX).min(-1)
    return m, sec


def ratio_of(S):
    m, sec = min_sec(S)
    r = m / sec
    assert r.dtype == np.float32
    return r


def view_volumes(left, right, D, s, sky, paths, P1=10, P2=100, sky_l=None, sky_r=None):
    """The aggregated volumes (S_left, S_right) of a pair; the sky mask `sky` serves both
    views unless sky_l / sky_r give a view its own."""
    ctl, ctr = census(left, s), census(right, s)
    return tuple(aggregate(cost_volume(ctl, ctr, D, s, v, mask), paths, P1, P2)
                 for v, mask in enumerate(masks(sky, sky_l, sky_r)))


def _frozen(arrs):
    for a in arrs:
        a.setflags(write=False)
    return tuple(arrs)


@functools.lru_cache(maxsize=None)
def volumes(shape, paths=8):
    """(S_left, S_right) of a SHAPES entry, computed once per session; read-only."""
    h, w, D, s, kind, sky = shape
    left, right, mask = make_inputs(*shape)
    return _frozen(view_volumes(left, right, D, s, mask, paths))


@functools.lru_cache(maxsize=None)
def expected(shape, paths=8):
    """(ratio_left, ratio_right) of a SHAPES entry; read-only."""
    return _frozen([ratio_of(S) for S in volumes(shape, paths)])


def schedule_inputs(h, w, D):
    left, right = synthetic.stereo_pair(h, w, D, pair_index=5, kind="road")
    return left, right, synthetic.sky_mask(h, w)


@functools.lru_cache(maxsize=None)
def schedule_expected(h, w, D):
    """(ratio_left, ratio_right) of a SCHEDULE_SHAPES frame, 8 paths; read-only."""
    left, right, mask = schedule_inputs(h, w, D)
    return _frozen([ratio_of(S) for S in view_volumes(left, right, D, 1, mask, 8)])
