"""The occlusion-aware hole filling (Hirschmueller 2008, 2.6) in
numpy: what sgm_fill.hip must equal bit for bit.

F: the frame's final left map, rows x cols float32 in true disparity; R: the
right view's sub-pixel map.  inv = D + min_disp + 1; a pixel is valid iff
F <= D + min_disp - 1 (a NaN is invalid).  Every candidate comes from the input
map, so the result depends on no order:

  candidates  per direction the first valid pixel along the ray, if any
  class       mismatch iff some integer d in [min_disp, min_disp + D) has
              jr = j - d // scale >= 0, R[i, jr] valid and
              |R[i, jr] - float32(d)| <= lr_max_diff (one fp32 subtraction);
              else occlusion; mode "background": always occlusion
  value       occlusion: sorted[min(1, k - 1)]; mismatch: sorted[k // 2];
              k = 0: inv
  mask        0 measured, 1 occlusion, 2 mismatch, 3 still invalid
"""
from __future__ import annotations

import numpy as np

MEASURED, OCCLUSION, MISMATCH, INVALID = 0, 1, 2, 3
# (di, dj) of the 8 rays
DIRECTIONS = ((0, -1), (0, 1), (-1, 0), (-1, -1), (-1, 1), (1, 0), (1, 1), (1, -1))


def valid(F, D, min_disp=0):
    F = np.asarray(F, np.float32)
    with np.errstate(invalid="ignore"):
        return F <= np.float32(D + min_disp - 1)      # (NaN <= x is False)


def _shift(a, di, dj, fill):
    """out[i, j] = a[i + di, j + dj], `fill` where that is outside."""
    rows, cols = a.shape
    out = np.full_like(a, fill)
    i0, i1 = max(0, -di), min(rows, rows - di)
    j0, j1 = max(0, -dj), min(cols, cols - dj)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out


def candidates(F, D, min_disp=0):
    """8 x rows x cols float32: per direction the value of the first valid pixel
    along the ray from each pixel, +inf where the ray leaves the image first.
    A "last valid seen" propagation: the neighbour's value if valid, else the
    neighbour's own candidate, repeated until the longest ray is covered."""
    F = np.asarray(F, np.float32)
    ok = valid(F, D, min_disp)
    rows, cols = F.shape
    out = np.empty((8, rows, cols), np.float32)
    for n, (di, dj) in enumerate(DIRECTIONS):
        nb_ok = _shift(ok, di, dj, False)
        nb_val = _shift(F, di, dj, np.float32(np.inf))
        cand = np.full((rows, cols), np.inf, np.float32)
        for _ in range(max(rows, cols)):
            cand = np.where(nb_ok, nb_val, _shift(cand, di, dj, np.float32(np.inf)))
        out[n] = cand
    return out


def mismatch(R, D, min_disp=0, scale=1, lr_max_diff=1.0):
    """rows x cols bool: the class test at every pixel."""
    R = np.asarray(R, np.float32)
    rows, cols = R.shape
    r_ok = valid(R, D, min_disp)
    res = np.zeros((rows, cols), bool)
    j = np.arange(cols)
    tol = np.float32(lr_max_diff)
    for d in range(min_disp, min_disp + D):
        jr = j - d // scale
        sel = jr >= 0
        if not sel.any():
            break
        jc = jr[sel]
        with np.errstate(invalid="ignore", over="ignore"):
            hit = r_ok[:, jc] & (np.abs(R[:, jc] - np.float32(d)) <= tol)
        res[:, sel] |= hit
    return res


def pick(cand, mis, inv):
    """cand: 8 x ... candidates (+inf: none); mis: the class; -> (value, code) of
    invalid pixels."""
    c = np.sort(np.asarray(cand, np.float32), axis=0)
    k = np.isfinite(c).sum(axis=0)
    at = np.where(mis, k // 2, np.minimum(1, np.maximum(k - 1, 0)))
    val = np.take_along_axis(c, at[None], axis=0)[0]
    val = np.where(k == 0, np.float32(inv), val).astype(np.float32)
    code = np.where(k == 0, INVALID, np.where(mis, MISMATCH, OCCLUSION)).astype(np.uint8)
    return val, code


def fill(F, D, min_disp=0, scale=1, R=None, mode="interpolate", lr_max_diff=1.0):
    """(filled map, uint8 mask) of F."""
    if mode not in ("background", "interpolate"):
        raise ValueError(mode)
    F = np.ascontiguousarray(F, np.float32)
    ok = valid(F, D, min_disp)
    if mode == "interpolate":
        mis = mismatch(R, D, min_disp, scale, lr_max_diff)
    else:
        mis = np.zeros(F.shape, bool)
    val, code = pick(candidates(F, D, min_disp), mis, D + min_disp + 1)
    out = np.where(ok, F, val).astype(np.float32)
    mask = np.where(ok, MEASURED, code).astype(np.uint8)
    return out, mask
