"""The reprojection's pinned form in numpy, float64: the yardstick
of sgm_reproject_device and of the frame's output slot.

Q is 16 doubles, row-major.  For working-grid pixel (i, j) of a handle with
scale s: x = j * s, y = i * s, d = disp[i, j] (true disparity), and

    X' = ((q0 x + q1 y) + q2 d) + q3        Y' = ((q4 x + q5 y) + q6 d) + q7
    Z' = ((q8 x + q9 y) + q10 d) + q11      W' = ((q12 x + q13 y) + q14 d) + q15
    iW = 1.0 / W',  X = (float)(X' iW),  Y = (float)(Y' iW),  Z = (float)(Z' iW)

every operation one IEEE double operation in the order written (numpy's
elementwise float64 arithmetic fuses nothing), the conversions to float32 to
nearest.  A pixel is missing when disp == (float)invalid, or W' == 0, or
max_range > 0 and not (0 < Z <= max_range) on the rounded Z; xyz and depth then
hold the bit pattern 0x7FC00000, depth16 holds 0.  depth16 = rint(Z *
depth_scale) in float32 (ties to even) when that lies in [1, 65535], else 0.

Compare float products through bits(): the missing value is a NaN.
"""
from __future__ import annotations

import numpy as np

from support import bits  # noqa: F401  (re-exported: the reproject tests compare through rp.bits)

MISSING_BITS = 0x7FC00000
XYZ, DEPTH, DEPTH16 = 1, 2, 4
OUTPUT_BITS = {"xyz": XYZ, "depth": DEPTH, "depth16": DEPTH16}


def camera_q(fx, fy, cx, cy, baseline):
    """sgm_camera_q: the pinhole Q, 16 float64 values row-major (fx, fy, cx, cy
    are the camera's float32 fields)."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    q = np.zeros(16, np.float64)
    q[0] = 1.0
    q[3] = -cx
    q[5] = 1.0
    q[7] = -cy
    q[11] = (fx + fy) / 2
    q[14] = 1.0 / float(baseline)
    return q


def homogeneous(disp, q, scale=1):
    """X', Y', Z', W' (float64, rows x cols each) in the pinned association."""
    disp = np.asarray(disp, np.float32)
    q = np.asarray(q, np.float64).reshape(16)
    rows, cols = disp.shape
    x = (np.arange(cols, dtype=np.int64) * scale).astype(np.float64)[None, :]
    y = (np.arange(rows, dtype=np.int64) * scale).astype(np.float64)[:, None]
    d = disp.astype(np.float64)
    with np.errstate(all="ignore"):
        return tuple(((q[4 * r] * x + q[4 * r + 1] * y) + q[4 * r + 2] * d) + q[4 * r + 3] for r in range(4))


def reproject(disp, q, invalid, scale=1, max_range=0.0, depth_scale=1000.0):
    """{"xyz": rows x cols x 3 float32, "depth": rows x cols float32, "depth16":
    rows x cols uint16, "missing": rows x cols bool} of a working-grid map."""
    disp = np.asarray(disp, np.float32)
    xp, yp, zp, wp = homogeneous(disp, q, scale)
    w0 = wp == 0.0
    with np.errstate(all="ignore"):
        iw = 1.0 / np.where(w0, 1.0, wp)            # (a missing pixel's values are never used)
        X, Y, Z = ((v * iw).astype(np.float32) for v in (xp, yp, zp))
        missing = (disp == np.float32(invalid)) | w0
        mr = np.float32(max_range)
        if mr > 0:
            missing = missing | ~((Z > np.float32(0)) & (Z <= mr))
        r = np.rint(Z * np.float32(depth_scale))    # float32 x float32 -> float32, then ties to even
    assert r.dtype == np.float32
    fits = (r >= np.float32(1)) & (r <= np.float32(65535)) & ~missing
    depth16 = np.where(fits, np.clip(r, 0, 65535), 0).astype(np.uint16)
    xyz = np.stack([X, Y, Z], axis=2).view(np.uint32)
    xyz[missing] = MISSING_BITS
    depth = Z.view(np.uint32).copy()
    depth[missing] = MISSING_BITS
    return {"xyz": xyz.view(np.float32), "depth": depth.view(np.float32), "depth16": depth16, "missing": missing}


def skewed_q():
    """A Q with all sixteen entries non-zero whose W' keeps clear of 0 on small
    grids with disparities up to a few hundred."""
    return np.array([1.0, 0.013, -0.21, -317.5,
                     -0.007, 1.002, 0.033, -181.25,
                     0.0021, -0.0013, 0.011, 713.4,
                     0.00031, 0.00017, 1.9, 0.37], np.float64)


def hand_map(rows, cols, D, m, seed=0):
    """A hand-made true-disparity map of a handle with max_disp D and minimum
    disparity m: every map holds the invalid marker, 0.0, D - 1, fractional
    values and (under camera_q-like Qs) depths on both sides of a range test;
    the rest is uniform over [0, D + m)."""
    special = [float(D + m + 1), 0.0, float(D - 1), 0.5, float(D + m) - 0.25, 1.0, 3.75]
    assert rows * cols >= 2 * len(special)
    rng = np.random.default_rng(1000 * rows + cols + seed)
    a = (rng.random((rows, cols)) * (D + m)).astype(np.float32)
    flat = a.ravel()
    # (spread over the map, the first and the last pixel included)
    at = np.linspace(0, flat.size - 1, len(special)).astype(np.int64)
    flat[np.roll(at, seed)] = special
    return a
