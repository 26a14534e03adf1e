"""The pinned definition of the input resize (sgm_resize_device):
cv::resize(src, dst, Size(dw, dh)) of an 8-bit one-channel image with the
default INTER_LINEAR, in OpenCV's fixed-point form, restated in numpy
independently of the HIP code.

  * exact half size (sw == 2 dw and sh == 2 dh): dst = (a + b + c + d + 2) >> 2
    over each 2x2 block (OpenCV's switch to its area path);
  * otherwise scale_x = 1.0 / (double(dw) / double(sw)) (scale_y alike) and per
    destination column dx (rows alike):
        fx = float32((dx + 0.5) * scale_x - 0.5)   double, unfused, rounded once
        sx = floor(fx); fx -= sx                   float32
        sx < 0       -> sx = 0,      fx = 0
        sx >= sw - 1 -> sx = sw - 1, fx = 0
        a0 = sat_s16(rint((1 - fx) * 2048)), a1 = sat_s16(rint(fx * 2048))   ties to even
    Hrow(y, dx) = src(y, sx) * a0 + src(y, sx + 1) * a1 in int32 (no second term,
    and no read, where a1 == 0), and
        dst(dy, dx) = uint8((((b0 * (Hrow(sy) >> 4)) >> 16)
                             + ((b1 * (Hrow(min(sy + 1, sh - 1)) >> 4)) >> 16) + 2) >> 2)
    with arithmetic int32 shifts.

Parity with a particular OpenCV build is not pinned at this boundary (as for
the pre-blur): this text is the definition.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def coefficients(n_dst: int, n_src: int):
    """(s, c0, c1) per destination index of one axis: the source index and the
    two 11-bit weights."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    s[lo] = 0
    f[lo] = 0
    hi = s >= n_src - 1
    s[hi] = n_src - 1
    f[hi] = 0
    one, k = np.float32(1), np.float32(2048)
    c0 = np.clip(np.rint((one - f) * k), -32768, 32767).astype(np.int32)
    c1 = np.clip(np.rint(f * k), -32768, 32767).astype(np.int32)
    return s, c0, c1


def resize(src, dh: int, dw: int) -> np.ndarray:
    """cv::resize(src, dst, Size(dw, dh)) as pinned above."""
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    if sw == 2 * dw and sh == 2 * dh:
        q = src.astype(np.int32)
        return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = coefficients(dw, sw)
    sy, b0, b1 = coefficients(dh, sh)
    q = src.astype(np.int32)
    # (where a1 == 0 the neighbour is not read: its index is clamped for numpy's sake only)
    nb = np.where(a1 != 0, q[:, np.minimum(sx + 1, sw - 1)] * a1, 0)
    hrow = (q[:, sx] * a0 + nb).astype(np.int32)          # sh x dw
    r0 = hrow[sy] >> 4
    r1 = hrow[np.minimum(sy + 1, sh - 1)] >> 4
    v = (((b0[:, None] * r0) >> 16) + ((b1[:, None] * r1) >> 16) + 2) >> 2
    return v.astype(np.int32).astype(np.uint8)


def random_image(h: int, w: int, seed: int) -> np.ndarray:
    """Random u8 with forced runs of 0 and of 255 (the extremes of every sum)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img[:, : max(1, w // 7)] = 0
    img[:, w - max(1, w // 9):] = 255
    img[h // 2, :] = 255
    img[h // 3, w // 4: w // 2] = 0
    return img


def kitti_crop() -> np.ndarray:
    """The gray KITTI image (360 x 1240) of the sky detector's golden file."""
    with np.load(os.path.join(GOLDEN, "sky_000017_14.npz")) as z:
        return np.ascontiguousarray(z["image"])


def fit(img, h: int, w: int) -> np.ndarray:
    """img tiled to h x w (sources larger than the crop keep its texture)."""
    img = np.asarray(img, np.uint8)
    reps = (-(-h // img.shape[0]), -(-w // img.shape[1]))
    return np.ascontiguousarray(np.tile(img, reps)[:h, :w])
