"""The pinned definition of the rectification remap (sgm_set_rectify /
sgm_remap_device): cv::convertMaps followed by cv::remap for
8-bit, one channel, INTER_LINEAR, BORDER_CONSTANT value 0, in OpenCV's
fixed-point form (5 fraction bits, 15 coefficient bits), restated in numpy
independently of the HIP code.

  * per coordinate c of a float32 map: t = c * 32 in float32 (exact); a NaN t
    becomes -32768 * 32; t is clamped to [-32768 * 32, 32767 * 32];
    q = rint(t), ties to even; the integer part is q >> 5 (it floors), the
    fraction q & 31;
  * with (x0, y0) the integer parts and a, b the fractions of x and y, and
    S(y, x) the source pixel or 0 outside the source (each tap on its own):
        dst = ((32-a)*(32-b)*S(y0,x0) + a*(32-b)*S(y0,x0+1)
             + (32-a)*b*S(y0+1,x0)    + a*b*S(y0+1,x0+1) + 512) >> 10
    (OpenCV's (sum w*S + (1 << 14)) >> 15 with its table weights w = 32 x these
    products, which sum to 1024: no weight correction, int32 holds the sum);
  * valid = 255 where all four taps lie inside the source, else 0.

Parity with a particular OpenCV build is not pinned at this boundary (as for
the pre-blur and the resize): this text is the definition.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

FIX_MIN, FIX_MAX = -32768 * 32, 32767 * 32
SPECIALS = (np.nan, np.inf, -np.inf, 1e30, -1e30)


def fix(c) -> np.ndarray:
    """q per coordinate (int32): the map conversion's fixed-point value."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(c, np.float32) * np.float32(32)
        t = np.where(np.isnan(t), np.float32(FIX_MIN), t)
        t = np.clip(t, np.float32(FIX_MIN), np.float32(FIX_MAX))
        return np.rint(t).astype(np.int32)


def convert(map_x, map_y, src_rows: int, src_cols: int):
    """(x0, y0, a, b, valid) per destination pixel."""
    qx, qy = fix(map_x), fix(map_y)
    x0, y0, a, b = qx >> 5, qy >> 5, qx & 31, qy & 31
    valid = (x0 >= 0) & (x0 + 1 < src_cols) & (y0 >= 0) & (y0 + 1 < src_rows)
    return x0, y0, a, b, np.where(valid, 255, 0).astype(np.uint8)


def packed(map_x, map_y, src_rows: int, src_cols: int) -> np.ndarray:
    """The two words per pixel as the library packs them (h x w x 2 uint32):
    (x0 & 0xffff) | (y0 << 16), then a | (b << 5)."""
    x0, y0, a, b, _ = convert(map_x, map_y, src_rows, src_cols)
    w0 = (x0.astype(np.int64) & 0xffff) | ((y0.astype(np.int64) & 0xffff) << 16)
    return np.stack([w0, a.astype(np.int64) | (b.astype(np.int64) << 5)], axis=-1).astype(np.uint32)


def remap(src, map_x, map_y) -> np.ndarray:
    """cv::remap(src, dst, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0) as pinned above."""
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    x0, y0, a, b, _ = convert(map_x, map_y, sh, sw)
    q = src.astype(np.int32)

    def tap(y, x):
        inside = (y >= 0) & (y < sh) & (x >= 0) & (x < sw)
        return np.where(inside, q[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)], 0)

    v = ((32 - a) * (32 - b) * tap(y0, x0) + a * (32 - b) * tap(y0, x0 + 1)
         + (32 - a) * b * tap(y0 + 1, x0) + a * b * tap(y0 + 1, x0 + 1) + 512) >> 10
    return v.astype(np.uint8)


def identity_maps(h: int, w: int):
    return (np.tile(np.arange(w, dtype=np.float32), (h, 1)),
            np.tile(np.arange(h, dtype=np.float32)[:, None], (1, w)))


def maps(h: int, w: int, src_rows: int, src_cols: int, view: int):
    """One view's deterministic h x w maps onto a src_rows x src_cols source: a
    radial term, a small rotation and a vertical offset, different per view,
    scaled so that every side of the destination has pixels sampling outside
    the source; then one row and one column of exact integer coordinates and
    the special values (NaN, +-inf, +-1e30, x*32 = k + 0.5 ties) spliced in."""
    v = np.linspace(-1.0, 1.0, h)[:, None] if h > 1 else np.zeros((1, 1))
    u = np.linspace(-1.0, 1.0, w)[None, :] if w > 1 else np.zeros((1, 1))
    r2 = u * u + v * v
    k1 = 0.06 if view == 0 else -0.04                # barrel / pincushion
    th = 0.02 if view == 0 else -0.015               # rotation, radians
    rad = 1.0 + k1 * r2
    c, s = np.cos(th), np.sin(th)
    # normalised source position in [-1.15, 1.15]: beyond the source on every side
    xn = 1.15 * rad * (c * u - s * v)
    yn = 1.15 * rad * (s * u + c * v) + (0.03 if view == 0 else -0.02)
    mx = ((xn + 1.0) * 0.5 * src_cols - 0.5).astype(np.float32)
    my = ((yn + 1.0) * 0.5 * src_rows - 0.5).astype(np.float32)
    mx, my = np.array(np.broadcast_to(mx, (h, w))), np.array(np.broadcast_to(my, (h, w)))   # (writable copies)
    # a row and a column of exact integer coordinates (fractions 0; some outside)
    i, j = h // 2, w - 1 - w // 3                    # (clear of the special values below)
    mx[i] = np.rint(np.linspace(-2, src_cols + 1, w))
    my[i] = float(src_rows // 2)
    my[:, j] = np.rint(np.linspace(-2, src_rows + 1, h))
    mx[:, j] = float(src_cols // 2)
    # the special values and the ties, on the top rows' first pixels
    flat_x, flat_y = mx.reshape(-1), my.reshape(-1)
    n = flat_x.size
    vals = list(SPECIALS) + [(2 * k + 0.5) / 32.0 for k in (0, 1, 2, 3)] + [(2 * k + 1.5) / 32.0 for k in (0, 1)] \
        + [-0.5 / 32.0, -1.5 / 32.0]
    for k, val in enumerate(vals):
        if 2 * k + 1 < n:
            flat_x[2 * k] = val                      # special x, ordinary y
            flat_y[2 * k + 1] = val                  # ordinary x, special y
    return mx, my


def random_image(h: int, w: int, seed: int) -> np.ndarray:
    """Random u8 with forced runs of 0 and of 255 (the extremes of every sum)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img[:, : max(1, w // 7)] = 255
    img[h // 2, :] = 255
    img[h // 3, w // 4: w // 2] = 0
    return img
