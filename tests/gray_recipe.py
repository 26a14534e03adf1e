"""The colour input's grey conversion, restated in numpy: what
sgm_gray_device computes and what the fused resize and remap launches compute
per tap.

    Y = (4899 R + 9617 G + 1868 B + 8192) >> 14

0.299, 0.587 and 0.114 at 14 bits (they sum to 16384), OpenCV 2.4.13's
cvtColor(BGR2GRAY) and its decoder's IMREAD_GRAYSCALE conversion.  The alpha
byte of a 4-channel format is ignored."""
from __future__ import annotations

import numpy as np

FORMATS = ("bgr8", "rgb8", "bgra8", "rgba8")
_RED_AT = {"bgr8": 2, "rgb8": 0, "bgra8": 2, "rgba8": 0}


def bytes_per_pixel(fmt: str) -> int:
    return {"gray8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}[fmt]


def gray(img: np.ndarray, fmt: str) -> np.ndarray:
    """(h, w, bytes_per_pixel(fmt)) uint8 -> (h, w) uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == bytes_per_pixel(fmt), img.shape
    red = _RED_AT[fmt]
    r = img[..., red].astype(np.int64)
    g = img[..., 1].astype(np.int64)
    b = img[..., 2 - red].astype(np.int64)
    y = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
    assert y.min(initial=0) >= 0 and y.max(initial=0) <= 255
    return y.astype(np.uint8)


def random_image(h: int, w: int, ch: int, seed: int) -> np.ndarray:
    """Random (h, w, ch) u8 with forced runs of black, white and the pure primaries."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    img[:, : max(1, w // 7)] = 255
    img[h // 2, :] = 0
    for c in range(3):
        img[(h // 3 + c) % h, w // 4: w // 2] = 0
        img[(h // 3 + c) % h, w // 4: w // 2, c] = 255
    return img


def from_gray(g: np.ndarray, fmt: str, alpha: int = 77) -> np.ndarray:
    """The colour image with R = G = B = g (its grey is g again)."""
    ch = bytes_per_pixel(fmt)
    img = np.repeat(np.asarray(g, np.uint8)[..., None], ch, axis=2)
    if ch == 4:
        img[..., 3] = alpha
    return np.ascontiguousarray(img)
