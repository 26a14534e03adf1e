"""sgm_device_bytes through every allocating setter on one handle: min_disp,
confidence, fill, reprojection and the input stages switched on one after the
other and off in another order; after each step the handle's bytes are the
fresh handle's plus the sum of what is on, and at the end the fresh handle's."""
from __future__ import annotations

import pytest

import rectify_recipe as rc
import reproject_recipe as rp
from stereo_matching_amd import SGM, _capi

pytestmark = pytest.mark.gpu

H, W, D = 24, 40, 32
RAW = (37, 53)          # the input size, then the maps' source size
NPX = H * W


def test_device_bytes_are_the_sum_of_what_is_on():
    raw = 2 * RAW[0] * RAW[1]        # the staging of two raw images
    size = {
        "min_disp": 16 * NPX,                        # both shifted tables
        "confidence": 2 * 4 * NPX,                   # 4 B per pixel per view
        "fill": 25 * NPX,                            # six f32 planes and the mask
        "reproject": (12 + 4 + 2) * NPX,             # xyz, depth, depth16
        "input_size": 2 * NPX + raw,                 # two full-size grey images, the staging (test_gpu_resize.py)
        "rectify": 2 * 8 * NPX + 2 * NPX + raw,      # two packed maps more (test_gpu_rectify.py)
    }
    maps = (*rc.maps(H, W, *RAW, 0), *rc.maps(H, W, *RAW, 1))
    with SGM(H, W, 1, D, views=2) as sgm, SGM(H, W, 1, D, views=2) as fresh:
        lib, base = _capi.lib(), fresh.device_bytes
        on = {
            "min_disp": lambda: _capi.check(lib.sgm_set_min_disp(sgm._h, 16), sgm._h),
            "confidence": lambda: sgm.set_confidence(True),
            "fill": lambda: sgm.set_fill("interpolate"),
            "reproject": lambda: sgm.set_reproject(rp.skewed_q(), outputs=("xyz", "depth", "depth16")),
            "input_size": lambda: sgm.set_input_size(*RAW),
            "rectify": lambda: (sgm.set_input_size(0, 0), sgm.set_rectify(*RAW, *maps)),
        }
        off = {
            "min_disp": lambda: _capi.check(lib.sgm_set_min_disp(sgm._h, 0), sgm._h),
            "confidence": lambda: sgm.set_confidence(False),
            "fill": lambda: sgm.set_fill("off"),
            "reproject": lambda: sgm.set_reproject(None),
            "rectify": lambda: sgm.set_rectify(0, 0),
        }
        assert sgm.device_bytes == base
        live = set()
        for name in ("min_disp", "confidence", "fill", "reproject", "input_size", "rectify"):
            on[name]()
            live.add(name)
            live -= {"input_size"} if name == "rectify" else set()   # (the maps take the input size's place)
            print(name, "on:", sgm.device_bytes - base)
            assert sgm.device_bytes == base + sum(size[k] for k in live), name
        for name in ("fill", "min_disp", "rectify", "confidence", "reproject"):
            off[name]()
            live.remove(name)
            print(name, "off:", sgm.device_bytes - base)
            assert sgm.device_bytes == base + sum(size[k] for k in live), name
        assert not live and sgm.device_bytes == base
