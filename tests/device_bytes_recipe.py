"""sgm_device_bytes of a few small handles, one per allocation path of sgm_create
and of the two setters that allocate beside it: the cases, and the one function
that measures them.  tests/test_gpu_device_bytes.py compares them with
tests/golden/device_bytes.json; tests/golden/make_device_bytes_golden.py
records that file (from the commit before a change to sgm_create, on the same
device)."""
from __future__ import annotations

import os
from contextlib import contextmanager

# name -> (constructor, (h, w, s, D), keyword arguments, environment switches)
# (min_disp, confidence: the constructor calls sgm_set_min_disp, sgm_set_confidence after sgm_create)
CASES = {
    "sgm_96x260_D128_v1": ("SGM", (96, 260, 1, 128), {"views": 1}, {}),
    "sgm_96x260_D128_v2": ("SGM", (96, 260, 1, 128), {"views": 2}, {}),
    "paths4_96x260_D128_v1": ("SGM", (96, 260, 1, 128), {"views": 1, "paths": 4}, {}),
    "paths4_96x260_D128_v2": ("SGM", (96, 260, 1, 128), {"views": 2, "paths": 4}, {}),
    "slant_80x240_D256": ("SGM", (80, 240, 1, 256), {}, {"SGM_SLANT": "1"}),
    "bands16_120x330_D64": ("SGM", (120, 330, 1, 64), {}, {"SGM_BAND_ROWS": "16"}),
    "bm_96x260_D64": ("BM", (96, 260, 1, 64), {}, {}),
    "aux_only_96x260_D128": ("SGM", (96, 260, 1, 128), {"aux_only": True}, {}),
    "setters_96x260_D64": ("SGM", (96, 260, 1, 64), {"min_disp": 16, "confidence": True}, {}),
}

SWITCHES = ("SGM_SLANT", "SGM_VSTRIP", "SGM_BAND_ROWS", "SGM_P4_HPAIR", "SGM_CONFIDENCE")


@contextmanager
def switches(env):
    """The switches sgm_create reads, set to env alone for the block."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def measure(name):
    """sgm_device_bytes of the case's handle."""
    import stereo_matching_amd as pkg
    cls, size, kw, env = CASES[name]
    with switches(env), getattr(pkg, cls)(*size, **kw) as sgm:
        return sgm.device_bytes
