"""CPU checks of the median fill's launch budget: include/sgm_hip.h declares
sgm_set_post_filter_launches and sgm_post_filter_proved_at, the built library
exports them, _capi binds them, they validate before touching a device, and
the option lives on the handle: sgm_params and SGM_HIP_VERSION are unchanged
(tests/test_paths4_cpu.py pins the layout)."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import subprocess

import pytest

from stereo_matching_amd import BM, GPU_SGM, SGM, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgm_hip.h")
NEW = ("sgm_set_post_filter_launches", "sgm_post_filter_proved_at")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    return _capi.lib()


def test_header_declares_the_two_functions():
    text = open(HEADER).read()
    assert re.search(r"^int sgm_set_post_filter_launches\(sgm_handle \*h, int n\);", text, re.M)
    assert re.search(r"^int sgm_post_filter_proved_at\(sgm_handle \*h, int \*launch\);", text, re.M)
    # the option is a handle setter: the struct still ends with `paths`, version 2
    body = text[text.index("typedef struct sgm_params {"):text.index("} sgm_params;")]
    fields = re.findall(r"^\s*(?:int|float)\s+(\w+);", body, re.M)
    assert fields[-1] == "paths" and len(fields) == len(_capi.Params._fields_) == 17
    assert re.search(r"^#define SGM_HIP_VERSION 2\b", text, re.M)
    assert "unless a launch budget is set" in text and "EXCEPT with post_filter" not in text


def test_library_exports_and_binding(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    for name in NEW:
        assert name in _capi.EXPORTS
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.sgm_set_post_filter_launches.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.sgm_post_filter_proved_at.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]


def test_null_handle_rejected(lib):
    k = ctypes.c_int(7)
    assert lib.sgm_set_post_filter_launches(None, 3) == _capi.SGM_ERR_INVALID_ARG
    assert lib.sgm_post_filter_proved_at(None, ctypes.byref(k)) == _capi.SGM_ERR_INVALID_ARG
    assert k.value == 7


def test_python_surface():
    for cls in (SGM, BM, GPU_SGM):
        p = inspect.signature(cls.__init__).parameters["post_filter_launches"]
        assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(SGM.set_post_filter_launches) and callable(SGM.post_filter_proved_at)
