"""What the tests share: the two g++ recipes for the tests' C++ programs, a
runner, the PGM writer and the bit-pattern views.  A plain module (tests/ is on
sys.path): test files import it as they import pyref or the *_recipe modules.

The two recipes are claims about the code, each made here once:
  - include/sgm_amd/*.h compile with -std=c++11 -Wall -Werror; without HIP
    headers unless a surface asks for them (library_program);
  - the host-side headers under csrc/ that tests/cpp/*_main.cpp replay compile
    as c++17 with -Wall -Werror and run clean under ASan and UBSan
    (host_program)."""
from __future__ import annotations

import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_built = {}     # (source, flags) -> program, for one pytest process: five files run examples/stereo_node.cpp


def _stem(src):
    return os.path.splitext(os.path.basename(src))[0]


def _compile(argv):
    subprocess.run(argv, check=True, capture_output=True, text=True)


def library_program(tmp_path_factory, src, *, hip_headers=False, link_hip=True, pthread=False):
    """src as a program linked to libsgm_hip.so (built first if it is missing); returns its path.
    hip_headers: the source uses the HIP runtime API on the host (plain g++, no hipcc).
    link_hip: link amdhip64 too (the example node goes through the library alone)."""
    from stereo_matching_amd import _capi
    key = (src, hip_headers, link_hip, pthread)
    if key not in _built:
        if not os.path.exists(_capi.LIB_PATH):
            _capi.build()
        out = str(tmp_path_factory.mktemp("cpp") / _stem(src))
        libdir = os.path.dirname(_capi.LIB_PATH)
        _compile(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
                 + (["-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"] if hip_headers else [])
                 + [src, "-L", libdir, "-lsgm_hip", f"-Wl,-rpath,{libdir}"]
                 + (["-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"] if link_hip else [])
                 + (["-pthread"] if pthread else []) + ["-o", out])
        _built[key] = out
    return _built[key]


def host_program(outdir, src, *, sanitized=True, fp_contract_off=False):
    """src (a stand-alone host program with its own main) built into outdir; returns its path.
    sanitized: -O1 -g under ASan and UBSan with every report fatal (no sanitized build goes without
    -fno-sanitize-recover=all, so it is no option); otherwise a plain -O2 build.
    fp_contract_off: no FMA, as the library's kernels are built."""
    out = os.path.join(str(outdir), _stem(src) + ("" if sanitized else "_plain"))
    _compile(["g++", "-std=c++17", "-Wall", "-Werror"]
             + (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"])
             + (["-ffp-contract=off"] if fp_contract_off else []) + [src, "-o", out])
    return out


def run(exe, *args, timeout=60):
    """The program run directly (no wrapper, no preload, the environment as it is)."""
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=timeout)


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def bits(a):
    """A float32 array as its uint32 bit patterns; any other dtype unchanged."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def f32_bits(a):
    """The array cast to float32, then as uint32 bit patterns (a float64 array is rounded first)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
