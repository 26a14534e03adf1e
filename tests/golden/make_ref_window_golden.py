"""Generate tests/golden/window/ref_window_ct_*.npz and ref_window_ad_*.npz from the
REFERENCE's own CT_pts, SAD and SSD (src/cost.cpp) called with other windows
than WIN_H x WIN_W.

Run by hand from the repo root, where a checkout of the reference lies beside
the repository (oracle.reference_dir()):

    python tests/golden/make_ref_window_golden.py

The reference's src/cost.cpp is compiled unmodified, with the reference's own
flags and against the stand-in headers in oracle/ref/include, together with
ref_window_driver.cpp, into a temporary directory; nothing compiled is kept.
ref_window_ct_<rows>x<cols>_s<scale>.npz holds the census tables of a seeded pair
per window ("l_<win>", "r_<win>", uint64 rows x cols; the images are not
blurred), ref_window_ad_<shape>_s<scale>_<win>.npz the SAD and SSD volumes
("sad", "ssd", float32 rows x cols x 80: disparities 0 .. 79, of which a case
(D, min_disp) is a slice).  window_cases.py regenerates the images;
tests/test_window_cpu.py compares the recipe with every fixture bit for bit.
"""
from __future__ import annotations

import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
import window_cases as cases  # noqa: E402


def run(exe, tmp, L, R, D, scale, window, mode):
    rows, cols = L.shape
    e_h, e_w = cases.effective(window, scale)
    req, res = os.path.join(tmp, "req.bin"), os.path.join(tmp, "res.bin")
    with open(req, "wb") as fh:
        fh.write(struct.pack("<7i", rows, cols, D, scale, e_h, e_w, mode))
        fh.write(L.tobytes())
        fh.write(R.tobytes())
    subprocess.run([exe, req, res], check=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    return res


def save(path, arrays):
    np.savez_compressed(path, **arrays)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20


def main() -> int:
    ref = oracle.reference_dir()
    if ref is None:
        print("no reference checkout found", file=sys.stderr)
        return 1
    inc = os.path.join(ROOT, "oracle", "ref", "include")
    flags = ["-std=c++11", "-O3", "-fopenmp", "-ffp-contract=off", "-I" + inc, "-I" + ref]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "driver")
        subprocess.run(["g++", *flags, "-w", "-c", "-o", os.path.join(tmp, "cost.o"),
                        os.path.join(ref, "src", "cost.cpp")], check=True)
        subprocess.run(["g++", *flags, "-Wall", "-c", "-o", os.path.join(tmp, "driver.o"),
                        os.path.join(HERE, "ref_window_driver.cpp")], check=True)
        subprocess.run(["g++", *flags, "-o", exe, os.path.join(tmp, "cost.o"), os.path.join(tmp, "driver.o")],
                       check=True)
        for s in (1, 2):
            for shape in cases.CENSUS_SHAPES:
                left, right = cases.census_pair(shape, s)
                L, R = cases.working(left, s), cases.working(right, s)
                out = {}
                for win in cases.CENSUS_WINDOWS[s]:
                    t = np.fromfile(run(exe, tmp, L, R, 0, s, win, 0), np.uint64).reshape(2, *L.shape)
                    out["l_" + cases.wid(win)], out["r_" + cases.wid(win)] = t[0], t[1]
                save(cases.census_fixture(shape, s), out)
        for name, s, win in cases.cost_fixture_cases():
            left, right = cases.cost_pair(name, s)
            L, R = cases.working(left, s), cases.working(right, s)
            out = {}
            for k, kind in enumerate(cases.KINDS):
                res = run(exe, tmp, L, R, cases.COST_DMAX, s, win, k + 1)
                out[kind] = np.fromfile(res, np.float32).reshape(*L.shape, cases.COST_DMAX)
            save(cases.cost_fixture(name, s, win), out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
