"""Generate tests/golden/weighted/*.npz from the REFERENCE's own CT_pts, SAD and
SSD (src/cost.cpp) with WEIGHTED_COST switched on.

Run by hand from the repo root, where a checkout of the reference lies beside
the repository (oracle.reference_dir()):

    python tests/golden/make_ref_weighted_golden.py

The reference's src/cost.cpp is compiled unmodified, with the flags of
make_ref_window_golden.py and against the stand-in headers in oracle/ref/include,
into a temporary directory; nothing compiled is kept.  The constant is 0 in
inc/Solver.h; -D'WEIGHTED_COST=(*ref_weighted_cost)' turns its definition into a
global pointer that ref_weighted_driver.cpp points at a true, so that every
`if (WEIGHTED_COST)` of the unmodified source takes its weighted branch.

ref_weighted_weights.npz holds Solver::Solver's table per effective window
("<e_h>x<e_w>", float32), ref_weighted_ct_<rows>x<cols>_s<scale>.npz the census
tables of a seeded pair per window ("l_<win>", "r_<win>", uint64; not blurred),
ref_weighted_ad_<shape>_s<scale>_<win>.npz the SAD and SSD volumes ("sad", "ssd",
float32 rows x cols x 80).  tests/window_cases.py regenerates the images,
tests/weighted_recipe.py lists the cases; tests/test_weighted_cpu.py compares the
recipe with every fixture bit for bit.
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
import weighted_recipe as wt  # noqa: E402
import window_cases as cases  # noqa: E402


def run(exe, tmp, L, R, D, scale, e_h, e_w, mode):
    rows, cols = L.shape
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
    os.makedirs(wt.GOLDEN_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "driver")
        subprocess.run(["g++", *flags, "-w", "-DWEIGHTED_COST=(*ref_weighted_cost)", "-c", "-o",
                        os.path.join(tmp, "cost.o"), os.path.join(ref, "src", "cost.cpp")], check=True)
        subprocess.run(["g++", *flags, "-Wall", "-c", "-o", os.path.join(tmp, "driver.o"),
                        os.path.join(HERE, "ref_weighted_driver.cpp")], check=True)
        subprocess.run(["g++", *flags, "-o", exe, os.path.join(tmp, "cost.o"), os.path.join(tmp, "driver.o")],
                       check=True)
        none = np.zeros((1, 1), np.uint8)
        save(wt.WEIGHTS_FIXTURE,
             {f"{e_h}x{e_w}": np.fromfile(run(exe, tmp, none, none, 0, 1, e_h, e_w, 3), np.float32).reshape(e_h, e_w)
              for e_h, e_w in wt.weight_windows()})
        for s in (1, 2):
            for shape in wt.CENSUS_SHAPES:
                left, right = cases.census_pair(shape, s)
                L, R = cases.working(left, s), cases.working(right, s)
                out = {}
                for win in wt.CENSUS_WINDOWS[s]:
                    res = run(exe, tmp, L, R, 0, s, *cases.effective(win, s), 0)
                    t = np.fromfile(res, np.uint64).reshape(2, *L.shape)
                    out["l_" + cases.wid(win)], out["r_" + cases.wid(win)] = t[0], t[1]
                save(cases.census_fixture(shape, s, "weighted"), out)
        for name, s, win in wt.COST_FIXTURES:
            left, right = cases.cost_pair(name, s)
            L, R = cases.working(left, s), cases.working(right, s)
            out = {}
            for k, kind in enumerate(cases.KINDS):
                res = run(exe, tmp, L, R, cases.COST_DMAX, s, *cases.effective(win, s), k + 1)
                out[kind] = np.fromfile(res, np.float32).reshape(*L.shape, cases.COST_DMAX)
            save(cases.cost_fixture(name, s, win, "weighted"), out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
