"""Generate tests/golden/ct/ref_ct_<case>.npz from the REFERENCE's own CT
(src/cost.cpp:62-96), called as Solver::build_dsi calls it.

Run by hand from the repo root, where a checkout of the reference lies beside
the repository (oracle.reference_dir()):

    python tests/golden/make_ref_ct_golden.py

The reference's src/cost.cpp is compiled unmodified, with the flags of
make_ref_window_cost_golden.py and against the stand-in headers in
oracle/ref/include, together with ref_ct_driver.cpp, into a temporary directory;
nothing compiled is kept.  Two programs are built: the plain one, and for the
weighted cases one with -D'WEIGHTED_COST=(*ref_weighted_cost)' as
make_ref_weighted_golden.py compiles it.  Per case of ct_cost_recipe.GOLDEN the
fixture holds the full volume ("ct", uint8 rows x cols x D: the costs are
integers of at most 62) of a seeded pair, which ct_cost_recipe.inputs()
regenerates; tests/test_ct_cost_cpu.py compares the recipe with it bit for bit.
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
import ct_cost_recipe as ct  # noqa: E402


def build(tmp, ref, flags, tag, cost_defs, driver_defs):
    cost_o, driver_o, exe = (os.path.join(tmp, f"{n}_{tag}") for n in ("cost.o", "driver.o", "driver"))
    subprocess.run(["g++", *flags, "-w", *cost_defs, "-c", "-o", cost_o, os.path.join(ref, "src", "cost.cpp")],
                   check=True)
    subprocess.run(["g++", *flags, "-Wall", *driver_defs, "-c", "-o", driver_o,
                    os.path.join(HERE, "ref_ct_driver.cpp")], check=True)
    subprocess.run(["g++", *flags, "-o", exe, cost_o, driver_o], check=True)
    return exe


def main() -> int:
    ref = oracle.reference_dir()
    if ref is None:
        print("no reference checkout found", file=sys.stderr)
        return 1
    inc = os.path.join(ROOT, "oracle", "ref", "include")
    flags = ["-std=c++11", "-O3", "-fopenmp", "-ffp-contract=off", "-I" + inc, "-I" + ref]
    os.makedirs(ct.GOLDEN_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = {False: build(tmp, ref, flags, "plain", [], []),
               True: build(tmp, ref, flags, "weighted", ["-DWEIGHTED_COST=(*ref_weighted_cost)"],
                           ["-DREF_CT_WEIGHTED"])}
        for name in ct.GOLDEN:
            _, _, D, scale, m, _, weighted = ct.CASES[name]
            left, right = ct.inputs(name)
            L, R = ct.working(left, scale), ct.working(right, scale)
            rows, cols = L.shape
            req, res = os.path.join(tmp, "req.bin"), os.path.join(tmp, "res.bin")
            with open(req, "wb") as fh:
                fh.write(struct.pack("<7i", rows, cols, D, scale, m, *ct.effective(name)))
                fh.write(L.tobytes())
                fh.write(R.tobytes())
            subprocess.run([exe[weighted], req, res], check=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
            path = ct.fixture(name)
            np.savez_compressed(path, ct=np.fromfile(res, np.uint8).reshape(rows, cols, D))
            print(f"{name}: {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
