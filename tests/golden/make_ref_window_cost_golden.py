"""Generate tests/golden/ref_window_cost_<case>.npz from the REFERENCE's own
SAD and SSD (src/cost.cpp).

Run by hand from the repo root, where a checkout of the reference lies beside
the repository (oracle.reference_dir()):

    python tests/golden/make_ref_window_cost_golden.py

The reference's src/cost.cpp is compiled unmodified, with the reference's own
flags and against the stand-in headers in oracle/ref/include, together with
ref_window_cost_driver.cpp, into a temporary directory; nothing compiled is
kept.  Per case the fixture holds the full SAD and SSD volumes ("sad", "ssd",
float32 rows x cols x D) of a seeded pair, which window_cost_cases.inputs()
regenerates; tests/test_window_cost_cpu.py compares the recipe with them bit
for bit.
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
import window_cost_cases as cases  # noqa: E402
import window_cost_recipe as wc  # noqa: E402


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
                        os.path.join(HERE, "ref_window_cost_driver.cpp")], check=True)
        subprocess.run(["g++", *flags, "-o", exe, os.path.join(tmp, "cost.o"), os.path.join(tmp, "driver.o")],
                       check=True)
        for name, (h, w, D, scale, m) in cases.GOLDEN.items():
            left, right = cases.inputs(name)
            L, R = wc.working(left, scale), wc.working(right, scale)
            rows, cols = L.shape
            out = {}
            for k, kind in enumerate(wc.KINDS):
                req, res = os.path.join(tmp, "req.bin"), os.path.join(tmp, "res.bin")
                with open(req, "wb") as fh:
                    fh.write(struct.pack("<7i", rows, cols, D, scale, m, k + 1, 0))
                    fh.write(L.tobytes())
                    fh.write(R.tobytes())
                subprocess.run([exe, req, res], check=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
                out[kind] = np.fromfile(res, np.float32).reshape(rows, cols, D)
            path = os.path.join(HERE, f"ref_window_cost_{name}.npz")
            np.savez_compressed(path, **out)
            print(f"{name}: {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
