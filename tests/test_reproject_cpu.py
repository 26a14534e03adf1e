"""CPU checks of the reprojection's pinned form (tests/reproject_recipe.py,
DESIGN.md 5m): the recipe against the written-out formulas, camera_q against the
pinhole camera, the missing rules one by one, depth16's rounding; the header,
the binding and the build list name the feature; the host-side checks run under
sanitizers as a stand-alone program."""
from __future__ import annotations

import os

import numpy as np
import pytest

import reproject_recipe as rp
import support
from stereo_matching_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00000


def ulps(a, b):
    """Distance of two float32 arrays of one sign in units in the last place."""
    a, b = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(a - b)


@pytest.mark.parametrize("scale", [1, 2])
def test_recipe_equals_the_written_out_formulas(scale):
    q = rp.skewed_q()
    disp = rp.hand_map(7, 11, 32, 0, seed=scale)
    got = rp.reproject(disp, q, 33, scale, 0.0, 1000.0)
    for i in range(7):
        for j in range(11):
            x, y, d = float(j * scale), float(i * scale), float(disp[i, j])
            h = [((q[4 * r] * x + q[4 * r + 1] * y) + q[4 * r + 2] * d) + q[4 * r + 3] for r in range(4)]
            if disp[i, j] == np.float32(33) or h[3] == 0.0:
                assert (rp.bits(got["xyz"][i, j]) == NAN_BITS).all() and rp.bits(got["depth"])[i, j] == NAN_BITS
                assert got["depth16"][i, j] == 0 and got["missing"][i, j]
                continue
            iw = 1.0 / h[3]
            want = [np.float32(h[k] * iw) for k in range(3)]
            assert [v.tobytes() for v in got["xyz"][i, j]] == [v.tobytes() for v in want]
            assert got["depth"][i, j].tobytes() == want[2].tobytes()
            r = np.rint(want[2] * np.float32(1000.0))
            assert got["depth16"][i, j] == (int(r) if 1 <= r <= 65535 else 0)
    # python floats are IEEE doubles and a * b + c on them is two roundings: the loop above is the form


def test_camera_q_is_the_pinhole_camera_within_one_ulp():
    """With fx == fy = f: Z = f b / d and X = (x - cx) Z / f, Y = (y - cy) Z / f.

    The recipe rounds a double result to float32 once per coordinate: 0.5 ulp of float32 from the
    real value, plus the double arithmetic's relative error (Z: f * (1 / (d / b))... three double
    roundings, under 2^-51), which moves the rounded float32 only when the real value lies within
    2^-51 of a rounding boundary.  The pinhole formulas evaluated in double and rounded once are
    equally within 0.5 ulp of the same real value, so the two float32 results are equal or adjacent:
    at most 1 ulp apart.  Measured on this grid: 0 ulp for Z, X and Y on every pixel."""
    f, cx, cy, b = 721.5, 609.5, 172.75, 0.54
    q = rp.camera_q(f, f, cx, cy, b)
    assert list(q) == [1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 0, f, 0, 0, 1.0 / b, 0]
    rows, cols = 24, 80
    disp = (np.random.default_rng(3).random((rows, cols)) * 63 + 0.25).astype(np.float32)
    got = rp.reproject(disp, q, 65, 2)
    assert not got["missing"].any()
    x = (np.arange(cols) * 2.0)[None, :]
    y = (np.arange(rows) * 2.0)[:, None]
    d = disp.astype(np.float64)
    Z = f * b / d
    worst = [int(ulps(got["depth"], Z.astype(np.float32)).max()),
             int(ulps(got["xyz"][..., 0], ((x - cx) * Z / f).astype(np.float32)).max()),
             int(ulps(got["xyz"][..., 1], ((y - cy) * Z / f + 0 * x).astype(np.float32)).max())]
    print("ulps from the pinhole formulas (Z, X, Y):", worst)
    assert max(worst) <= 1
    assert np.array_equal(rp.bits(got["xyz"][..., 2]), rp.bits(got["depth"]))


@pytest.mark.parametrize("m", [0, 16])
def test_the_invalid_marker_is_missing(m):
    D = 32
    q = rp.camera_q(500, 500, 4, 2, 0.1)
    disp = np.full((3, 5), 7.5, np.float32)
    disp[1, 2] = D + m + 1
    disp[2, 4] = D + 1 if m else D + 2                # only the handle's own marker counts
    got = rp.reproject(disp, q, D + m + 1)
    want = np.zeros((3, 5), bool)
    want[1, 2] = True
    assert np.array_equal(got["missing"], want)
    assert (rp.bits(got["xyz"])[1, 2] == NAN_BITS).all() and rp.bits(got["depth"])[1, 2] == NAN_BITS
    assert got["depth16"][1, 2] == 0 and got["depth16"][2, 4] != 0


def test_a_zero_w_is_missing():
    q = rp.camera_q(500, 500, 4, 2, 0.1)              # W' = d / baseline: 0 at d = 0
    disp = np.array([[0.0, 1.0, 0.0, 2.0, 4.0]] * 3, np.float32)
    got = rp.reproject(disp, q, 33)
    assert np.array_equal(got["missing"], disp == 0)
    assert (rp.bits(got["depth"])[disp == 0] == NAN_BITS).all() and (got["depth16"][disp == 0] == 0).all()
    assert np.isfinite(got["xyz"][disp != 0]).all()


def test_the_range_test_on_both_sides_and_at_the_bound():
    q = rp.camera_q(512, 512, 0, 0, 0.125)            # Z = 64 / d, exact for powers of two
    disp = np.array([[8.0, 4.0, 2.0, 1.0, 0.5]] * 3, np.float32)
    z = np.array([8.0, 16.0, 32.0, 64.0, 128.0], np.float32)
    free = rp.reproject(disp, q, 33)
    assert np.array_equal(free["depth"][0], z) and not free["missing"].any()    # max_range = 0: no test
    got = rp.reproject(disp, q, 33, max_range=32.0)
    assert np.array_equal(got["missing"][0], z > 32)                            # Z == max_range stays
    assert np.array_equal(got["depth"][0][:3], z[:3])
    nxt = float(np.nextafter(np.float32(32), np.float32(0)))
    assert np.array_equal(rp.reproject(disp, q, 33, max_range=nxt)["missing"][0], z >= 32)


def test_a_depth_at_or_behind_the_camera_is_missing_under_a_range_test():
    q = rp.camera_q(512, 512, 0, 0, -0.125)           # a negative baseline: Z = -64 / d
    qz = rp.camera_q(512, 512, 0, 0, 0.125)
    qz[11] = 0.0                                      # Z' = 0 everywhere: Z = 0
    disp = np.array([[8.0, 4.0, 2.0, 1.0, 0.5]] * 3, np.float32)
    for qq, zs in ((q, -1), (qz, 0)):
        free = rp.reproject(disp, qq, 33)
        assert not free["missing"].any() and (np.sign(free["depth"]) == zs).all()
        assert (free["depth16"] == 0).all()                                     # below 1: 0, not missing
        assert rp.reproject(disp, qq, 33, max_range=1000.0)["missing"].all()


def test_depth16_rounds_to_even_and_saturates_to_zero():
    q = np.zeros(16)
    q[0] = q[5] = q[10] = q[15] = 1.0                 # Z' = d, W' = 1: Z is the map itself
    z = np.array([0.5, 1.5, 2.5, 0.75, 65535.0, 65535.5, 65534.5, 65536.0, 0.25, 3.5], np.float32)
    disp = z
    got = rp.reproject(np.tile(disp, (3, 1)), q, 1e9, depth_scale=1.0)
    assert np.array_equal(got["depth"][0], z)
    #                 0.5->0 (ties to even, below 1)  1.5->2  2.5->2  0.75->1  65535  65535.5->65536: 0
    assert list(got["depth16"][0]) == [0, 2, 2, 1, 65535, 0, 65534, 0, 0, 4]
    # one fp32 multiply: millimetres of a depth in metres
    got = rp.reproject(np.tile(disp, (3, 1)), q, 1e9, depth_scale=1000.0)
    want = np.rint(z * np.float32(1000))
    assert list(got["depth16"][0]) == [int(v) if 1 <= v <= 65535 else 0 for v in want]


def test_header_binding_and_build_list_carry_the_feature():
    header = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    for name in ("sgm_set_reproject", "sgm_get_reproject", "sgm_reproject_device", "sgm_stage_reproject",
                 "sgm_get_reprojected", "sgm_stage_reprojected", "sgm_camera_q"):
        assert name + "(" in header and name in _capi.EXPORTS
    assert "SGM_REPROJECT_XYZ = 1, SGM_REPROJECT_DEPTH = 2, SGM_REPROJECT_DEPTH16 = 4" in header
    assert _capi.REPROJECT_OUTPUTS == rp.OUTPUT_BITS == {"xyz": 1, "depth": 2, "depth16": 4}
    assert "#define SGM_HIP_VERSION 2 " in header     # the struct and the version stay
    mk = open(os.path.join(ROOT, "stereo_matching_amd", "csrc", "Makefile")).read()
    assert "sgm_reproject.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    assert "-ffp-contract=off" in mk                  # no FMA in the new file either


def test_host_side_checks_run_clean_under_sanitizers(tmp_path):
    # the setter's and the device call's checks (csrc/sgm_reproject_args.h) as a stand-alone CPU program
    exe = support.host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "reproject_args_main.cpp"))
    r = support.run(exe)
    assert r.returncode == 0 and "reproject args ok" in r.stdout, r.stdout + r.stderr
