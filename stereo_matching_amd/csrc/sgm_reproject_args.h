// sgm_reproject_args.h -- the host side of the reprojection (sgm_reproject.hip,
// DESIGN.md 5m): the checks of sgm_set_reproject's parameters and of a
// reprojection call's pointers and pitches, and the pinhole Q of sgm_camera_q.
// Plain C++ with no HIP in it, so that tests/cpp/reproject_args_main.cpp can run
// it on the CPU under a sanitizer.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdio.h>

namespace sgm {

// The product bits of include/sgm_hip.h (SGM_REPROJECT_*), by value.
constexpr int kReprojectXyz = 1, kReprojectDepth = 2, kReprojectDepth16 = 4;
constexpr int kReprojectAll = kReprojectXyz | kReprojectDepth | kReprojectDepth16;

// sgm_set_reproject's parameters on a handle that is aux_only (it runs no
// frames and may hold Q alone) or computes the right view (Q belongs to the
// left camera).  Returns false with the reason in why.
inline bool reproject_set_ok(const double *q, int outputs, float max_range, float depth_scale, bool aux_only,
                             bool right_view, char *why, size_t n) {
    if (right_view) {
        snprintf(why, n, "a SGM_VIEW_RIGHT handle: Q belongs to the left camera");
        return false;
    }
    for (int k = 0; k < 16; ++k)
        if (!isfinite(q[k])) {
            snprintf(why, n, "q[%d] is not finite", k);
            return false;
        }
    if (outputs & ~kReprojectAll) {
        snprintf(why, n, "unknown bits in outputs: %d", outputs);
        return false;
    }
    if (outputs == 0 && !aux_only) {
        snprintf(why, n, "outputs is 0: only an aux_only handle may hold Q alone (NULL switches reprojection off)");
        return false;
    }
    if (!isfinite(max_range) || max_range < 0.0f) {
        snprintf(why, n, "max_range must be finite and >= 0 (0: no range test), got %g", (double)max_range);
        return false;
    }
    if ((outputs & kReprojectDepth16) && (!isfinite(depth_scale) || !(depth_scale > 0.0f))) {
        snprintf(why, n, "depth_scale must be finite and > 0 for depth16, got %g", (double)depth_scale);
        return false;
    }
    return true;
}

// One reprojection call on a cols-wide working grid: Q set, a map, at least one
// product, and no pitch (in elements of each buffer's type) below its row.
inline bool reproject_call_ok(bool q_set, bool have_disp, int pitch, bool have_xyz, int xyz_pitch, bool have_depth,
                              int depth_pitch, bool have_depth16, int depth16_pitch, int cols, char *why,
                              size_t n) {
    if (!q_set) {
        snprintf(why, n, "no Q is set (sgm_set_reproject)");
        return false;
    }
    if (!have_disp) {
        snprintf(why, n, "NULL disparity map");
        return false;
    }
    if (!have_xyz && !have_depth && !have_depth16) {
        snprintf(why, n, "all three products are NULL");
        return false;
    }
    if (pitch < cols) {
        snprintf(why, n, "pitch %d below cols %d", pitch, cols);
        return false;
    }
    if (have_xyz && (long long)xyz_pitch < 3LL * cols) {
        snprintf(why, n, "xyz_pitch %d below 3 x cols %lld", xyz_pitch, 3LL * cols);
        return false;
    }
    if (have_depth && depth_pitch < cols) {
        snprintf(why, n, "depth_pitch %d below cols %d", depth_pitch, cols);
        return false;
    }
    if (have_depth16 && depth16_pitch < cols) {
        snprintf(why, n, "depth16_pitch %d below cols %d", depth16_pitch, cols);
        return false;
    }
    return true;
}

// `which` names exactly one product.
inline bool reproject_one_bit(int which) {
    return which == kReprojectXyz || which == kReprojectDepth || which == kReprojectDepth16;
}

// Elements per pixel of product `which` (one bit): 3 for XYZ, else 1.
inline int reproject_channels(int which) { return which == kReprojectXyz ? 3 : 1; }

// Bytes per element of product `which` (one bit): 2 for depth16, else 4.
inline int reproject_elem_bytes(int which) { return which == kReprojectDepth16 ? 2 : 4; }

// The pinhole Q of sgm_camera_q, row-major; false for a zero or non-finite
// baseline or a non-finite intrinsic (Q would not be finite).
inline bool camera_q(float fx, float fy, float cx, float cy, double baseline, double *q) {
    const double f = ((double)fx + fy) / 2;
    if (!isfinite(f) || !isfinite(cx) || !isfinite(cy) || !isfinite(baseline) || baseline == 0.0) return false;
    const double ib = 1.0 / baseline;
    if (!isfinite(ib)) return false;
    for (int k = 0; k < 16; ++k) q[k] = 0.0;
    q[0] = 1.0;
    q[3] = -(double)cx;
    q[5] = 1.0;
    q[7] = -(double)cy;
    q[11] = f;
    q[14] = ib;
    return true;
}

}  // namespace sgm
