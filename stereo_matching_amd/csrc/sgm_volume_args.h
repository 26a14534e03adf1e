// sgm_volume_args.h -- the host side of the caller's cost volume (sgm_volume.hip,
// DESIGN.md 5n): the stride rule of sgm_volume, its layout classification and
// the extent of the source, for the C-ABI's checks, the docs and the tests.
// Plain C++ with no HIP in it, so that tests/cpp/volume_args_main.cpp can run it
// on the CPU under a sanitizer.
#pragma once

#include <limits.h>
#include <stddef.h>
#include <stdio.h>

namespace sgm {

// The element types of include/sgm_hip.h (SGM_VOL_*), by value.
constexpr int kVolF32 = 0, kVolF16 = 1;

// Which stride is the unit one: "HWD" (stride_disp == 1, the library's own
// layout) or "DHW" (stride_col == 1, torch's [D, H, W]).
enum VolLayout { VOL_LAYOUT_BAD = 0, VOL_LAYOUT_HWD = 1, VOL_LAYOUT_DHW = 2 };

// Bytes per element (0: an unknown dtype).
inline int volume_elem_bytes(int dtype) { return dtype == kVolF32 ? 4 : dtype == kVolF16 ? 2 : 0; }

// The stride rule: exactly one of stride_disp == 1 and stride_col == 1, no
// negative stride, and no two elements of the rows x cols x D volume at one
// address -- by the closed form: the three (stride, extent) pairs sorted by
// stride, the smallest stride at least 1 and each further stride at least the
// previous stride times the previous extent.  Also refuses a volume whose last
// byte lies past what a signed 64-bit offset reaches.  Returns the layout, or
// VOL_LAYOUT_BAD with the reason in why.
inline VolLayout volume_layout(int dtype, long long stride_row, long long stride_col, long long stride_disp,
                               int rows, int cols, int D, char *why, size_t n) {
    const int eb = volume_elem_bytes(dtype);
    if (!eb) {
        snprintf(why, n, "dtype %d is neither SGM_VOL_F32 nor SGM_VOL_F16", dtype);
        return VOL_LAYOUT_BAD;
    }
    if (rows < 1 || cols < 1 || D < 1) {
        snprintf(why, n, "empty volume %d x %d x %d", rows, cols, D);
        return VOL_LAYOUT_BAD;
    }
    if (stride_row < 0 || stride_col < 0 || stride_disp < 0) {
        snprintf(why, n, "negative stride (%lld, %lld, %lld)", stride_row, stride_col, stride_disp);
        return VOL_LAYOUT_BAD;
    }
    const bool hwd = stride_disp == 1, dhw = stride_col == 1;
    if (hwd && dhw && cols > 1 && D > 1) {
        snprintf(why, n, "stride_col and stride_disp are both 1: columns and disparities share addresses");
        return VOL_LAYOUT_BAD;
    }
    if (!hwd && !dhw) {
        snprintf(why, n, "neither stride_disp (HWD) nor stride_col (DHW) is 1: (%lld, %lld, %lld)", stride_row,
                 stride_col, stride_disp);
        return VOL_LAYOUT_BAD;
    }
    long long s[3] = {stride_row, stride_col, stride_disp};
    long long e[3] = {rows, cols, D};
    for (int a = 0; a < 3; ++a)  // by stride; equal strides: the longer axis later
        for (int b = a + 1; b < 3; ++b)
            if (s[b] < s[a] || (s[b] == s[a] && e[b] < e[a])) {
                const long long ts = s[a], te = e[a];
                s[a] = s[b], e[a] = e[b];
                s[b] = ts, e[b] = te;
            }
    // (an axis of extent 1 takes no room: its stride is never multiplied in)
    long long need = 1;  // the smallest stride the next axis of extent > 1 may have
    for (int a = 0; a < 3; ++a) {
        if (e[a] == 1) continue;
        if (s[a] < need) {
            snprintf(why, n, "overlapping strides (%lld, %lld, %lld) for %d x %d x %d: a stride of %lld where %lld "
                             "is the least that keeps elements apart",
                     stride_row, stride_col, stride_disp, rows, cols, D, s[a], need);
            return VOL_LAYOUT_BAD;
        }
        // (three terms below LLONG_MAX / 16 elements each: their sum in bytes stays below LLONG_MAX)
        if (s[a] > LLONG_MAX / 16 / e[a]) {
            snprintf(why, n, "past a 64-bit byte offset: strides (%lld, %lld, %lld)", stride_row, stride_col,
                     stride_disp);
            return VOL_LAYOUT_BAD;
        }
        need = s[a] * e[a];
    }
    return hwd && !(dhw && D == 1) ? VOL_LAYOUT_HWD : VOL_LAYOUT_DHW;
}

// Elements from the volume's first to one past its last: what the source must
// hold behind d_cost (times volume_elem_bytes for bytes).  For strides
// volume_layout accepts.
inline long long volume_extent_elems(long long stride_row, long long stride_col, long long stride_disp, int rows,
                                     int cols, int D) {
    return (rows - 1) * stride_row + (cols - 1) * stride_col + (D - 1) * stride_disp + 1;
}

inline long long volume_extent_bytes(int dtype, long long stride_row, long long stride_col, long long stride_disp,
                                     int rows, int cols, int D) {
    return volume_extent_elems(stride_row, stride_col, stride_disp, rows, cols, D) * volume_elem_bytes(dtype);
}

}  // namespace sgm
