// sgm_rectify_maps.h -- the host side of the rectification remap
// (sgm_rectify.hip): cv::convertMaps' conversion of float maps to
// the packed fixed-point maps the kernel reads, the valid mask that falls out
// of it, and the checks of the calls' arguments.  Plain C++ with no HIP in it,
// so that tests/cpp/rectify_maps_main.cpp can run it on the CPU under a
// sanitizer.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace sgm {

constexpr int kRectifyMaxSize = 32767;  // source rows and cols: the integer parts are s16
constexpr int kRectifyFixMin = -32768 * 32, kRectifyFixMax = 32767 * 32;

// One coordinate in 5 fraction bits: t = c * 32 (exact in fp32), NaN ->
// the lower clamp, clamped to [-32768 * 32, 32767 * 32], rounded to nearest
// with ties to even.  NaN is found by its bits: the library is built with
// -fno-honor-nans, which may fold a floating-point test for it.
inline int rectify_fix(float c) {
    const float t = c * 32.0f;
    uint32_t bits;
    memcpy(&bits, &t, sizeof(bits));
    if ((bits & 0x7fffffffu) > 0x7f800000u) return kRectifyFixMin;
    if (t <= (float)kRectifyFixMin) return kRectifyFixMin;
    if (t >= (float)kRectifyFixMax) return kRectifyFixMax;
    return (int)rintf(t);
}

// One view's maps (rows x cols floats, map_pitch floats per row) to the packed
// map and the valid mask, both dense.  Per pixel two words:
//   packed[2 k]     = (x0 & 0xffff) | (y0 << 16)    the integer parts, s16 each
//   packed[2 k + 1] = a | (b << 5)                  the fractions of x and y, 5 bits each
// with x0 = q >> 5 (arithmetic: it floors) and a = q & 31 of q = rectify_fix.
// valid = 255 where all four taps (x0, y0) .. (x0 + 1, y0 + 1) lie inside the
// src_rows x src_cols source, else 0.
inline void rectify_convert(const float *map_x, const float *map_y, int map_pitch, int rows, int cols,
                            int src_rows, int src_cols, uint32_t *packed, uint8_t *valid) {
    for (int i = 0; i < rows; ++i) {
        const float *mx = map_x + (size_t)i * map_pitch, *my = map_y + (size_t)i * map_pitch;
        uint32_t *out = packed + 2 * (size_t)i * cols;
        uint8_t *ok = valid + (size_t)i * cols;
        for (int j = 0; j < cols; ++j) {
            const int qx = rectify_fix(mx[j]), qy = rectify_fix(my[j]);
            const int x0 = qx >> 5, y0 = qy >> 5;
            out[2 * j] = ((uint32_t)x0 & 0xffffu) | ((uint32_t)y0 << 16);
            out[2 * j + 1] = (uint32_t)(qx & 31) | ((uint32_t)(qy & 31) << 5);
            ok[j] = x0 >= 0 && x0 + 1 < src_cols && y0 >= 0 && y0 + 1 < src_rows ? 255 : 0;
        }
    }
}

// sgm_set_rectify's arguments: (0, 0) with no map switches it off; otherwise
// both sizes in [1, 32767], four maps, rows no narrower than the handle's
// width.  Returns false with the reason in why.
inline bool rectify_args_ok(int src_rows, int src_cols, const float *const maps[4], int map_pitch, int width,
                            char *why, size_t n) {
    const bool any = maps[0] || maps[1] || maps[2] || maps[3];
    if (src_rows == 0 && src_cols == 0 && !any) return true;
    if ((src_rows == 0) != (src_cols == 0)) {
        snprintf(why, n, "both sizes are zero (off) or neither, got %d x %d", src_rows, src_cols);
        return false;
    }
    if (src_rows < 1 || src_rows > kRectifyMaxSize || src_cols < 1 || src_cols > kRectifyMaxSize) {
        snprintf(why, n, "source sizes must be in [1, %d] (or 0 x 0 with no maps: off), got %d x %d",
                 kRectifyMaxSize, src_rows, src_cols);
        return false;
    }
    if (!maps[0] || !maps[1] || !maps[2] || !maps[3]) {
        snprintf(why, n, "NULL map (both views' map_x and map_y are needed)");
        return false;
    }
    if (map_pitch < width) {
        snprintf(why, n, "map_pitch %d below the width %d", map_pitch, width);
        return false;
    }
    return true;
}

// One remap call's view and pitches.
inline bool rectify_call_ok(int view, int src_pitch, int src_cols, int dst_pitch, int width, char *why,
                            size_t n) {
    if (view != 0 && view != 1) {
        snprintf(why, n, "view must be 0 (left) or 1 (right), got %d", view);
        return false;
    }
    if (src_pitch < src_cols) {
        snprintf(why, n, "src_pitch %d below src_cols %d", src_pitch, src_cols);
        return false;
    }
    if (dst_pitch < width) {
        snprintf(why, n, "dst_pitch %d below the width %d", dst_pitch, width);
        return false;
    }
    return true;
}

}  // namespace sgm
