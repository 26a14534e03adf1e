// sgm_fill_select.h -- the per-pixel part of the occlusion-aware hole filling
// (Hirschmueller 2008, 2.6): which values count as valid, the
// class test against the right view's map, the sort of the up to 8 directional
// candidates and the pick, with the code of the fill mask.  The kernels
// (sgm_fill.hip) own the ray marches and the memory accesses and run every
// pixel's decision through these functions.
// Plain C++ with no HIP in it (g++ compiles it for tests/cpp/fill_select_main.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SGM_FILL_FN __host__ __device__ __forceinline__
#else
#define SGM_FILL_FN inline
#endif

namespace sgm {

// sgm_set_fill's modes (SGM_FILL_*)
constexpr int kFillOff = 0, kFillBackground = 1, kFillInterpolate = 2;
// the fill mask's codes
constexpr uint8_t kFillMeasured = 0, kFillOcclusion = 1, kFillMismatch = 2, kFillInvalid = 3;

// "no candidate": what a ray that left the image carries, and the sort's padding
SGM_FILL_FN float fill_none() { return __builtin_huge_valf(); }

// The post filter's own test, v <= D + min_disp - 1 (lim), with a NaN invalid.
// The NaN test is on the bit pattern: the library is built with
// -fno-honor-nans, under which a float comparison may not be relied on for it.
SGM_FILL_FN bool fill_valid(float v, float lim) {
    uint32_t b;
    __builtin_memcpy(&b, &v, sizeof(b));
    if ((b & 0x7fffffffu) > 0x7f800000u) return false;
    return v <= lim;
}

SGM_FILL_FN void fill_cswap(float &a, float &b) {
    const float lo = b < a ? b : a, hi = b < a ? a : b;
    a = lo;
    b = hi;
}

// Batcher's odd-even merge sort of 8 values, ascending: 19 compare-exchanges
SGM_FILL_FN void fill_sort8(float (&c)[8]) {
    fill_cswap(c[0], c[1]); fill_cswap(c[2], c[3]); fill_cswap(c[4], c[5]); fill_cswap(c[6], c[7]);
    fill_cswap(c[0], c[2]); fill_cswap(c[1], c[3]); fill_cswap(c[4], c[6]); fill_cswap(c[5], c[7]);
    fill_cswap(c[1], c[2]); fill_cswap(c[5], c[6]);
    fill_cswap(c[0], c[4]); fill_cswap(c[1], c[5]); fill_cswap(c[2], c[6]); fill_cswap(c[3], c[7]);
    fill_cswap(c[2], c[4]); fill_cswap(c[3], c[5]);
    fill_cswap(c[1], c[2]); fill_cswap(c[3], c[4]); fill_cswap(c[5], c[6]);
}

// The class test of the invalid pixel in column j: a mismatch iff some integer
// disparity d in [min_disp, min_disp + D) leads to a valid pixel jr = j - d /
// scale >= 0 of the right view's row whose value is within lr_max_diff of d
// (one fp32 subtraction).  right(jr): the right map's value in column jr of the
// pixel's row.  (jr falls as d grows: the first negative one ends the search.)
template <typename R>
SGM_FILL_FN bool fill_mismatch(R &&right, int j, int min_disp, int D, int scale, float lim, float lr_max_diff) {
    for (int d = min_disp; d < min_disp + D; ++d) {
        const int jr = j - d / scale;
        if (jr < 0) break;
        const float r = right(jr);
        if (fill_valid(r, lim) && __builtin_fabsf(r - (float)d) <= lr_max_diff) return true;
    }
    return false;
}

// The value and the mask code of an INVALID pixel from its 8 directional
// candidates (any order; fill_none() where a ray found nothing) and its class:
// k = the candidates found; the occlusion takes the second lowest (the
// background), sorted[min(1, k - 1)], the mismatch the upper median sorted[k / 2]
// (as Solver::post_filter picks v[valid_cnt / 2]); k = 0 leaves `inv`.
SGM_FILL_FN float fill_pick(float (&c)[8], float lim, bool mismatch, float inv, uint8_t *code) {
    int k = 0;
    for (int t = 0; t < 8; ++t) {
        const bool ok = fill_valid(c[t], lim);
        k += ok ? 1 : 0;
        if (!ok) c[t] = fill_none();
    }
    if (k == 0) {
        *code = kFillInvalid;
        return inv;
    }
    fill_sort8(c);
    const int at = mismatch ? k / 2 : (k > 1 ? 1 : 0);
    *code = mismatch ? kFillMismatch : kFillOcclusion;
    float v = c[0];
    for (int t = 1; t < 8; ++t)  // (a select chain, not an indexed register array)
        if (t == at) v = c[t];
    return v;
}

}  // namespace sgm
