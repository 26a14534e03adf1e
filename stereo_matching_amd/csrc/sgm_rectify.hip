// sgm_rectify.hip -- rectification of camera images on the GPU: cv::remap for
// 8-bit, one channel, INTER_LINEAR, BORDER_CONSTANT 0 over maps converted by
// cv::convertMaps' fixed-point form (5 fraction bits), pinned as DESIGN.md 5k
// states it and tests/rectify_recipe.py restates it.
//
//   per destination pixel the packed map (sgm_rectify_maps.h, built on the host
//   when the maps are set) holds the source position's integer parts x0, y0
//   (s16 each, one word) and its fractions a, b (5 bits each, a second word);
//   S(y, x) is the source pixel, or 0 outside the source, each tap on its own:
//     dst = ((32-a)*(32-b)*S(y0,x0) + a*(32-b)*S(y0,x0+1)
//          + (32-a)*b*S(y0+1,x0)    + a*b*S(y0+1,x0+1) + 512) >> 10
//
// One launch for one or both views (grid z, as resize_kernel).  A workgroup
// covers 64 destination columns and 16 rows, lanes along x: each wave reads
// 512 contiguous bytes of map per row (one dwordx2 per lane) and stores 64
// contiguous bytes; a rectification map is smooth, so a wave's four byte
// gathers fall in a few cache lines of two source rows.  A tap outside the
// source issues no load.  Nothing is read back, allocated or copied per call.
//
// The kernel is a template over the source's pixel format (sgm_pix.h, DESIGN.md
// 5l): a colour source's taps are converted to grey as they are read, which is
// bit-equal to remapping the converted image (a tap outside is still 0 and
// still issues no load); format 0 (grey) is the plain byte load.
#include "sgm_device.h"
#include "sgm_pix.h"

namespace sgm {
namespace {

constexpr int kRectifyCols = 64;  // destination columns per workgroup (one per lane)
constexpr int kRectifyRows = 16;  // destination rows per workgroup (4 per wave)

struct RectifyViews {
    const uint8_t *src[2];
    const uint2 *map[2];
    uint8_t *dst[2];
};

template <int F>
__global__ __launch_bounds__(256) void rectify_kernel(RectifyViews rv, int sh, int sw, int sp, int dh,
                                                      int dw, int dp) {
    constexpr int bpp = Pix<F>::bpp;
    const int z = (int)__builtin_amdgcn_workgroup_id_z();
    const uint8_t *__restrict__ src = rv.src[z];
    const uint2 *__restrict__ map = rv.map[z];
    uint8_t *__restrict__ dst = rv.dst[z];
    const int lane = tid_x() & 63, wave = wave_id();
    const int dx = bid_x() * kRectifyCols + lane;
    const int y_first = bid_y() * kRectifyRows + wave * 4;
    if (dx >= dw) return;
    // the wave's map entries first: four independent loads in flight
    uint2 m[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int dy = y_first + r < dh ? y_first + r : dh - 1;  // (a row past the end re-reads the last)
        m[r] = map[(size_t)dy * dw + dx];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int dy = y_first + r;
        if (dy >= dh) break;
        const int x0 = (int)(m[r].x << 16) >> 16, y0 = (int)m[r].x >> 16;
        const int a = (int)(m[r].y & 31u), b = (int)((m[r].y >> 5) & 31u);
        // each tap tested on its own (unsigned: one compare per side pair);
        // x0, y0 in [-32768, 32767], so x0 + 1 and y0 + 1 cannot wrap
        const bool in_x0 = (unsigned)x0 < (unsigned)sw, in_x1 = (unsigned)(x0 + 1) < (unsigned)sw;
        const bool in_y0 = (unsigned)y0 < (unsigned)sh, in_y1 = (unsigned)(y0 + 1) < (unsigned)sh;
        // the tap's offset as an integer: the source is indexed under the tap's own test only
        const long long o = (long long)y0 * sp + x0 * bpp;
        int s00 = 0, s01 = 0, s10 = 0, s11 = 0;
        if (in_y0 && in_x0) s00 = gray_px<F>(src + o);
        if (in_y0 && in_x1) s01 = gray_px<F>(src + o + bpp);
        if (in_y1 && in_x0) s10 = gray_px<F>(src + o + sp);
        if (in_y1 && in_x1) s11 = gray_px<F>(src + o + sp + bpp);
        const int v = ((32 - a) * (32 - b) * s00 + a * (32 - b) * s01 + (32 - a) * b * s10 + a * b * s11 + 512) >> 10;
        dst[(size_t)dy * dp + dx] = (uint8_t)v;
    }
}

}  // namespace

hipError_t launch_rectify(const uint8_t *const *src, int src_rows, int src_cols, int src_pitch,
                          const uint32_t *const *map, uint8_t *const *dst, int dst_rows, int dst_cols,
                          int dst_pitch, int nviews, hipStream_t st, int fmt) {
    RectifyViews rv{};
    for (int v = 0; v < nviews; ++v) {
        rv.src[v] = src[v];
        rv.map[v] = reinterpret_cast<const uint2 *>(map[v]);
        rv.dst[v] = dst[v];
    }
    const dim3 grid((unsigned)((dst_cols + kRectifyCols - 1) / kRectifyCols),
                    (unsigned)((dst_rows + kRectifyRows - 1) / kRectifyRows), (unsigned)nviews);
#define SGM_RECTIFY_LAUNCH(F)                                                                        \
    hipLaunchKernelGGL(rectify_kernel<F>, grid, dim3(256), 0, st, rv, src_rows, src_cols, src_pitch, \
                       dst_rows, dst_cols, dst_pitch)
    SGM_PIX_DISPATCH(fmt, SGM_RECTIFY_LAUNCH);
#undef SGM_RECTIFY_LAUNCH
    return hipGetLastError();
}

}  // namespace sgm
