// sgm_resize.hip -- the node's cv::resize(img, img, Size(w, h)) (node.cpp:75-76)
// on the GPU: 8-bit, one channel, INTER_LINEAR in OpenCV's fixed-point form,
// pinned as DESIGN.md 5j states it and tests/resize_recipe.py restates it.
//
//   exact half size: the 2x2 mean (a + b + c + d + 2) >> 2 (OpenCV's switch to
//     its area path; the sky detector's decimation, sgm_sky.hip);
//   otherwise, per destination column dx (rows alike):
//     fx = (float)((dx + 0.5) * scale_x - 0.5)   (double, unfused, rounded once)
//     sx = floor(fx), fx -= sx; clamped to [0, sw - 1] with fx = 0 at the clamps
//     a0 = rint((1 - fx) * 2048), a1 = rint(fx * 2048)      (s16, ties to even)
//     Hrow(y, dx) = src(y, sx) * a0 + src(y, sx + 1) * a1   (int32; no read at a1 = 0)
//     dst = (((b0 * (Hrow(sy) >> 4)) >> 16) + ((b1 * (Hrow(sy + 1) >> 4)) >> 16) + 2) >> 2
//
// One launch for one or both views (grid z).  A workgroup covers 64
// destination columns and 16 rows: each lane computes its column's
// coefficients once (gfx950 runs fp64 at the fp32 rate; -ffp-contract=off
// keeps the expression unfused), each wave walks 4 rows whose coefficients are
// wave-uniform.  Nothing is read back, allocated or copied per call.
//
// The kernel is a template over the source's pixel format (sgm_pix.h, DESIGN.md
// 5l): a colour source's taps are converted to grey as they are read, which is
// bit-equal to resizing the converted image; format 0 (grey) is the plain byte
// load.
#include "sgm_device.h"
#include "sgm_pix.h"

namespace sgm {
namespace {

constexpr int kResizeCols = 64;  // destination columns per workgroup (one per lane)
constexpr int kResizeRows = 16;  // destination rows per workgroup (4 per wave)

struct ResizeViews {
    const uint8_t *src[2];
    uint8_t *dst[2];
};

__device__ __forceinline__ int sat_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// The source index and the two fixed-point weights of destination index d on
// an axis of n source pixels.
__device__ __forceinline__ void resize_coef(int d, double scale, int n, int &s, int &c0, int &c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    c0 = sat_s16((int)rintf((1.f - f) * 2048.f));
    c1 = sat_s16((int)rintf(f * 2048.f));
}

template <int F>
__global__ __launch_bounds__(256) void resize_kernel(ResizeViews rv, int sh, int sw, int sp, int dh,
                                                     int dw, int dp, double scale_x, double scale_y,
                                                     int half) {
    constexpr int bpp = Pix<F>::bpp;
    const int z = (int)__builtin_amdgcn_workgroup_id_z();
    const uint8_t *__restrict__ src = rv.src[z];
    uint8_t *__restrict__ dst = rv.dst[z];
    const int lane = tid_x() & 63, wave = wave_id();
    const int dx = bid_x() * kResizeCols + lane;
    const int y0 = bid_y() * kResizeRows + wave * 4;
    if (dx >= dw) return;
    if (half) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int dy = y0 + r;
            if (dy >= dh) break;
            const uint8_t *a = src + (size_t)(2 * dy) * sp + 2 * dx * bpp, *b = a + sp;
            dst[(size_t)dy * dp + dx] =
                (uint8_t)((gray_px<F>(a) + gray_px<F>(a + bpp) + gray_px<F>(b) + gray_px<F>(b + bpp) + 2) >> 2);
        }
        return;
    }
    int sx, a0, a1;
    resize_coef(dx, scale_x, sw, sx, a0, a1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int dy = y0 + r;
        if (dy >= dh) break;
        int sy, b0, b1;
        resize_coef(dy, scale_y, sh, sy, b0, b1);
        sy = uniform(sy);
        b0 = uniform(b0);
        b1 = uniform(b1);
        const int sy1 = sy + 1 < sh ? sy + 1 : sh - 1;
        const uint8_t *p0 = src + (size_t)sy * sp + sx * bpp, *p1 = src + (size_t)sy1 * sp + sx * bpp;
        int h0 = gray_px<F>(p0) * a0, h1 = gray_px<F>(p1) * a0;
        if (a1 != 0) {  // (the clamped right edge reads no pixel past the row)
            h0 += gray_px<F>(p0 + bpp) * a1;
            h1 += gray_px<F>(p1 + bpp) * a1;
        }
        const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        dst[(size_t)dy * dp + dx] = (uint8_t)v;
    }
}

}  // namespace

hipError_t launch_resize(const uint8_t *const *src, int src_rows, int src_cols, int src_pitch,
                         uint8_t *const *dst, int dst_rows, int dst_cols, int dst_pitch, int nviews,
                         hipStream_t st, int fmt) {
    ResizeViews rv{};
    for (int v = 0; v < nviews; ++v) {
        rv.src[v] = src[v];
        rv.dst[v] = dst[v];
    }
    const ResizeScale sc = resize_scale(src_rows, src_cols, dst_rows, dst_cols);
    const dim3 grid((unsigned)((dst_cols + kResizeCols - 1) / kResizeCols),
                    (unsigned)((dst_rows + kResizeRows - 1) / kResizeRows), (unsigned)nviews);
#define SGM_RESIZE_LAUNCH(F)                                                                        \
    hipLaunchKernelGGL(resize_kernel<F>, grid, dim3(256), 0, st, rv, src_rows, src_cols, src_pitch, \
                       dst_rows, dst_cols, dst_pitch, sc.x, sc.y, sc.half)
    SGM_PIX_DISPATCH(fmt, SGM_RESIZE_LAUNCH);
#undef SGM_RESIZE_LAUNCH
    return hipGetLastError();
}

}  // namespace sgm
