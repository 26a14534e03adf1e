// sgm_gray.hip -- colour camera images to the grey the frame works on: 8-bit
// interleaved BGR8 / RGB8 / BGRA8 / RGBA8 to one channel, pinned as DESIGN.md 5l
// states it and tests/gray_recipe.py restates it (sgm_pix.h holds the formula;
// the fused input stages, sgm_resize.hip and sgm_rectify.hip, convert each tap
// with the same function).
//
// A pure streaming kernel, one launch for one or both views (grid z, as
// resize_kernel).  A lane converts four neighbouring pixels of a row: it loads
// their 12 bytes as three dwords (one dwordx3; 16 as one dwordx4), and stores the four grey
// bytes as one dword, so a wave reads 768 (1024) and writes 256 contiguous
// bytes per row.  The caller's pointers and pitches may have any alignment: the
// wide accesses are unaligned-safe ones (global memory takes dwords at any byte
// address), a row's last one to three pixels go byte by byte, and nothing is
// read past cols x bytes per pixel of a row or written past cols.  A workgroup
// covers 256 columns and 16 rows, each wave four rows whose loads are issued
// before the first is converted.  Nothing is read back, allocated or copied per
// call.
#include "sgm_device.h"
#include "sgm_gray_args.h"
#include "sgm_pix.h"

namespace sgm {
namespace {

constexpr int kGrayPx = 4;               // pixels per lane and row
constexpr int kGrayCols = 64 * kGrayPx;  // columns per workgroup
constexpr int kGrayRows = 16;            // rows per workgroup (4 per wave)

struct GrayViews {
    const uint8_t *src[2];
    uint8_t *dst[2];
};

// byte i of the lane's dwords
template <int N>
__device__ __forceinline__ int byte_of(const uint32_t (&w)[N], int i) {
    return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
}

template <int F>
__global__ __launch_bounds__(256) void gray_kernel(GrayViews gv, int rows, int cols, int sp, int dp) {
    constexpr int bpp = Pix<F>::bpp, red = Pix<F>::red;
    const int z = (int)__builtin_amdgcn_workgroup_id_z();
    const uint8_t *__restrict__ src = gv.src[z];
    uint8_t *__restrict__ dst = gv.dst[z];
    const int lane = tid_x() & 63, wave = wave_id();
    const int x = (bid_x() * 64 + lane) * kGrayPx;
    const int y_first = bid_y() * kGrayRows + wave * 4;
    if (x >= cols) return;
    if (x + kGrayPx > cols) {  // the row's last 1..3 pixels: bytes
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y_first + r;
            if (y >= rows) break;
            for (int k = x; k < cols; ++k)
                dst[(size_t)y * dp + k] = (uint8_t)gray_px<F>(src + (size_t)y * sp + (size_t)k * bpp);
        }
        return;
    }
    uint32_t w[4][bpp];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = y_first + r < rows ? y_first + r : rows - 1;  // (a row past the end re-reads the last)
        __builtin_memcpy(w[r], src + (size_t)y * sp + (size_t)x * bpp, kGrayPx * bpp);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = y_first + r;
        if (y >= rows) break;
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < kGrayPx; ++k) {
            const int v = gray_y(byte_of(w[r], k * bpp + red), byte_of(w[r], k * bpp + 1),
                                 byte_of(w[r], k * bpp + 2 - red));
            out |= (uint32_t)v << (8 * k);
        }
        __builtin_memcpy(dst + (size_t)y * dp + x, &out, 4);
    }
}

}  // namespace

hipError_t launch_gray(int fmt, const uint8_t *const *src, int rows, int cols, int src_pitch,
                       uint8_t *const *dst, int dst_pitch, int nviews, hipStream_t st) {
    GrayViews gv{};
    for (int v = 0; v < nviews; ++v) {
        gv.src[v] = src[v];
        gv.dst[v] = dst[v];
    }
    const dim3 grid((unsigned)((cols + kGrayCols - 1) / kGrayCols),
                    (unsigned)((rows + kGrayRows - 1) / kGrayRows), (unsigned)nviews);
#define SGM_GRAY_LAUNCH(F) \
    hipLaunchKernelGGL(gray_kernel<F>, grid, dim3(256), 0, st, gv, rows, cols, src_pitch, dst_pitch)
    switch (fmt) {
    case 1: SGM_GRAY_LAUNCH(1); break;
    case 2: SGM_GRAY_LAUNCH(2); break;
    case 3: SGM_GRAY_LAUNCH(3); break;
    case 4: SGM_GRAY_LAUNCH(4); break;
    default: return hipErrorInvalidValue;  // (grey included: there is no copy kernel to fall back on)
    }
#undef SGM_GRAY_LAUNCH
    return hipGetLastError();
}

}  // namespace sgm
