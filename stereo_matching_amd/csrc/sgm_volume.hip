// sgm_volume.hip -- a caller's cost volume into the library's own.
//
// One launch re-lays a strided fp32 or fp16 rows x cols x D volume out as the
// dense fp32 HWD volume the path passes read, and derives the right view's
// volume from it:
//   C_R[i, j, d] = C_L[i, min(j + (d + min_disp) / scale, cols - 1), d]
// (build_dsi_from_table_beta's column index, Solver.cpp:239).  A workgroup of
// four waves takes one row, 64 columns and 64 disparities (32 at D = 32) and
// writes the views it was asked for one after the other, so that the right
// view's reads find the left view's in the caches.
//
// DHW source (stride_col == 1): each plane's 64-column segment is read along j,
// 16 bytes per lane where the segment's address allows (else element by
// element), the right view's at column offset (d + min_disp) / scale with the
// clamp; the tile is transposed through LDS (rows of 65 words; the lane
// mappings below keep every ds access conflict-free) and leaves as 16-byte
// stores along d.
// HWD source (stride_disp == 1): the left view is a pitched copy, 16 bytes per
// lane in and out.  The right view gathers (j + shift(d), d): the span of
// columns the tile needs (64 + the chunk's shift range) is staged in LDS by
// 16-byte loads along d, then read back skewed, one disparity per lane
// (conflict-free at rows of DC words: the bank is d mod 32), and stored as
// whole 256-byte lines.
// No address depends on a cost value.
#include "sgm_internal.h"

#include "sgm_volume_args.h"

namespace sgm {
namespace {

constexpr int kTJ = 64;  // columns per workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct VolArgs {
    const void *src;
    long long sr, sc, sd;  // strides in elements
    float *dst[2];         // the left and the right view's volume (null: not wanted)
    int H, W, D;
    int sshift;            // log2(scale)
    int min_disp;
    int dst_vec;           // both destinations are 16-byte aligned
};

template <typename T>
struct VecOf;
template <>
struct VecOf<float> {
    typedef f32x4 type;
};
template <>
struct VecOf<_Float16> {
    typedef f16x8 type;
};

// V elements from p: one 16-byte load where p is aligned, else V loads
template <typename T, int V>
__device__ __forceinline__ void load_vec(const T *p, float (&x)[V]) {
    if (((uintptr_t)p & 15) == 0) {
        const typename VecOf<T>::type v = *reinterpret_cast<const typename VecOf<T>::type *>(p);
#pragma unroll
        for (int e = 0; e < V; ++e) x[e] = (float)v[e];
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) x[e] = (float)p[e];
    }
}

__device__ __forceinline__ void store4(float *o, const float *x, int vec) {
    if (vec) {
        *reinterpret_cast<f32x4 *>(o) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
        o[0] = x[0];
        o[1] = x[1];
        o[2] = x[2];
        o[3] = x[3];
    }
}

// DHW: element (i, j, d) at src[i * sr + d * sd + j]
template <typename T, int DC>
__global__ __launch_bounds__(256) void vol_dhw_kernel(VolArgs a) {
    constexpr int V = 16 / sizeof(T);  // elements per 16-byte load
    constexpr int AH = kTJ / V / 2;    // vectors of a segment per half wave (8 | 4)
    constexpr int LD = kTJ + 1;
    __shared__ float tile[DC * LD];
    const int ntj = (a.W + kTJ - 1) / kTJ;
    const int i = blockIdx.x / ntj, j0 = (blockIdx.x % ntj) * kTJ, d0 = blockIdx.y * DC;
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    // load phase: lane -> (vector la of the segment, plane lb of V); a half wave's 32 lanes
    // write banks lb + V * (la % AH) + e, all different (ds_write_b32: 32 banks)
    const int la = (l % AH) + AH * (l >> 5), lb = (l & 31) / AH;
    // store phase: lane -> (four disparities 4 q .., column js); a half wave reads banks
    // 4 q + js + e over q = 0..7, js = 0..3, all different
    constexpr int NQ = DC / 4;
    const int q = NQ == 16 ? (l & 7) + 8 * (l >> 5) : (l & 7);
    const int js = NQ == 16 ? (l & 31) >> 3 : l >> 3;
    constexpr int CW = NQ == 16 ? 4 : 8;  // columns per wave and step
    const T *src = static_cast<const T *>(a.src) + (long long)i * a.sr;
    for (int v = 0; v < 2; ++v) {
        float *dst = a.dst[v];
        if (!dst) continue;
        for (int dd = w * V + lb; dd < DC; dd += 4 * V) {
            const int d = d0 + dd;
            const int sh = v ? (d + a.min_disp) >> a.sshift : 0;
            const T *row = src + (long long)d * a.sd;
            const int jj = la * V, c = j0 + jj + sh;
            float x[V];
            if (c + V <= a.W) {
                load_vec<T, V>(row + c, x);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int ce = c + e < a.W ? c + e : a.W - 1;
                    x[e] = j0 + jj + e < a.W ? (float)row[ce] : 0.0f;
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) tile[dd * LD + jj + e] = x[e];
        }
        __syncthreads();
        for (int jj = w * CW + js; jj < kTJ; jj += 4 * CW) {
            const int j = j0 + jj;
            if (j < a.W) {
                float x[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = tile[(4 * q + e) * LD + jj];
                store4(dst + ((long long)i * a.W + j) * a.D + d0 + 4 * q, x, a.dst_vec);
            }
        }
        __syncthreads();
    }
}

// HWD: element (i, j, d) at src[i * sr + j * sc + d]
template <typename T, int DC>
__global__ __launch_bounds__(256) void vol_hwd_kernel(VolArgs a) {
    constexpr int V = 16 / sizeof(T);
    constexpr int NA = DC / V;  // 16-byte loads per column of the chunk
    __shared__ __attribute__((aligned(16))) float tile[(kTJ + DC) * DC];
    const int ntj = (a.W + kTJ - 1) / kTJ;
    const int i = blockIdx.x / ntj, j0 = (blockIdx.x % ntj) * kTJ, d0 = blockIdx.y * DC;
    const int t = threadIdx.x;
    const T *src = static_cast<const T *>(a.src) + (long long)i * a.sr + d0;
    if (float *dst = a.dst[0]) {
        for (int idx = t; idx < kTJ * NA; idx += 256) {
            const int j = j0 + idx / NA, dd = (idx % NA) * V;
            if (j >= a.W) break;
            float x[V];
            load_vec<T, V>(src + (long long)j * a.sc + dd, x);
            float *o = dst + ((long long)i * a.W + j) * a.D + d0 + dd;
#pragma unroll
            for (int e = 0; e < V; e += 4) store4(o + e, x + e, a.dst_vec);
        }
    }
    if (float *dst = a.dst[1]) {
        // the chunk's span: source columns c_lo .. c_lo + nc - 1, each clamped to W - 1
        const int sh0 = (d0 + a.min_disp) >> a.sshift;
        const int nc = kTJ + ((d0 + DC - 1 + a.min_disp) >> a.sshift) - sh0;  // <= kTJ + DC - 1
        const int c_lo = j0 + sh0;
        for (int idx = t; idx < nc * NA; idx += 256) {
            const int cc = idx / NA, dd = (idx % NA) * V;
            const int c = c_lo + cc < a.W ? c_lo + cc : a.W - 1;
            float x[V];
            load_vec<T, V>(src + (long long)c * a.sc + dd, x);
#pragma unroll
            for (int e = 0; e < V; e += 4)
                *reinterpret_cast<f32x4 *>(&tile[cc * DC + dd + e]) = f32x4{x[e], x[e + 1], x[e + 2], x[e + 3]};
        }
        __syncthreads();
        for (int idx = t; idx < kTJ * DC; idx += 256) {
            const int jj = idx / DC, dd = idx % DC, j = j0 + jj;
            if (j >= a.W) break;
            const int cc = jj + ((d0 + dd + a.min_disp) >> a.sshift) - sh0;
            dst[((long long)i * a.W + j) * a.D + d0 + dd] = tile[cc * DC + dd];
        }
    }
}

template <typename T, int DC>
hipError_t launch_t(bool hwd, const VolArgs &a, hipStream_t st) {
    const int ntj = (a.W + kTJ - 1) / kTJ;
    const dim3 grid((unsigned)((long long)a.H * ntj), (unsigned)(a.D / DC));
    if (hwd)
        hipLaunchKernelGGL((vol_hwd_kernel<T, DC>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((vol_dhw_kernel<T, DC>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_volume_import(const void *src, int dtype, long long stride_row, long long stride_col,
                                long long stride_disp, float *dst_l, float *dst_r, int min_disp, Geom g,
                                hipStream_t st) {
    if (!src || (!dst_l && !dst_r) || (long long)g.H * ((g.W + kTJ - 1) / kTJ) > 0x7fffffffLL)
        return hipErrorInvalidValue;
    VolArgs a{};
    a.src = src;
    a.sr = stride_row;
    a.sc = stride_col;
    a.sd = stride_disp;
    a.dst[0] = dst_l;
    a.dst[1] = dst_r;
    a.H = g.H;
    a.W = g.W;
    a.D = g.D;
    a.sshift = g.scale == 2 ? 1 : 0;
    a.min_disp = min_disp;
    a.dst_vec = (((uintptr_t)dst_l | (uintptr_t)dst_r) & 15) == 0;
    const bool hwd = stride_disp == 1;
    const bool f16 = dtype == kVolF16;
    if (g.D == 32)
        return f16 ? launch_t<_Float16, 32>(hwd, a, st) : launch_t<float, 32>(hwd, a, st);
    return f16 ? launch_t<_Float16, 64>(hwd, a, st) : launch_t<float, 64>(hwd, a, st);
}

}  // namespace sgm
