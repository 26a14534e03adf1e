// sgm_volume_filter.hip -- cost_horizontal_filter (Solver.cpp:296-330) over a
// finished cost volume in device memory.
//
// The census frames run this filter inside the kernel that builds their raw
// costs from census words staged in LDS (cost_h_body, sgm_cost.hip).  The
// volume entry of the pipeline -- a caller's volume (sgm_aggregate_device), a
// SAD or SSD window cost -- has the raw costs as a dense fp32 HWD volume
// instead, and this kernel runs the same recursion (HFilter, sgm_cost_iir.h: an
// IIR, not a box filter) reading them from there: step t = 0 .. T-1,
// T = W - 2 (WIN/2), writes column LAG + t (LAG = WIN - WIN/2 - 1); columns
// below LAG and from LAG + T on keep their raw values.
//
// Shape: cost_h's.  One lane per (row, d) chain, lanes along d, so every load
// and store of a wave is one whole 256-byte line (128 bytes per half wave at
// D = 32).  A view has only H * D chains (750 waves at 375 x 1242 x 128), less
// than one wave per SIMD, so nothing hides a load's latency but the chain
// itself: the main loop runs blocks of kVolfU branch-free steps over a register
// ring of kVolfU raw values, each step refilling the slot it consumed with the
// value kVolfU steps ahead.  Positions past the row's end are clamped to its last
// column (a scalar min per load; the value feeds nothing), which lets the tail
// run from prefetched values too instead of one exposed load per step.
//
// In place (in == out) is safe: within a chain every load is of a column above
// every store made so far (the prefetch only widens that gap; the clamped loads
// read the last column, which the filter never writes), and chains share no
// element.  The pointers are therefore not __restrict__, which also pins each
// block's loads above its stores.
// No address depends on a cost value.
#include "sgm_device.h"

namespace sgm {
namespace {

#ifndef VOLF_U
#define VOLF_U 32
#endif
constexpr int kVolfU = VOLF_U;
static_assert(kVolfU >= 1 && kVolfU <= 32, "2 * kVolfU - 1 memory operations stay in flight: vmcnt holds 63");

template <bool NT>
__device__ __forceinline__ void volf_store(float v, float *p) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// DC: D as a compile-time constant (0: run-time D), as cost_h's.  NT: the output
// by non-temporal stores (the Ch volume vfwd reads once).  Workgroup z = view.
template <int WIN, int DC, bool NT>
__global__ __launch_bounds__(256) void vol_hfilter_kernel(const float *in0, float *out0, const float *in1,
                                                          float *out1, int H, int W, int D) {
    const bool second = __builtin_amdgcn_workgroup_id_z() != 0;
    const float *in = second ? in1 : in0;
    float *out = second ? out1 : out0;
    const int Dn = DC ? DC : D;
    const int R = 256 / Dn;  // rows per workgroup
    const int r = tid_x() / Dn, d = tid_x() - r * Dn;
    const int i = bid_x() * R + r;
    if (i >= H) return;
    const size_t DS = (size_t)Dn;
    const float *p = in + (size_t)i * W * DS + d;
    float *o = out + (size_t)i * W * DS + d;
    const bool copy = in != out;  // the border columns of another volume are written too

    constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1, U = kVolfU;
    constexpr int TAIL = 2 * HALF - LAG;  // raw columns after the last output: LAG + T .. W - 1
    const int T = W - 2 * HALF;
    // a raw value at position j, clamped to the row (j is wave-uniform)
    auto raw = [&](int j) { return p[(size_t)(j < W - 1 ? j : W - 1) * DS]; };

    float first[WIN];
#pragma unroll
    for (int k = 0; k < WIN; ++k) first[k] = p[(size_t)k * DS];
    float cur[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = raw(WIN + u);
    HFilter<WIN> f;  // the recursion: sgm_cost_iir.h
    f.init(first);
    if (copy) {
#pragma unroll
        for (int q = 0; q < LAG; ++q) volf_store<NT>(first[q], o + (size_t)q * DS);
    }
    auto step = [&](int t, float rw) {
        const float v = f.out();
        volf_store<NT>(v, o + (size_t)(LAG + t) * DS);
        f.advance(v, rw);
    };
    // steps t < T-1 write and update, the last step only writes.  Each step refills the ring slot
    // it consumed with the value U steps ahead: a load is followed by 2U - 1 younger loads and
    // stores before its value is needed, which a wave's in-order memory counter (63 at most)
    // lets stay in flight, so no step waits for a store's acknowledgement
    int t = 0;
    for (; t + U <= T - 1; t += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            step(t + u, cur[u]);
            cur[u] = raw(WIN + t + U + u);
        }
    }
    // the last border columns, requested before the tail's steps
    float last[TAIL > 0 ? TAIL : 1];
    if (copy) {
#pragma unroll
        for (int q = 0; q < TAIL; ++q) last[q] = p[(size_t)(LAG + T + q) * DS];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (t + u < T - 1) step(t + u, cur[u]);
    if (T >= 1) volf_store<NT>(f.out(), o + (size_t)(LAG + T - 1) * DS);
    if (copy) {
#pragma unroll
        for (int q = 0; q < TAIL; ++q) volf_store<NT>(last[q], o + (size_t)(LAG + T + q) * DS);
    }
}

template <int WIN, int DC>
void launch_t(const float *const *in, float *const *out, int nviews, bool nt, Geom g, hipStream_t st) {
    const int R = 256 / g.D;
    const dim3 grid((g.H + R - 1) / R, 1, nviews);
    const float *in1 = nviews == 2 ? in[1] : in[0];
    float *out1 = nviews == 2 ? out[1] : out[0];
    if (nt)
        vol_hfilter_kernel<WIN, DC, true><<<grid, 256, 0, st>>>(in[0], out[0], in1, out1, g.H, g.W, g.D);
    else
        vol_hfilter_kernel<WIN, DC, false><<<grid, 256, 0, st>>>(in[0], out[0], in1, out1, g.H, g.W, g.D);
}

}  // namespace

int volume_filter_block() { return kVolfU; }

hipError_t launch_volume_hfilter(const float *const *in, float *const *out, int nviews, bool nt, Geom g,
                                 hipStream_t st) {
    const int win = 5 / g.scale;  // COST_WIN_W / scale (SGM.cpp:66-72)
    if ((nviews != 1 && nviews != 2) || (g.scale != 1 && g.scale != 2) || g.W < win || g.H < 1 ||
        (g.D != 32 && g.D != 64 && g.D != 128 && g.D != 256))
        return hipErrorInvalidValue;
    for (int v = 0; v < nviews; ++v)
        if (!in[v] || !out[v]) return hipErrorInvalidValue;
    if (g.scale == 1) {
        if (g.D == 128) launch_t<5, 128>(in, out, nviews, nt, g, st);
        else launch_t<5, 0>(in, out, nviews, nt, g, st);
    } else {
        if (g.D == 128) launch_t<2, 128>(in, out, nviews, nt, g, st);
        else launch_t<2, 0>(in, out, nviews, nt, g, st);
    }
    return hipGetLastError();
}

}  // namespace sgm
