// sgm_window_cost.hip -- the reference's SAD / SSD window costs as a cost
// volume: Solver::build_dsi (Solver.cpp:96-117) over SAD and SSD
// (cost.cpp:4-59), one launch; and over CT (cost.cpp:62-96), the
// per-disparity census build_dsi calls, on the same tile (window_cost_ct_kernel).
//
//   AD(y, x, d)  = |L[y][x] - R[y][max(x - (d + min_disp) / scale, 0)]|   (SSD: its square)
//   C[i][j][d]   = (sum over the (2 hh + 1) x (2 hw + 1) taps of
//                   AD(clamp(i + a, 0, H - 1), clamp(j + b, 0, W - 1), d)) / win_h / win_w
//
// The output is the library's dense fp32 HWD volume.  A workgroup of 256 lanes
// takes kWinCostBandRows rows, kWinCostTileCols columns and DC disparities (64;
// 32 at D = 32): lane = disparity, so a store is a whole 256-byte line (128 at
// D = 32, two columns per wave), and each group of DC lanes owns NC columns.
// The band's rows of L and R are staged in LDS as bytes at clamped coordinates
// (sgm_window_cost_args.h: R's span is the tile's columns plus the chunk's shift
// range), so no tap tests an edge.  Each lane keeps its NC + 2 hw column sums
// over the window's rows in registers while it walks down the band -- one AD
// added, one dropped per column and row -- and slides the window sum along its
// columns.  The sums are integers (at most 63 * 255^2: exact in any order);
// two correctly rounded divisions follow (div_win: proven against IEEE
// division over every reachable sum by tests/cpp/window_cost_args_main.cpp).
// The window is the handle's (sgm_set_window): the default 7 x 9
// with every constant at compile time, any other through the instantiation of
// its half width (window_cost_kernel's comment).  The weighted kernel
// (sgm_set_weighted, 5r) shares the tile: win_tile, stage_rows and WinLane are
// both kernels' prologue, launch_tiles and by_half_width both kernels' launch.
#include "sgm_device.h"

#include "sgm_window_cost_args.h"

namespace sgm {
namespace {

struct WinArgs {
    const uint8_t *left, *right;
    size_t rpitch;  // bytes between working-grid rows
    float *dst;
    int H, W, D;
    int min_disp;
    // a window other than the default (sgm_set_window): read only by the
    // instantiations that leave these to run time
    int scale, hh;
    float fh, rh, fw, rw;  // e_h, RN(1 / e_h), e_w, RN(1 / e_w)
};

// x / f with r = RN(1 / f): div_win's form (sgm_device.h) with the divisor at run time.
// sgm_window_cost_args.h's win_div is its host mirror, proven for every divisor 1 .. 9.
__device__ __forceinline__ float div_rt(float x, float f, float r) {
    const float q0 = x * r;
    const float e = __builtin_fmaf(-q0, f, x);
    return __builtin_fmaf(e, r, q0);
}

// A workgroup's tile: its first row, column and disparity, the chunk's largest column shift and
// the columns a staged row of R takes at this scale.
struct WinTile {
    int i0, j0, d0, s_hi, RC;
};

template <int HW, int DC>
__device__ __forceinline__ WinTile win_tile(const WinArgs &a, int SCALE) {
    const int ntj = (a.W + kWinCostTileCols - 1) / kWinCostTileCols;
    const int d0 = bid_y() * DC;
    return {(bid_x() / ntj) * kWinCostBandRows, (bid_x() % ntj) * kWinCostTileCols, d0,
            (d0 + DC - 1 + a.min_disp) / SCALE, win_r_cols(HW, SCALE, DC)};
}

// The band's rows of L and R into the kernel's LDS arrays as bytes at clamped coordinates.  SCALE,
// HH: constants in the default window's instantiations (they fold after inlining), else WinArgs'.
template <int HW>
__device__ __forceinline__ void stage_rows(const WinArgs &a, WinTile t, int SCALE, int HH, uint8_t *sl, uint8_t *sr) {
    constexpr int LC = win_l_cols(HW);
    const int NR = win_rows(HH), RC = t.RC;
    for (int idx = tid_x(); idx < NR * LC; idx += 256) {
        const int r = idx / LC, c = idx - r * LC;
        const int y = clampi(t.i0 - HH + r, 0, a.H - 1), x = clampi(t.j0 - HW + c, 0, a.W - 1);
        sl[idx] = a.left[(size_t)y * a.rpitch + (size_t)x * SCALE];
    }
    for (int idx = tid_x(); idx < NR * RC; idx += 256) {
        const int r = idx / RC, c = idx - r * RC;
        const int y = clampi(t.i0 - HH + r, 0, a.H - 1), x = win_r_col(t.j0, c, a.W, HW, t.s_hi);
        sr[idx] = a.right[(size_t)y * a.rpitch + (size_t)x * SCALE];
    }
    __syncthreads();
}

// A lane's place in the tile: its group's first tile column c0 (tile column c0 + c is image
// column j0 - HW + c0 + c: output column k of the group takes its taps k .. k + 2 HW), its
// disparity d, the columns ru[] of its taps in a staged row of R, and the tap itself.
template <int HW, int DC, bool SSD>
struct WinLane {
    static constexpr int NC = kWinCostTileCols / (256 / DC);  // columns per group of DC lanes
    static constexpr int NCA = NC + 2 * HW;                   // taps of a staged row the group reads
    static constexpr int LC = win_l_cols(HW);
    int c0, d, RC, ru[NCA];
    const uint8_t *sl, *sr;
    __device__ __forceinline__ WinLane(const WinArgs &a, WinTile t, int SCALE, const uint8_t *sl_, const uint8_t *sr_)
        : c0((tid_x() / DC) * NC), d(t.d0 + tid_x() % DC), RC(t.RC), sl(sl_), sr(sr_) {
        const int s = (d + a.min_disp) / SCALE;
#pragma unroll
        for (int c = 0; c < NCA; ++c) ru[c] = win_r_index(t.j0, c0 + c, a.W, HW, t.s_hi, s);
    }
    // AD(staged row r, the group's tap c, d)
    __device__ __forceinline__ int ad(int r, int c) const {
        const int v = (int)sl[r * LC + c0 + c] - (int)sr[r * RC + ru[c]];
        return SSD ? v * v : (v < 0 ? -v : v);
    }
};

// HW, the window's half width, sizes the register arrays and is always a template
// argument.  SCALE_T, HH_T, WH_T, WW_T are the default window's constants (the
// code of before sgm_set_window); 0, -1, 0, 0 leave the scale, the half height
// and the two divisors to WinArgs, so that one instantiation per half width
// serves every other accepted window (the staged rows are then sized for the
// largest half height and for scale 1, and indexed by the run-time strides).
template <int HW, int DC, bool SSD, int SCALE_T, int HH_T, int WH_T, int WW_T>
__global__ __launch_bounds__(256) void window_cost_kernel(WinArgs a) {
    constexpr bool FIXED = SCALE_T != 0;
    static_assert(FIXED == (HH_T >= 0) && FIXED == (WH_T != 0) && FIXED == (WW_T != 0), "all or none");
    const int SCALE = FIXED ? SCALE_T : a.scale, HH = FIXED ? HH_T : a.hh;
    using Lane = WinLane<HW, DC, SSD>;
    constexpr int RB = kWinCostBandRows, NC = Lane::NC, NCA = Lane::NCA;  // NCA column sums a group keeps
    constexpr int RC_MAX = win_r_cols(HW, FIXED ? SCALE_T : 1, DC), NR_MAX = win_rows(FIXED ? HH_T : kWinMax / 2);
    __shared__ uint8_t sl[NR_MAX * Lane::LC];
    __shared__ uint8_t sr[NR_MAX * RC_MAX];
    const WinTile t = win_tile<HW, DC>(a, SCALE);
    stage_rows<HW>(a, t, SCALE, HH, sl, sr);
    const Lane ln(a, t, SCALE, sl, sr);
    const int i0 = t.i0, j0 = t.j0, c0 = ln.c0, d = ln.d;
    int cs[NCA];
#pragma unroll
    for (int c = 0; c < NCA; ++c) {
        cs[c] = 0;
#pragma unroll
        for (int r = 0; r <= 2 * HH; ++r) cs[c] += ln.ad(r, c);
    }
    const int rows = a.H - i0 < RB ? a.H - i0 : RB;
    for (int rr = 0; rr < rows; ++rr) {
        int sum = 0;
#pragma unroll
        for (int c = 0; c <= 2 * HW; ++c) sum += cs[c];
        float *o = a.dst + ((size_t)(i0 + rr) * a.W + j0 + c0) * a.D + d;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (j0 + c0 + k < a.W) {
                if constexpr (FIXED)
                    o[(size_t)k * a.D] = div_win<WW_T>(div_win<WH_T>((float)sum));
                else
                    o[(size_t)k * a.D] = div_rt(div_rt((float)sum, a.fh, a.rh), a.fw, a.rw);
            }
            if (k + 1 < NC) sum += cs[k + 2 * HW + 1] - cs[k];
        }
        // the window moves down a row: staged row rr + 2 HH + 1 enters, rr leaves
        if (rr + 1 < rows) {
#pragma unroll
            for (int c = 0; c < NCA; ++c) cs[c] += ln.ad(rr + 2 * HH + 1, c) - ln.ad(rr, c);
        }
    }
}

// ---------------------------------------------------------------- weighted taps
//
// sgm_set_weighted: cost.cpp:19-22, :48-51 with WEIGHTED_COST on.  Every tap is
// multiplied by its Gaussian weight, so a cost is a chain of (2 hh + 1)(2 hw + 1) fp32 multiplies
// and adds in the reference's tap order (rows outer, columns inner, from 0.0f; never fused:
// -ffp-contract=off), and no two outputs share a partial sum.  The tile, the staged rows and the
// stores are window_cost_kernel's.  What is shared is the tap itself: (float)AD(row, column, d)
// does not depend on the output it feeds, so a lane converts a staged row's NCA taps once and
// feeds them to every output column of its group, and to the two output rows it carries at a
// time (staged row rr + a is window row a of output row rr and a - 1 of rr + 1).  The lane's
// outputs are paired by column (k, k + NC / 2) in two-float vectors, the form v_pk_mul_f32 /
// v_pk_add_f32 take; the weights come from the kernel's arguments (scalar registers).  Two
// correctly rounded divisions end the chain (HIP's default f32 division; div_win's proof covers
// integer sums only).
struct WinWeights {
    float w[kWinMax * kWinMax];  // w[a * e_w + b], window_weights' table
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int HW, int DC, bool SSD>
__global__ __launch_bounds__(256) void window_cost_weighted_kernel(WinArgs a, WinWeights ww) {
    const int SCALE = a.scale, HH = a.hh;
    using Lane = WinLane<HW, DC, SSD>;
    constexpr int RB = kWinCostBandRows, NC = Lane::NC, NCA = Lane::NCA;
    constexpr int NH = NC / 2;       // output pairs (k, k + NH)
    constexpr int NG = NH + 2 * HW;  // tap pairs (c, c + NH)
    constexpr int EW = 2 * HW + 1;   // e_w (weighted windows are odd)
    constexpr int RC_MAX = win_r_cols(HW, 1, DC), NR_MAX = win_rows(kWinMax / 2);
    static_assert(RB % 2 == 0 && NC % 2 == 0, "two rows and two columns per step");
    __shared__ uint8_t sl[NR_MAX * Lane::LC];
    __shared__ uint8_t sr[NR_MAX * RC_MAX];
    const WinTile t = win_tile<HW, DC>(a, SCALE);
    stage_rows<HW>(a, t, SCALE, HH, sl, sr);
    const Lane ln(a, t, SCALE, sl, sr);
    const int i0 = t.i0, j0 = t.j0, c0 = ln.c0, d = ln.d;
    f32x2 g[NG];
    // staged row r's taps, as floats: g[c] = (tap c, tap c + NH)
    auto taps = [&](int r) {
        float f[NCA];
#pragma unroll
        for (int c = 0; c < NCA; ++c) f[c] = (float)ln.ad(r, c);
#pragma unroll
        for (int c = 0; c < NG; ++c) g[c] = f32x2{f[c], f[c + NH]};
    };
    // window row wr of the outputs in acc: cost = cost + AD * w, columns in order
    auto row = [&](f32x2 *acc, int wr) {
#pragma unroll
        for (int b = 0; b < EW; ++b) {
            const float w = ww.w[wr * EW + b];
#pragma unroll
            for (int k = 0; k < NH; ++k) acc[k] = acc[k] + g[k + b] * w;
        }
    };
    const int rows = a.H - i0 < RB ? a.H - i0 : RB;
    for (int rr = 0; rr < rows; rr += 2) {
        f32x2 acc0[NH], acc1[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) acc0[k] = acc1[k] = f32x2{0.0f, 0.0f};
        // output rows rr and rr + 1 read staged rows rr .. rr + 2 HH + 1 (< NR: rr <= RB - 2)
        taps(rr);
        row(acc0, 0);
        for (int ap = 1; ap <= 2 * HH; ++ap) {
            taps(rr + ap);
            row(acc0, ap);
            row(acc1, ap - 1);
        }
        taps(rr + 2 * HH + 1);
        row(acc1, 2 * HH);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (rr + q >= rows) break;
            float *o = a.dst + ((size_t)(i0 + rr + q) * a.W + j0 + c0) * a.D + d;
            const f32x2 *acc = q ? acc1 : acc0;
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                if (j0 + c0 + k < a.W) o[(size_t)k * a.D] = acc[k].x / a.fh / a.fw;
                if (j0 + c0 + k + NH < a.W) o[(size_t)(k + NH) * a.D] = acc[k].y / a.fh / a.fw;
            }
        }
    }
}

// ---------------------------------------------------------------- CT
//
// SGM_COST_CT: cost.cpp:62-96, the census per pixel and per disparity that
// Solver::build_dsi calls.  With k = (d + min_disp) / scale and the centres
// cl = L[i][j], cr = R[i][max(j - (d + min_disp), 0)] (the disparity itself, whatever the scale),
//   cost = the kept taps (a, b) with x_r = clamp(j + b, 0, W - 1) - k >= 0 at which
//          (L[y][x_l] > cl) != (R[y][x_r] > cr)
// The tile, the staged rows and the lane's columns are the SAD kernel's; the staged right rows
// clamp at column 0 where CT skips, so a skipped tap is read like any other and masked out.  A
// window row's taps are a word of 2 HW + 1 bits, bit b = tap column b:
//   left   (L > cl) does not depend on d: the workgroup computes every output pixel's rows once,
//          into LDS, and a lane reads them back as one broadcast word per row;
//   right  a lane reads a staged row's NCA bytes once and shifts one compare per tap into the
//          word of each of its NC columns;
//   kept   cm.row[a]: not the centre, and on a weighted handle only the disc (scalar registers);
//   valid  x_l - k >= 0 depends on the tap's image column alone: one word per lane, bit c = the
//          group's tap column c, shifted by the output column.
// cost += popcount((left ^ right) & kept & valid) over the window's rows: the reference's two
// words shift alike and keep at most 62 taps, so its Hamming cost is this count.
struct CtMasks {
    unsigned row[kWinMax];  // ct_row_mask of window row a
};

// HW is always a template argument; SCALE_T, HH_T are the default window's constants, 0 and -1
// leave them to WinArgs (window_cost_kernel's comment).
template <int HW, int DC, int SCALE_T, int HH_T>
__global__ __launch_bounds__(256) void window_cost_ct_kernel(WinArgs a, CtMasks cm) {
    constexpr bool FIXED = SCALE_T != 0;
    static_assert(FIXED == (HH_T >= 0), "both or none");
    const int SCALE = FIXED ? SCALE_T : a.scale, HH = FIXED ? HH_T : a.hh;
    using Lane = WinLane<HW, DC, false>;
    constexpr int RB = kWinCostBandRows, TC = kWinCostTileCols, NC = Lane::NC, NCA = Lane::NCA, LC = Lane::LC;
    constexpr int EW = 2 * HW + 1;
    constexpr int RC_MAX = win_r_cols(HW, FIXED ? SCALE_T : 1, DC), NR_MAX = win_rows(FIXED ? HH_T : kWinMax / 2);
    constexpr int EH_MAX = FIXED ? 2 * HH_T + 1 : kWinMax;
    static_assert(NCA <= 32 && EW <= 16, "a lane's tap columns and a row's taps are one word each");
    __shared__ uint8_t sl[NR_MAX * LC];
    __shared__ uint8_t sr[NR_MAX * RC_MAX];
    __shared__ uint16_t lb[RB * TC * EH_MAX];  // [(r * TC + c) * EH + a]: output pixel (r, c)'s left bits of window row a
    const WinTile t = win_tile<HW, DC>(a, SCALE);
    stage_rows<HW>(a, t, SCALE, HH, sl, sr);
    const int EH = 2 * HH + 1;
    for (int idx = tid_x(); idx < RB * TC * EH; idx += 256) {
        const int p = idx / EH, wa = idx - p * EH;
        const int r = p / TC, c = p - r * TC;
        const int cl = sl[(r + HH) * LC + c + HW];
        const uint8_t *row = sl + (r + wa) * LC + c;
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < EW; ++b) w |= (unsigned)((int)row[b] > cl) << b;
        lb[idx] = (uint16_t)w;
    }
    __syncthreads();
    const Lane ln(a, t, SCALE, sl, sr);
    const int i0 = t.i0, j0 = t.j0, c0 = ln.c0, d = ln.d, RC = t.RC;
    const int disp = d + a.min_disp, k = disp / SCALE;
    unsigned valid = 0;
#pragma unroll
    for (int c = 0; c < NCA; ++c) valid |= (unsigned)(clampi(j0 - HW + c0 + c, 0, a.W - 1) >= k) << c;
    const int rows = a.H - i0 < RB ? a.H - i0 : RB;
    for (int rr = 0; rr < rows; ++rr) {
        // the right centres: at scale 1 the staged centre tap; at scale 2 column j - disp lies
        // left of the staged span (its shifts are disp / 2): read from the image
        int cr[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            if (SCALE == 1) {
                cr[q] = sr[(rr + HH) * RC + ln.ru[q + HW]];
            } else {
                const int j = j0 + c0 + q < a.W ? j0 + c0 + q : a.W - 1;
                const int x = j - disp > 0 ? j - disp : 0;
                cr[q] = a.right[(size_t)(i0 + rr) * a.rpitch + (size_t)x * SCALE];
            }
        }
        int cost[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) cost[q] = 0;
        for (int wa = 0; wa < EH; ++wa) {
            int rb[NCA];
#pragma unroll
            for (int c = 0; c < NCA; ++c) rb[c] = sr[(rr + wa) * RC + ln.ru[c]];
            const unsigned kept = cm.row[wa];
            const uint16_t *lrow = lb + ((rr * TC + c0) * EH + wa);
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                unsigned w = 0;  // bit b = R's tap b > cr: the sign of cr - tap, shifted in from b = 2 HW down
#pragma unroll
                for (int b = EW - 1; b >= 0; --b) w = (w << 1) | ((unsigned)(cr[q] - rb[q + b]) >> 31);
                cost[q] += __builtin_popcount((w ^ lrow[q * EH]) & kept & (valid >> q));
            }
        }
        float *o = a.dst + ((size_t)(i0 + rr) * a.W + j0 + c0) * a.D + d;
#pragma unroll
        for (int q = 0; q < NC; ++q)
            if (j0 + c0 + q < a.W) o[(size_t)q * a.D] = (float)cost[q];
    }
}

// One launch of `kernel` over the volume's tiles: a.W x a.H in tiles by bands, D / DC chunks
template <int DC, typename... Extra>
hipError_t launch_tiles(void (*kernel)(WinArgs, Extra...), hipStream_t st, const WinArgs &a, const Extra &...extra) {
    const long long ntj = (a.W + kWinCostTileCols - 1) / kWinCostTileCols;
    const long long nb = (a.H + kWinCostBandRows - 1) / kWinCostBandRows;
    if (ntj * nb > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(ntj * nb), (unsigned)(a.D / DC));
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a, extra...);
    return hipGetLastError();
}

// f(the half width 0 .. 4 as a compile-time constant)
template <typename F>
hipError_t by_half_width(int hw, F &&f) {
    switch (hw) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    }
    return hipErrorInvalidValue;
}

// the default window at SCALE: every constant at compile time
template <int SCALE, int DC, bool SSD>
hipError_t launch_default(const WinArgs &a, hipStream_t st) {
    constexpr Window w = default_window(SCALE);
    return launch_tiles<DC>(window_cost_kernel<w.hw(), DC, SSD, SCALE, w.hh(), w.eh, w.ew>, st, a);
}

}  // namespace

hipError_t launch_window_cost(int kind, const uint8_t *left, const uint8_t *right, int pitch, float *dst,
                              int min_disp, Geom g, Window win, const float *weights, hipStream_t st) {
    if (!left || !right || !dst || !window_cost_kind(kind) || min_disp < 0 ||
        (g.scale != 1 && g.scale != 2) || g.D % 32 != 0 || win.eh < 1 || win.eh > kWinMax || win.ew < 1 ||
        win.ew > kWinMax || win.bits() > 64 || (win.weighted && (!weights || win.eh % 2 == 0 || win.ew % 2 == 0)))
        return hipErrorInvalidValue;
    WinArgs a{};
    a.left = left;
    a.right = right;
    a.rpitch = (size_t)pitch * g.scale;  // SGM.cpp:47-48's decimation, as the census reads
    a.dst = dst;
    a.H = g.H;
    a.W = g.W;
    a.D = g.D;
    a.min_disp = min_disp;
    a.scale = g.scale;
    a.hh = win.hh();
    a.fh = (float)win.eh;
    a.rh = 1.0f / a.fh;
    a.fw = (float)win.ew;
    a.rw = 1.0f / a.fw;
    WinWeights ww{};
    if (win.weighted)
        for (int k = 0; k < win.eh * win.ew; ++k) ww.w[k] = weights[k];
    const Window def = default_window(g.scale);
    if (kind == kCostCt) {
        // the default window's sizes with SCALE and HH at compile time (weighted or not: the disc
        // is in the masks), any other window by the instantiation of its half width
        CtMasks cm{};
        for (int r = 0; r <= 2 * win.hh(); ++r) cm.row[r] = ct_row_mask(win, r);
        auto ct = [&](auto DC_C) -> hipError_t {
            constexpr int DC = DC_C;
            if (win.eh != def.eh || win.ew != def.ew)
                return by_half_width(win.hw(), [&](auto HW) {
                    return launch_tiles<DC>(window_cost_ct_kernel<HW, DC, 0, -1>, st, a, cm);
                });
            constexpr Window d1 = default_window(1), d2 = default_window(2);
            return g.scale == 1 ? launch_tiles<DC>(window_cost_ct_kernel<d1.hw(), DC, 1, d1.hh()>, st, a, cm)
                                : launch_tiles<DC>(window_cost_ct_kernel<d2.hw(), DC, 2, d2.hh()>, st, a, cm);
        };
        return g.D == 32 ? ct(std::integral_constant<int, 32>{}) : ct(std::integral_constant<int, 64>{});
    }
    // DC and SSD as compile-time constants: the weighted kernel and any window but the default by
    // the instantiation of its half width, the default window with every constant at compile time
    auto launch = [&](auto DC_C, auto SSD_C) -> hipError_t {
        constexpr int DC = DC_C;
        constexpr bool SSD = SSD_C;
        if (win.weighted)
            return by_half_width(win.hw(), [&](auto HW) {
                return launch_tiles<DC>(window_cost_weighted_kernel<HW, DC, SSD>, st, a, ww);
            });
        if (win.eh != def.eh || win.ew != def.ew)
            return by_half_width(win.hw(), [&](auto HW) {
                return launch_tiles<DC>(window_cost_kernel<HW, DC, SSD, 0, -1, 0, 0>, st, a);
            });
        return g.scale == 1 ? launch_default<1, DC, SSD>(a, st) : launch_default<2, DC, SSD>(a, st);
    };
    using DC32 = std::integral_constant<int, 32>;
    using DC64 = std::integral_constant<int, 64>;
    auto by_dc = [&](auto SSD_C) { return g.D == 32 ? launch(DC32{}, SSD_C) : launch(DC64{}, SSD_C); };
    return kind == kCostSsd ? by_dc(std::true_type{}) : by_dc(std::false_type{});
}

}  // namespace sgm
