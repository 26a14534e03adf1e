// sgm_window_cost_args.h -- the host side of the SAD/SSD window costs and of CT
// (sgm_window_cost.hip): the cost kinds, the window and its two
// divisions, the argument checks of the C-ABI and the tile geometry the kernel
// indexes its staged rows by.  Plain C++ with no HIP in it, so that
// tests/cpp/window_cost_args_main.cpp can run it on the CPU under a sanitizer;
// the index helpers are constexpr, which is what lets the kernel call them.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace sgm {

// The cost kinds of include/sgm_hip.h (SGM_COST_*), by value.
constexpr int kCostCensus = 0, kCostSad = 1, kCostSsd = 2;
// CT, build_dsi's per-disparity census.  3 stays refused: the reference's cost.cpp has
// three functions beside CT_pts, and the value is pinned as invalid by the tests of before CT.
constexpr int kCostCt = 4;
constexpr bool window_cost_kind(int kind) { return kind == kCostSad || kind == kCostSsd || kind == kCostCt; }

// The matching window: sgm_set_window's (win_h, win_w) are the
// reference's WIN_H, WIN_W; Solver::build_dsi and build_cost_table divide them by
// the scale (Solver.cpp:98-99, :127-128), and CT_pts, SAD and SSD loop over
// -e / 2 .. e / 2 on either side (cost.cpp:8,14,107,111): an even e_w = 4 still
// has 5 taps, and SAD / SSD divide by e_h and e_w, not by the tap counts.
struct Window {
    int eh, ew;  // win_h / scale, win_w / scale
    bool weighted = false;  // sgm_set_weighted: Gaussian SAD / SSD taps, the census's disc
    constexpr int hh() const { return eh / 2; }  // taps above and below
    constexpr int hw() const { return ew / 2; }  // taps left and right
    constexpr int bits() const { return (2 * hh() + 1) * (2 * hw() + 1) - 1; }  // census bits (unmasked)
};
constexpr int kWinH = 7, kWinW = 9;  // inc/Solver.h
constexpr int kWinMax = 9;           // the largest e_h, e_w served (half sizes <= 4)
constexpr Window window_of(int win_h, int win_w, int scale) { return Window{win_h / scale, win_w / scale}; }
constexpr Window default_window(int scale) { return window_of(kWinH, kWinW, scale); }

// Why sgm_set_window refuses (win_h, win_w) at this scale, or null.  The census
// word holds 64 bits: 9 x 9 taps (80 bits) would shift bits out in the
// reference's own word, so it is refused, not served wrong.
constexpr const char *window_refusal(int win_h, int win_w, int scale) {
    if (scale != 1 && scale != 2) return "scale must be 1 or 2";
    const Window w = window_of(win_h, win_w, scale);
    if (w.eh < 1 || w.eh > kWinMax || w.ew < 1 || w.ew > kWinMax)
        return "win_h / scale and win_w / scale must lie in 1..9";
    if (w.hh() == 0 && w.hw() == 0) return "the window has no tap beside its centre";
    if (w.bits() > 64) return "the census word holds 64 bits (a 9 x 9 window has 80)";
    return nullptr;
}

// The reference's WEIGHTED_COST (inc/Solver.h:15).  Solver::Solver's table
// (Solver.cpp:29-45) is weight[a * e_w + b] = exp(((a - hh)^2 + (b - hw)^2) / -25.0), computed in
// double and stored as float; SAD and SSD multiply every tap by it, CT_pts skips the taps whose
// weight is below 0.5.  exp(-17 / 25) = 0.5066 and exp(-18 / 25) = 0.4868, so the census keeps the
// disc da^2 + db^2 <= 17 (weighted_args_main.cpp compares the two forms over every tap).
constexpr int kWeightDisc = 17;
constexpr bool weighted_tap_kept(int da, int db) { return da * da + db * db <= kWeightDisc; }
// census bits of the window's disc (the centre skipped): 7 x 9 keeps 50 of 62
constexpr int weighted_bits(int hh, int hw) {
    int n = 0;
    for (int da = -hh; da <= hh; ++da)
        for (int db = -hw; db <= hw; ++db) n += (da || db) && weighted_tap_kept(da, db);
    return n;
}
// The table of an odd window, e_h * e_w floats in row-major order (out: kWinMax * kWinMax at the
// most); the count written.
inline int window_weights(Window w, float *out) {
    for (int a = 0; a < w.eh; ++a)
        for (int b = 0; b < w.ew; ++b) {
            const double da = a - w.hh(), db = b - w.hw();
            out[a * w.ew + b] = (float)exp((da * da + db * db) / -25.0);
        }
    return w.eh * w.ew;
}
// Why a weighted handle refuses (win_h, win_w) at this scale, or null: window_refusal's rules, and
// both effective sides odd.  With an even side the reference's loops run one tap past the table's
// row (cost.cpp:21 with j + win_w / 2 = win_w) and, at the last row, past the table: no definition.
constexpr const char *weighted_refusal(int win_h, int win_w, int scale) {
    if (const char *why = window_refusal(win_h, win_w, scale)) return why;
    const Window w = window_of(win_h, win_w, scale);
    if (w.eh % 2 == 0 || w.ew % 2 == 0)
        return "weighted windows need odd win_h / scale and win_w / scale (the reference reads past its "
               "weight table with an even side)";
    return nullptr;
}

// CT (cost.cpp:62-96) keeps the taps CT_pts keeps: every tap but the centre, and on
// a weighted handle only the disc's.  Window row a's kept taps as a bit mask, bit b = tap column b
// (a = 0 .. 2 hh, b = 0 .. 2 hw): the kernel ANDs it over the row's XORed census bits.
constexpr unsigned ct_row_mask(Window w, int a) {
    unsigned m = 0;
    for (int b = 0; b <= 2 * w.hw(); ++b) {
        const int da = a - w.hh(), db = b - w.hw();
        if ((da || db) && (!w.weighted || weighted_tap_kept(da, db))) m |= 1u << b;
    }
    return m;
}
// the taps it keeps in all: the largest CT cost (62 at the most)
constexpr int ct_taps(Window w) {
    int n = 0;
    for (int a = 0; a <= 2 * w.hh(); ++a)
        for (unsigned m = ct_row_mask(w, a); m; m &= m - 1) ++n;
    return n;
}

// The largest window sum: 63 taps of 255 (SAD) or 255^2 (SSD); exact in int32 and in fp32.
constexpr int kWinCostMaxSum = 63 * 255 * 255;

// x / win, correctly rounded, for win = 1 .. 9 (div_win<WIN>, sgm_device.h: the
// rounded reciprocal's product corrected by one FMA residual step; with win a
// power of two the reciprocal and the product are exact and the residual is 0).
// tests/cpp/window_cost_args_main.cpp and window_args_main.cpp compare it with
// IEEE division on every input a window sum can reach.
inline float win_div(float x, int win) {
    if (win == 4) return x * 0.25f;
    const float r = 1.0f / (float)win;
    const float q0 = x * r;
    const float e = fmaf(-q0, (float)win, x);
    return fmaf(e, r, q0);
}

// cost.cpp:29,58: cost / win_h / win_w, two divisions in that order.
inline float win_cost_value(int sum, Window w) { return win_div(win_div((float)sum, w.eh), w.ew); }

// The kernel's tile: a workgroup writes kWinCostTileCols columns of
// kWinCostBandRows rows for a chunk of DC disparities (64; 32 at D = 32).
constexpr int kWinCostTileCols = 64;
constexpr int kWinCostBandRows = 16;

// Staged columns, with hw the window's half width.  The left rows hold
// L[clamp(j0 - hw + t, 0, W - 1)] at t, the right rows
// R[clamp(j0 - hw - s_hi + u, 0, W - 1)] at u, where s_lo .. s_hi are the chunk's
// column shifts (d + min_disp) / scale.  A tap at tile column t under shift s
// reads u = min(j0 - hw + t, W - 1) - (j0 - hw) + (s_hi - s): the right edge's
// clamp comes before the shift (cost.cpp:17-18), the left edge's after it,
// where the staged clamp gives the same column.
constexpr int win_l_cols(int hw) { return kWinCostTileCols + 2 * hw; }
constexpr int win_r_cols(int hw, int scale, int DC) { return win_l_cols(hw) + DC / scale; }
constexpr int win_rows(int hh) { return kWinCostBandRows + 2 * hh; }
constexpr int win_r_index(int j0, int t, int W, int hw, int s_hi, int s) {
    const int x = j0 - hw + t;
    return (x < W - 1 ? x : W - 1) - (j0 - hw) + (s_hi - s);
}
// the image column that index stands for
constexpr int win_r_col(int j0, int u, int W, int hw, int s_hi) {
    const int c = j0 - hw - s_hi + u;
    return c < 0 ? 0 : c > W - 1 ? W - 1 : c;
}
// LDS bytes of a workgroup's staged rows.  The largest over the accepted windows, at scale 1
// and DC = 64, is 9 x 7's 24 rows of 70 + 134 bytes = 4896 (the default 7 x 9: 22 x (72 + 136)
// = 4576), of the 64 KiB a workgroup may take.
constexpr int win_lds_bytes(Window w, int scale, int DC) {
    return win_rows(w.hh()) * (win_l_cols(w.hw()) + win_r_cols(w.hw(), scale, DC));
}

// The checks sgm_window_cost_device makes before it enqueues anything: the
// reason a call is refused, or null.  width: the images' columns (bytes per row).
inline const char *window_cost_refusal(int kind, const void *left, const void *right, int pitch, int width,
                                       const void *dst) {
    if (!window_cost_kind(kind)) return "kind must be SGM_COST_SAD, SGM_COST_SSD or SGM_COST_CT";
    if (!left || !right) return "NULL image";
    if (pitch < width) return "pitch below the image width";
    if (!dst) return "d_dst is NULL";
    if ((uintptr_t)dst % sizeof(float)) return "d_dst is not a float pointer";
    return nullptr;
}

}  // namespace sgm
