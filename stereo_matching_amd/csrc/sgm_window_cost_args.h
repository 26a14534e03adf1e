// sgm_window_cost_args.h -- the host side of the SAD/SSD window costs
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

// Solver::build_dsi's window (Solver.cpp:98-99): WIN_H / scale x WIN_W / scale.
// SAD and SSD (cost.cpp:8,14) loop over -win/2 .. win/2 on either side, so at
// scale 2 (3 x 4) they sum 3 x 5 taps and divide by 3 and 4.
constexpr int win_cost_h(int scale) { return 7 / scale; }
constexpr int win_cost_w(int scale) { return 9 / scale; }
constexpr int win_cost_hh(int scale) { return win_cost_h(scale) / 2; }  // taps above and below
constexpr int win_cost_hw(int scale) { return win_cost_w(scale) / 2; }  // taps left and right

// The largest window sum: 63 taps of 255 (SAD) or 255^2 (SSD); exact in int32 and in fp32.
constexpr int kWinCostMaxSum = 63 * 255 * 255;

// x / win, correctly rounded, for win = 3, 7, 9 (div_win<WIN>, sgm_device.h: the
// rounded reciprocal's product corrected by one FMA residual step) and win = 4
// (exact).  tests/cpp/window_cost_args_main.cpp compares it with IEEE division
// on every input a window sum can reach.
inline float win_div(float x, int win) {
    if (win == 4) return x * 0.25f;
    const float r = 1.0f / (float)win;
    const float q0 = x * r;
    const float e = fmaf(-q0, (float)win, x);
    return fmaf(e, r, q0);
}

// cost.cpp:29,58: cost / win_h / win_w, two divisions in that order.
inline float win_cost_value(int sum, int scale) {
    return win_div(win_div((float)sum, win_cost_h(scale)), win_cost_w(scale));
}

// The kernel's tile: a workgroup writes kWinCostTileCols columns of
// kWinCostBandRows rows for a chunk of DC disparities (64; 32 at D = 32).
constexpr int kWinCostTileCols = 64;
constexpr int kWinCostBandRows = 16;

// Staged columns.  The left rows hold L[clamp(j0 - hw + t, 0, W - 1)] at t, the
// right rows R[clamp(j0 - hw - s_hi + u, 0, W - 1)] at u, where s_lo .. s_hi
// are the chunk's column shifts (d + min_disp) / scale.  A tap at tile column t
// under shift s reads u = min(j0 - hw + t, W - 1) - (j0 - hw) + (s_hi - s):
// the right edge's clamp comes before the shift (cost.cpp:17-18), the left
// edge's after it, where the staged clamp gives the same column.
constexpr int win_cost_l_cols(int scale) { return kWinCostTileCols + 2 * win_cost_hw(scale); }
constexpr int win_cost_r_cols(int scale, int DC) { return win_cost_l_cols(scale) + DC / scale; }
constexpr int win_cost_rows(int scale) { return kWinCostBandRows + 2 * win_cost_hh(scale); }
constexpr int win_cost_r_index(int j0, int t, int W, int scale, int s_hi, int s) {
    const int hw = win_cost_hw(scale);
    const int x = j0 - hw + t;
    return (x < W - 1 ? x : W - 1) - (j0 - hw) + (s_hi - s);
}
// the image column that index stands for
constexpr int win_cost_r_col(int j0, int u, int W, int scale, int s_hi) {
    const int c = j0 - win_cost_hw(scale) - s_hi + u;
    return c < 0 ? 0 : c > W - 1 ? W - 1 : c;
}

// The checks sgm_window_cost_device makes before it enqueues anything: the
// reason a call is refused, or null.  width: the images' columns (bytes per row).
inline const char *window_cost_refusal(int kind, const void *left, const void *right, int pitch, int width,
                                       const void *dst) {
    if (kind != kCostSad && kind != kCostSsd) return "kind must be SGM_COST_SAD or SGM_COST_SSD";
    if (!left || !right) return "NULL image";
    if (pitch < width) return "pitch below the image width";
    if (!dst) return "d_dst is NULL";
    if ((uintptr_t)dst % sizeof(float)) return "d_dst is not a float pointer";
    return nullptr;
}

}  // namespace sgm
