// The host side of the weighted windows (stereo_matching_amd/csrc/
// sgm_window_cost_args.h) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all weighted_args_main.cpp
// The weight table against its formula, the census's disc against the table's
// `< 0.5`, the kept-bit counts, the refusal rule over every (win_h, win_w) in
// 0 .. 20 at both scales, and the weighted producer's indices -- staged rows,
// staged columns, tap pairs, weight entries -- over whole rows of tiles for every
// accepted window, W < D and a large min_disp included.
// Exits 0 when every check holds.
#include "../../stereo_matching_amd/csrc/sgm_window_cost_args.h"

#include <string.h>
#include <vector>

static int failures = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
        }                                                          \
    } while (0)

static bool odd_rule(int win_h, int win_w, int scale) {
    if (sgm::window_refusal(win_h, win_w, scale)) return false;
    return (win_h / scale) % 2 == 1 && (win_w / scale) % 2 == 1;
}

static void rule() {
    int n_ok = 0;
    for (int scale : {1, 2})
        for (int wh = 0; wh <= 20; ++wh)
            for (int ww = 0; ww <= 20; ++ww) {
                const char *why = sgm::weighted_refusal(wh, ww, scale);
                if ((why == nullptr) != odd_rule(wh, ww, scale)) {
                    ++failures;
                    fprintf(stderr, "window (%d, %d) scale %d: %s\n", wh, ww, scale, why ? why : "accepted");
                }
                // every other rule stays as it is: its message is window_refusal's own
                if (const char *plain = sgm::window_refusal(wh, ww, scale)) EXPECT(why == plain);
                n_ok += why == nullptr;
            }
    // scale 1: odd pairs of 1, 3, 5, 7, 9 less 1 x 1 and 9 x 9; scale 2: each from two values
    EXPECT(n_ok == 23 + 4 * 23);
    EXPECT(strstr(sgm::weighted_refusal(7, 9, 2), "odd") && strstr(sgm::weighted_refusal(5, 6, 1), "odd") &&
           strstr(sgm::weighted_refusal(10, 12, 2), "odd"));
    EXPECT(strstr(sgm::weighted_refusal(9, 9, 1), "64 bits") && strstr(sgm::weighted_refusal(1, 1, 1), "centre"));
    EXPECT(!sgm::weighted_refusal(7, 9, 1) && !sgm::weighted_refusal(14, 18, 2) && !sgm::weighted_refusal(15, 19, 2) &&
           !sgm::weighted_refusal(10, 18, 2) && !sgm::weighted_refusal(1, 9, 1) && !sgm::weighted_refusal(3, 3, 1));
}

static void table_and_mask(sgm::Window w) {
    std::vector<float> t((size_t)w.eh * w.ew);  // (exactly the table's size: an overrun is the sanitizer's)
    EXPECT(sgm::window_weights(w, t.data()) == w.eh * w.ew);
    int kept = 0;
    for (int a = 0; a < w.eh; ++a)
        for (int b = 0; b < w.ew; ++b) {
            const int da = a - w.hh(), db = b - w.hw();
            const float want = (float)exp((pow(da, 2) + pow(db, 2)) / -25.0);
            EXPECT(memcmp(&want, &t[(size_t)a * w.ew + b], sizeof(float)) == 0);
            // cost.cpp:115: the float against the double 0.5
            EXPECT((t[(size_t)a * w.ew + b] < 0.5) == !sgm::weighted_tap_kept(da, db));
            kept += (da || db) && sgm::weighted_tap_kept(da, db);
        }
    EXPECT(kept == sgm::weighted_bits(w.hh(), w.hw()) && kept <= w.bits() && kept >= 2);
    EXPECT(t[(size_t)w.hh() * w.ew + w.hw()] == 1.0f);
}

// The weighted producer's reads for the tiles of one row of tiles (DC lanes along d, NC columns
// per group, two output rows per step): every index inside its array, every staged column the
// column cost.cpp:16-18 reads.
static void tile_row(sgm::Window win, int W, int DC, int scale, int min_disp, int D) {
    const int hw = win.hw(), hh = win.hh();
    const int TJ = sgm::kWinCostTileCols, RB = sgm::kWinCostBandRows;
    const int NC = TJ / (256 / DC), NH = NC / 2, NCA = NC + 2 * hw, NG = NH + 2 * hw, EW = 2 * hw + 1;
    const int lc = sgm::win_l_cols(hw), rc = sgm::win_r_cols(hw, scale, DC), nr = sgm::win_rows(hh);
    EXPECT(rc <= sgm::win_r_cols(hw, 1, DC) && nr <= sgm::win_rows(sgm::kWinMax / 2));
    long bad = 0;
    for (int j0 = 0; j0 < W; j0 += TJ)
        for (int d0 = 0; d0 < D; d0 += DC) {
            const int s_hi = (d0 + DC - 1 + min_disp) / scale;
            std::vector<int> staged((size_t)rc);
            for (int u = 0; u < rc; ++u) staged[(size_t)u] = sgm::win_r_col(j0, u, W, hw, s_hi);
            for (int t = 0; t < 256; ++t) {
                const int c0 = (t / DC) * NC, s = (d0 + t % DC + min_disp) / scale;
                for (int c = 0; c < NCA; ++c) {
                    const int lidx = c0 + c, u = sgm::win_r_index(j0, c0 + c, W, hw, s_hi, s);
                    int xl = j0 - hw + c0 + c;
                    xl = xl < 0 ? 0 : xl > W - 1 ? W - 1 : xl;
                    const int xr = xl - s > 0 ? xl - s : 0;
                    if (lidx < 0 || lidx >= lc || u < 0 || u >= rc || staged.at((size_t)u) != xr) ++bad;
                }
                for (int c = 0; c < NG; ++c)
                    if (c + NH >= NCA) ++bad;  // g[c] = (f[c], f[c + NH])
                for (int k = 0; k < NH; ++k)
                    for (int b = 0; b < EW; ++b)
                        if (k + b >= NG) ++bad;  // acc[k] += g[k + b] * w
            }
        }
    // staged rows of a step: rr .. rr + 2 hh + 1 for rr = 0, 2, .. RB - 2; weight rows 0 .. 2 hh
    for (int rr = 0; rr < RB; rr += 2)
        if (rr + 2 * hh + 1 >= nr) ++bad;
    if ((2 * hh) * EW + EW - 1 >= sgm::kWinMax * sgm::kWinMax || (2 * hh + 1) * EW != win.eh * win.ew) ++bad;
    if (bad)
        fprintf(stderr, "window %d x %d W %d DC %d scale %d min_disp %d: %ld indices off\n", win.eh, win.ew, W, DC,
                scale, min_disp, bad);
    EXPECT(bad == 0);
}

int main() {
    rule();
    static_assert(sgm::weighted_bits(3, 4) == 50 && sgm::weighted_bits(4, 3) == 50 && sgm::weighted_bits(3, 3) == 44 &&
                      sgm::weighted_bits(2, 4) == 40 && sgm::weighted_bits(2, 2) == 24 && sgm::weighted_bits(1, 1) == 8 &&
                      sgm::weighted_bits(0, 4) == 8,
                  "the disc's bits");
    int n = 0;
    for (int scale : {1, 2})
        for (int wh = 0; wh <= 20; ++wh)
            for (int ww = 0; ww <= 20; ++ww) {
                if (sgm::weighted_refusal(wh, ww, scale)) continue;
                sgm::Window win = sgm::window_of(wh, ww, scale);
                EXPECT(!win.weighted);
                win.weighted = true;
                table_and_mask(win);
                ++n;
                if (wh % scale || ww % scale) continue;  // (the same effective window again)
                for (int DC : {32, 64})
                    for (int W : {1, 5, 20, 63, 64, 65, 130})  // W < D included
                        for (int m : {0, 16, 4096}) tile_row(win, W, DC, scale, m, 2 * DC);
            }
    EXPECT(n == 23 + 4 * 23);
    if (failures) return 1;
    printf("weighted args ok\n");
    return 0;
}
