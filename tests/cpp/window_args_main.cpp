// The host side of the matching-window setting (stereo_matching_amd/csrc/
// sgm_window_cost_args.h) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all window_args_main.cpp
// The accept / refuse rule over every (win_h, win_w) in 0 .. 20 at both scales,
// win_div against IEEE division for every divisor 1 .. 9 over every reachable
// sum (and over every first quotient, for the second division), the staged-row
// index helpers against a brute-force clamp for every accepted window.
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

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(a)) == 0; }

// the issue's rule, restated: 1 <= e_h, e_w <= 9, not HH = HW = 0, at most 64 bits
static bool accepted(int win_h, int win_w, int scale) {
    const int eh = win_h / scale, ew = win_w / scale;
    if (eh < 1 || eh > 9 || ew < 1 || ew > 9) return false;
    const int hh = eh / 2, hw = ew / 2;
    if (hh == 0 && hw == 0) return false;
    return (2 * hh + 1) * (2 * hw + 1) - 1 <= 64;
}

static void rule() {
    int n_ok = 0;
    for (int scale : {1, 2})
        for (int wh = 0; wh <= 20; ++wh)
            for (int ww = 0; ww <= 20; ++ww) {
                const char *why = sgm::window_refusal(wh, ww, scale);
                if ((why == nullptr) != accepted(wh, ww, scale)) {
                    ++failures;
                    fprintf(stderr, "window (%d, %d) scale %d: %s\n", wh, ww, scale, why ? why : "accepted");
                }
                if (!why) {
                    ++n_ok;
                    const sgm::Window w = sgm::window_of(wh, ww, scale);
                    EXPECT(w.eh == wh / scale && w.ew == ww / scale && w.hh() <= 4 && w.hw() <= 4);
                    EXPECT(w.bits() <= 64 && w.bits() >= 2);
                    EXPECT((w.bits() + 1) * 255 * 255 <= sgm::kWinCostMaxSum);
                    // the staged rows fit a workgroup's LDS with room to spare
                    EXPECT(sgm::win_lds_bytes(w, scale, 64) <= 4896);
                }
            }
    // scale 1: 9 * 9 sizes less 1x1 and the four e = 8, 9 pairs; scale 2: e = 1 .. 9 from 2 .. 19
    EXPECT(n_ok == (81 - 1 - 4) + (18 * 18 - 4 - 16));
    EXPECT(sgm::window_refusal(-3, 9, 1) && sgm::window_refusal(7, -9, 2) && sgm::window_refusal(7, 9, 3));
    EXPECT(strstr(sgm::window_refusal(9, 9, 1), "64 bits") && strstr(sgm::window_refusal(1, 1, 1), "centre"));
    EXPECT(strstr(sgm::window_refusal(10, 9, 1), "1..9") && strstr(sgm::window_refusal(1, 9, 2), "1..9"));
    EXPECT(sgm::window_refusal(7, 9, 1) == nullptr && sgm::window_refusal(7, 9, 2) == nullptr);
    EXPECT(sgm::default_window(1).eh == 7 && sgm::default_window(1).ew == 9 && sgm::default_window(2).eh == 3 &&
           sgm::default_window(2).ew == 4 && sgm::default_window(1).bits() == 62);
}

// win_div(x, w) == x / w for every w in 1 .. 9 and every integer x a window sum can reach;
// then the second division, over every quotient the first can hand it
static void divisions() {
    for (int w = 1; w <= 9; ++w) {
        volatile float fw = (float)w;  // (no constant folding into a reciprocal)
        long bad = 0;
        for (int x = 0; x <= sgm::kWinCostMaxSum; ++x)
            if (!same_bits((float)x / fw, sgm::win_div((float)x, w))) ++bad;
        if (bad) fprintf(stderr, "divisor %d: %ld quotients differ\n", w, bad);
        EXPECT(bad == 0);
    }
    for (int eh = 1; eh <= 9; ++eh)
        for (int ew = 1; ew <= 9; ++ew) {
            volatile float fh = (float)eh, fw = (float)ew;
            const sgm::Window win{eh, ew};
            // (the sums this window reaches: its taps of 255^2)
            const int top = (win.bits() + 1 > 63 ? 63 : win.bits() + 1) * 255 * 255;
            long bad = 0;
            for (int x = 0; x <= top; ++x)
                if (!same_bits((float)x / fh / fw, sgm::win_cost_value(x, win))) ++bad;
            if (bad) fprintf(stderr, "window %d x %d: %ld costs differ\n", eh, ew, bad);
            EXPECT(bad == 0);
        }
}

// Every tap of the tile at j0 of a W-column row: the staged index lies inside the staged row
// and stands for the column cost.cpp:16-18 reads; the left row's index likewise.
static void staged_columns(sgm::Window win, int W, int j0, int DC, int scale, int min_disp) {
    const int hw = win.hw();
    const int lc = sgm::win_l_cols(hw), rc = sgm::win_r_cols(hw, scale, DC);
    std::vector<int> staged((size_t)rc);
    long bad = 0;
    for (int d0 = 0; d0 < 2 * DC; d0 += DC) {
        const int s_hi = (d0 + DC - 1 + min_disp) / scale;
        for (int u = 0; u < rc; ++u) staged[(size_t)u] = sgm::win_r_col(j0, u, W, hw, s_hi);
        for (int t = 0; t < lc; ++t)
            for (int dd = 0; dd < DC; ++dd) {
                const int s = (d0 + dd + min_disp) / scale;
                const int u = sgm::win_r_index(j0, t, W, hw, s_hi, s);
                int xl = j0 - hw + t;
                xl = xl < 0 ? 0 : xl > W - 1 ? W - 1 : xl;
                const int xr = xl - s > 0 ? xl - s : 0;
                if (u < 0 || u >= rc || staged.at((size_t)u) != xr) ++bad;
            }
    }
    if (bad)
        fprintf(stderr, "window %d x %d W %d j0 %d DC %d scale %d min_disp %d: %ld taps off\n", win.eh, win.ew, W,
                j0, DC, scale, min_disp, bad);
    EXPECT(bad == 0);
}

int main() {
    rule();
    divisions();
    for (int scale : {1, 2})
        for (int wh = 0; wh <= 20; ++wh)
            for (int ww = 0; ww <= 20; ++ww) {
                if (sgm::window_refusal(wh, ww, scale)) continue;
                const sgm::Window win = sgm::window_of(wh, ww, scale);
                EXPECT(sgm::win_rows(win.hh()) == sgm::kWinCostBandRows + 2 * win.hh());
                for (int W : {1, 2, 63, 64, 65})
                    for (int j0 : {0, 64}) {
                        if (j0 >= W) continue;  // (no such tile)
                        for (int DC : {32, 64})
                            for (int m : {0, 16}) staged_columns(win, W, j0, DC, scale, m);
                    }
            }
    if (failures) return 1;
    printf("window args ok\n");
    return 0;
}
