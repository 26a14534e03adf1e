// The host side of the SAD/SSD window costs (stereo_matching_amd/csrc/
// sgm_window_cost_args.h) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all window_cost_args_main.cpp
// The two divisions against IEEE division over every reachable input, the
// staged-column index over whole rows of tiles, the argument checks.
// Exits 0 when every check holds.
#include "../../stereo_matching_amd/csrc/sgm_window_cost_args.h"

#include "../../include/sgm_hip.h"

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

// every window sum 0 .. 63 * 255^2 through the first division, each of those
// quotients through the second: the FMA form against IEEE division
static void divisions(int scale) {
    const sgm::Window win = sgm::default_window(scale);
    const int wh = win.eh, ww = win.ew;
    volatile float fh = (float)wh, fw = (float)ww;  // (no constant folding into a reciprocal)
    long bad1 = 0, bad2 = 0, bad = 0;
    for (int x = 0; x <= sgm::kWinCostMaxSum; ++x) {
        const float q = (float)x / fh;
        const float g = sgm::win_div((float)x, wh);
        if (!same_bits(q, g)) ++bad1;
        if (!same_bits(q / fw, sgm::win_div(q, ww))) ++bad2;
        if (!same_bits((float)x / fh / fw, sgm::win_cost_value(x, win))) ++bad;
    }
    if (bad1 || bad2 || bad)
        fprintf(stderr, "scale %d: %ld first, %ld second, %ld composed divisions differ\n", scale, bad1, bad2, bad);
    EXPECT(bad1 == 0 && bad2 == 0 && bad == 0);
}

// Every tap of every tile of a W-column row: the staged index lies inside the
// staged row and stands for the column cost.cpp:16-18 reads.
static void staged_columns(int W, int D, int scale, int min_disp) {
    const int DC = D == 32 ? 32 : 64, hw = sgm::default_window(scale).hw();
    const int lc = sgm::win_l_cols(hw), rc = sgm::win_r_cols(hw, scale, DC);
    std::vector<int> staged((size_t)rc);
    long bad = 0;
    for (int j0 = 0; j0 < W; j0 += sgm::kWinCostTileCols)
        for (int d0 = 0; d0 < D; d0 += DC) {
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
    if (bad) fprintf(stderr, "W %d D %d scale %d min_disp %d: %ld taps off\n", W, D, scale, min_disp, bad);
    EXPECT(bad == 0);
}

int main() {
    EXPECT(sgm::kCostCensus == SGM_COST_CENSUS && sgm::kCostSad == SGM_COST_SAD && sgm::kCostSsd == SGM_COST_SSD);
    const sgm::Window w1 = sgm::default_window(1), w2 = sgm::default_window(2);
    EXPECT(w1.eh == 7 && w1.ew == 9 && w2.eh == 3 && w2.ew == 4);
    EXPECT(w1.hh() == 3 && w1.hw() == 4 && w2.hh() == 1 && w2.hw() == 2);
    EXPECT(sgm::kWinCostMaxSum == 4096575);
    divisions(1);
    divisions(2);
    EXPECT(same_bits(sgm::win_cost_value(sgm::kWinCostMaxSum, w1), 65025.0f));

    const int widths[] = {5, 33, 40, 63, 64, 65, 170, 300};
    for (int W : widths)
        for (int D : {32, 64, 128, 256})
            for (int scale : {1, 2})
                for (int m : {0, 16, 600}) staged_columns(W, D, scale, m);

    char img[4] = {}, dst[8] __attribute__((aligned(8))) = {};
    EXPECT(sgm::window_cost_refusal(SGM_COST_SAD, img, img, 4, 4, dst) == nullptr);
    EXPECT(sgm::window_cost_refusal(SGM_COST_SSD, img, img, 9, 4, dst) == nullptr);
    EXPECT(strstr(sgm::window_cost_refusal(SGM_COST_CENSUS, img, img, 4, 4, dst), "kind"));
    EXPECT(strstr(sgm::window_cost_refusal(3, img, img, 4, 4, dst), "kind"));
    EXPECT(strstr(sgm::window_cost_refusal(-1, img, img, 4, 4, dst), "kind"));
    EXPECT(strstr(sgm::window_cost_refusal(SGM_COST_SAD, nullptr, img, 4, 4, dst), "NULL image"));
    EXPECT(strstr(sgm::window_cost_refusal(SGM_COST_SAD, img, nullptr, 4, 4, dst), "NULL image"));
    EXPECT(strstr(sgm::window_cost_refusal(SGM_COST_SAD, img, img, 3, 4, dst), "pitch"));
    EXPECT(strstr(sgm::window_cost_refusal(SGM_COST_SAD, img, img, 4, 4, nullptr), "NULL"));
    EXPECT(strstr(sgm::window_cost_refusal(SGM_COST_SAD, img, img, 4, 4, dst + 2), "float"));
    if (failures) return 1;
    printf("window cost args ok\n");
    return 0;
}
