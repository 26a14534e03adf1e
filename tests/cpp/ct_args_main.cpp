// The host side of the CT cost (stereo_matching_amd/csrc/sgm_window_cost_args.h,
// DESIGN.md 5s) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ct_args_main.cpp
// The kind's value and the argument checks; the row masks against the weight
// table's `< 0.5` and the centre, and the kept-tap count (at most 62) over every
// accepted window; and window_cost_ct_kernel's arithmetic replayed lane by lane
// on the host -- staged rows in exactly-sized arrays, the left words, the valid
// word, the shifted-in right words -- against the definition, over whole images
// of tiles for every accepted window, W < D, min_disp and scale 2 included.
// Exits 0 when every check holds.
#include "../../include/sgm_hip.h"
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

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

static void masks(sgm::Window w) {
    std::vector<float> t((size_t)w.eh * w.ew);
    if (w.weighted) sgm::window_weights(w, t.data());
    int kept = 0;
    for (int a = 0; a <= 2 * w.hh(); ++a) {
        const unsigned m = sgm::ct_row_mask(w, a);
        EXPECT(m >> (2 * w.hw() + 1) == 0);
        for (int b = 0; b <= 2 * w.hw(); ++b) {
            // cost.cpp:79-82: the centre, then the float weight against the double 0.5
            bool want = !(a == w.hh() && b == w.hw());
            if (want && w.weighted) want = !(t[(size_t)a * w.ew + b] < 0.5);
            EXPECT(((m >> b) & 1u) == (want ? 1u : 0u));
            kept += want;
        }
    }
    EXPECT(kept == sgm::ct_taps(w) && kept <= 62 && kept >= 2);
    if (w.weighted) EXPECT(kept == sgm::weighted_bits(w.hh(), w.hw()));
    else EXPECT(kept == w.bits());
}

// cost.cpp:62-96 as DESIGN.md 5s states it, on working-grid images
static int ct_definition(const std::vector<uint8_t> &L, const std::vector<uint8_t> &R, int H, int W, int i, int j,
                         int disp, sgm::Window w, int scale) {
    const int cl = L[(size_t)i * W + j], cr = R[(size_t)i * W + (j - disp > 0 ? j - disp : 0)];
    int cost = 0;
    for (int a = -w.hh(); a <= w.hh(); ++a)
        for (int b = -w.hw(); b <= w.hw(); ++b) {
            if (a == 0 && b == 0) continue;
            if (w.weighted && !sgm::weighted_tap_kept(a, b)) continue;
            const int y = clampi(i + a, 0, H - 1), xl = clampi(j + b, 0, W - 1), xr = xl - disp / scale;
            if (xr < 0) continue;
            cost += (L[(size_t)y * W + xl] > cl) != (R[(size_t)y * W + xr] > cr);
        }
    return cost;
}

// The kernel's tiles over one image, lane by lane.
static void replay(sgm::Window win, int H, int W, int D, int DC, int scale, int min_disp, unsigned seed) {
    const int HW = win.hw(), HH = win.hh(), EW = 2 * HW + 1, EH = 2 * HH + 1;
    const int TC = sgm::kWinCostTileCols, RB = sgm::kWinCostBandRows;
    const int NC = TC / (256 / DC), NCA = NC + 2 * HW;
    const int LC = sgm::win_l_cols(HW), RC = sgm::win_r_cols(HW, scale, DC), NR = sgm::win_rows(HH);
    EXPECT(NCA <= 32 && EW <= 16 && EH <= sgm::kWinMax);
    std::vector<uint8_t> L((size_t)H * W), R((size_t)H * W);
    for (size_t n = 0; n < L.size(); ++n) {  // few grey levels: equal neighbours meet the strict `>`
        seed = seed * 1664525u + 1013904223u;
        L[n] = (uint8_t)((seed >> 24) & 7);
        R[n] = (uint8_t)((seed >> 16) & 7);
    }
    long bad = 0;
    for (int i0 = 0; i0 < H; i0 += RB)
        for (int j0 = 0; j0 < W; j0 += TC)
            for (int d0 = 0; d0 < D; d0 += DC) {
                const int s_hi = (d0 + DC - 1 + min_disp) / scale;
                std::vector<uint8_t> sl((size_t)NR * LC), sr((size_t)NR * RC);
                for (int r = 0; r < NR; ++r) {
                    const int y = clampi(i0 - HH + r, 0, H - 1);
                    for (int c = 0; c < LC; ++c) sl[(size_t)r * LC + c] = L[(size_t)y * W + clampi(j0 - HW + c, 0, W - 1)];
                    for (int c = 0; c < RC; ++c)
                        sr[(size_t)r * RC + c] = R[(size_t)y * W + sgm::win_r_col(j0, c, W, HW, s_hi)];
                }
                std::vector<uint16_t> lb((size_t)RB * TC * EH);
                for (int idx = 0; idx < RB * TC * EH; ++idx) {
                    const int p = idx / EH, wa = idx - p * EH, r = p / TC, c = p - r * TC;
                    const int cl = sl.at((size_t)(r + HH) * LC + c + HW);
                    unsigned w = 0;
                    for (int b = 0; b < EW; ++b) w |= (unsigned)(sl.at((size_t)(r + wa) * LC + c + b) > cl) << b;
                    lb.at((size_t)idx) = (uint16_t)w;
                }
                const int rows = H - i0 < RB ? H - i0 : RB;
                for (int t = 0; t < 256; ++t) {
                    const int c0 = (t / DC) * NC, d = d0 + t % DC, disp = d + min_disp, k = disp / scale;
                    std::vector<int> ru((size_t)NCA);
                    unsigned valid = 0;
                    for (int c = 0; c < NCA; ++c) {
                        ru[(size_t)c] = sgm::win_r_index(j0, c0 + c, W, HW, s_hi, k);
                        valid |= (unsigned)(clampi(j0 - HW + c0 + c, 0, W - 1) >= k) << c;
                    }
                    for (int rr = 0; rr < rows; ++rr)
                        for (int q = 0; q < NC; ++q) {
                            if (j0 + c0 + q >= W) continue;  // (the kernel computes these too and stores nothing)
                            int cr;
                            if (scale == 1) {
                                cr = sr.at((size_t)(rr + HH) * RC + ru[(size_t)(q + HW)]);
                            } else {
                                const int x = j0 + c0 + q - disp > 0 ? j0 + c0 + q - disp : 0;
                                cr = R.at((size_t)(i0 + rr) * W + x);
                            }
                            int cost = 0;
                            for (int wa = 0; wa < EH; ++wa) {
                                unsigned w = 0;
                                for (int b = EW - 1; b >= 0; --b) {
                                    const int tap = sr.at((size_t)(rr + wa) * RC + ru[(size_t)(q + b)]);
                                    w = (w << 1) | ((unsigned)(cr - tap) >> 31);
                                }
                                const unsigned l = lb.at(((size_t)(rr * TC + c0) * EH + wa) + (size_t)q * EH);
                                cost += __builtin_popcount((w ^ l) & sgm::ct_row_mask(win, wa) & (valid >> q));
                            }
                            if (cost != ct_definition(L, R, H, W, i0 + rr, j0 + c0 + q, disp, win, scale)) ++bad;
                        }
                }
            }
    if (bad)
        fprintf(stderr, "window %d x %d%s %d x %d D %d DC %d scale %d min_disp %d: %ld costs off\n", win.eh, win.ew,
                win.weighted ? " weighted" : "", H, W, D, DC, scale, min_disp, bad);
    EXPECT(bad == 0);
}

int main() {
    EXPECT(sgm::kCostCt == SGM_COST_CT && SGM_COST_CT == 4);
    uint8_t img[4];
    float dst[4];
    EXPECT(sgm::window_cost_refusal(SGM_COST_CT, img, img, 4, 4, dst) == nullptr);
    for (int kind : {0, 3, 5, -1}) EXPECT(strstr(sgm::window_cost_refusal(kind, img, img, 4, 4, dst), "kind"));
    EXPECT(sgm::window_cost_kind(1) && sgm::window_cost_kind(2) && sgm::window_cost_kind(4));
    EXPECT(!sgm::window_cost_kind(0) && !sgm::window_cost_kind(3) && !sgm::window_cost_kind(-1));
    static_assert(sgm::ct_taps(sgm::default_window(1)) == 62 && sgm::ct_taps(sgm::default_window(2)) == 14, "taps");
    int n = 0;
    unsigned seed = 1;
    for (int scale : {1, 2})
        for (int wh = 0; wh <= 20; ++wh)
            for (int ww = 0; ww <= 20; ++ww) {
                if (sgm::window_refusal(wh, ww, scale)) continue;
                if (wh % scale || ww % scale) continue;  // (the same effective window again)
                for (int weighted = 0; weighted < 2; ++weighted) {
                    if (weighted && sgm::weighted_refusal(wh, ww, scale)) continue;
                    sgm::Window win = sgm::window_of(wh, ww, scale);
                    win.weighted = weighted != 0;
                    masks(win);
                    ++n;
                    // one tile and a bit, W < D with a large min_disp, two tiles; one band and a bit
                    replay(win, 5, 20, 32, 32, scale, 0, ++seed);
                    replay(win, 18, 67, 64, 64, scale, 0, ++seed);
                    replay(win, 3, 9, 64, 64, scale, 16, ++seed);
                }
            }
    EXPECT(n > 60);
    if (failures) return 1;
    printf("ct args ok\n");
    return 0;
}
