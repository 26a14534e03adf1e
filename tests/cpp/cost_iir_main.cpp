// The two cost filters' recursions (stereo_matching_amd/csrc/sgm_cost_iir.h) on
// the CPU, driven the way the kernels drive them, for a sanitizer build:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all cost_iir_main.cpp
// Usage: cost_iir_main MODE WIN N IN OUT.  IN holds chains of N floats each, OUT
// receives the filtered chains (raw float32, native byte order):
//   h     every chain through HFilter<WIN>: init, out, advance (cost_h_body's walk)
//   hif   the same positions through advance_if, every position of the chain
//         visited with filt / upd as selects (the strip pass's edge strips)
//   hck   WIN = 5: per chain, one output chain for every position p = 2 .. N-3:
//         the state before the step that produces p goes through
//         HCheckpoint::save and ::restore into a fresh state, which continues
//   v     the chains in pairs through VFilter<WIN, 2>: init, out, advance
//   vcar  WIN = 3: per pair, one output pair for every row b = 1 .. N-1: the
//         state before row b goes through store_carry and load_carry into a
//         fresh state, which continues
// tests/test_cost_iir_cpu.py compares every output with the oracle's filters.
#include "../../stereo_matching_amd/csrc/sgm_cost_iir.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using sgm::HCheckpoint;
using sgm::HFilter;
using sgm::VFilter;

// split: the position whose state is saved and restored first (-1: none)
template <int WIN>
static void hrow(const float *x, float *y, int W, int split) {
    constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1;
    const int T = W - 2 * HALF;
    HFilter<WIN> f{};
    float first[WIN];
    for (int k = 0; k < WIN; ++k) first[k] = x[k];
    f.init(first);
    for (int p = 0; p < LAG; ++p) y[p] = x[p];
    for (int t = 0; t < T; ++t) {
        if constexpr (WIN == 5) {
            if (LAG + t == split) {
                HCheckpoint ck;
                ck.save(f);
                HFilter<5> g;
                g.sum = g.hist[0] = g.hist[1] = NAN;
                ck.restore(g);
                f = g;
            }
        }
        const float v = f.out();
        y[LAG + t] = v;
        if (t < T - 1) f.advance(v, x[WIN + t]);
    }
    for (int p = LAG + T; p < W; ++p) y[p] = x[p];
}

template <int WIN>
static void hrow_if(const float *x, float *y, int W) {
    constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1;
    const int last = LAG + (W - 2 * HALF) - 1;  // the last filtered position
    HFilter<WIN> f{};
    float first[WIN];
    for (int k = 0; k < WIN; ++k) first[k] = x[k];
    f.init(first);
    for (int p = 0; p < W; ++p) {
        const bool filt = p >= LAG && p <= last, upd = p >= LAG && p < last;
        const float c = filt ? f.out() : x[p];
        const int nx = p + HALF + 1;  // (past the chain: clamped, feeds nothing)
        f.advance_if(filt, upd, c, x[nx < W - 1 ? nx : W - 1]);
        y[p] = c;
    }
}

// two chains x0, x1 of H rows; split: the row before which the state is carried (-1: none)
template <int WIN>
static void vpair(const float *x0, const float *x1, float *y0, float *y1, int H, int split) {
    constexpr int V = 2, HALF = WIN / 2, LAG = WIN - HALF - 1;
    const int T = H - 2 * HALF;
    const float *x[V] = {x0, x1};
    float *y[V] = {y0, y1};
    VFilter<WIN, V> vf{};
    float rows[WIN][V];
    for (int k = 0; k < WIN; ++k)
        for (int v = 0; v < V; ++v) rows[k][v] = x[v][k];
    vf.init(rows);
    for (int i = 0; i < H; ++i) {
        if (i == split) {
            float carry[2][V];
            vf.store_carry([&](const float(&s)[V], int k) { memcpy(carry[k], s, sizeof(s)); });
            VFilter<WIN, V> g;
            for (int v = 0; v < V; ++v) g.sum[v] = g.o1[v] = NAN;
            g.load_carry([&](float(&d)[V], int k) { memcpy(d, carry[k], sizeof(d)); });
            vf = g;
        }
        float c[V];
        if (i < LAG || i >= LAG + T) {
            for (int v = 0; v < V; ++v) c[v] = x[v][i];
        } else {
            vf.out(c);
            if (i - LAG < T - 1) {
                float r[V];
                for (int v = 0; v < V; ++v) r[v] = x[v][i + HALF + 1];
                vf.advance(c, r);
            }
        }
        for (int v = 0; v < V; ++v) y[v][i] = c[v];
    }
}

static bool read_floats(const char *path, std::vector<float> *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    float buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: cost_iir_main MODE WIN N IN OUT\n");
        return 2;
    }
    const std::string mode = argv[1];
    const int win = atoi(argv[2]), n = atoi(argv[3]);
    std::vector<float> in;
    if (n < 1 || !read_floats(argv[4], &in) || in.empty() || in.size() % (size_t)n != 0) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    const int chains = (int)(in.size() / (size_t)n);
    std::vector<float> out;
    auto grow = [&]() {
        out.resize(out.size() + (size_t)n);
        return out.data() + out.size() - (size_t)n;
    };
    bool ok = true;
    if (mode == "h" || mode == "hif") {
        ok = (win == 5 || win == 2) && n >= win;
        for (int c = 0; ok && c < chains; ++c) {
            const float *x = &in[(size_t)c * n];
            float *y = grow();
            if (mode == "h") win == 5 ? hrow<5>(x, y, n, -1) : hrow<2>(x, y, n, -1);
            else win == 5 ? hrow_if<5>(x, y, n) : hrow_if<2>(x, y, n);
        }
    } else if (mode == "hck") {
        ok = win == 5 && n >= 5;
        for (int c = 0; ok && c < chains; ++c)
            for (int p = 2; p <= n - 3; ++p) hrow<5>(&in[(size_t)c * n], grow(), n, p);
    } else if (mode == "v" || mode == "vcar") {
        ok = (mode == "v" ? (win == 3 || win == 1) : win == 3) && n >= 3 && chains % 2 == 0;
        for (int c = 0; ok && c < chains; c += 2) {
            const float *x0 = &in[(size_t)c * n], *x1 = x0 + n;
            for (int b = mode == "v" ? -1 : 1; b < (mode == "v" ? 0 : n); ++b) {
                out.resize(out.size() + 2 * (size_t)n);
                float *y0 = out.data() + out.size() - 2 * (size_t)n;
                win == 3 ? vpair<3>(x0, x1, y0, y0 + n, n, b) : vpair<1>(x0, x1, y0, y0 + n, n, b);
            }
        }
    } else {
        ok = false;
    }
    if (!ok) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    FILE *f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size() || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[5]);
        return 2;
    }
    return 0;
}
