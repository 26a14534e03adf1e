// sgm_cost.hip -- census, DSI + horizontal IIR (the vertical IIR runs fused
// with the L3 forward pass in sgm_pair.hip).
// CDNA4 (gfx950) kernels of the semi-global matcher.
//
// Stage map (reference -> kernel), full design in DESIGN.md:
//   cv::GaussianBlur + CT_pts     Solver.cpp:120-140, cost.cpp:99-129  -> census_kernel
//   build_dsi_from_table[_beta]   Solver.cpp:143-248
//     + cost_horizontal_filter    Solver.cpp:296-330                   -> cost_h_kernel (one view slot),
//                                                                         cost_h2_kernel (both),
//                                                                         cost_h_global_kernel (wide rows);
//                                                                         slanted frames: cost_ck_kernel
//                                                                         + vstrip_kernel (sgm_vstrip.hip)
//   cost_vertical_filter          Solver.cpp:333-368                   -> vfwd_kernel (sgm_pair.hip)
//   L1..L8 path DP                SGM.cpp:81-369                       -> stage_a/stage_b kernels,
//                                                                         sweep_kernel (sgm_sweep.hip)
//   aggregation + WTA + unique    SGM.cpp:372-418
//     + compute_subpixel          Solver.cpp:569-597                   -> pair_final_kernel
//   LR check                      SGM.cpp:803-818                      -> lr_kernel
//
// Bit-exactness rules (DESIGN.md "Numerics"): built with -ffp-contract=off,
// no fast-math, correctly rounded f32 division; every float expression keeps
// the reference's association order.
#include "sgm_device.h"

#include "sgm_window_cost_args.h"

#include <type_traits>

namespace sgm {

// ---------------------------------------------------------------- census

// Pinned cv::GaussianBlur(Size(3,3), 2, 1) on CV_8U (Solver.cpp:124-125):
// OpenCV 3.x fixed-point separable filter, kernels {82,93,82} x {70,116,70},
// BORDER_REFLECT_101, (acc + 2^15) >> 16, saturated.  Same formula as
// oracle/sgm_oracle.c:orc_blur (parity unpinned at this boundary).
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// Census inputs: rpitch = bytes between working-grid rows (step * pitch for
// SGM.cpp:47-48's decimation, pitch for BM.cpp:24-25's); step = pixels
// between columns.
constexpr int CT_TW = 64, CT_TH = 16, CT_RPT = CT_TH / 4;  // 4 waves x CT_RPT rows

// CT_pts (cost.cpp:99-129) for one image; window (2HH+1) x (2HWW+1) = 7x9 (3x5
// at scale 2), MSB first, centre skipped, coordinates clamped to the
// (working-grid) edge.  A workgroup owns a 64 x 16 pixel tile:
//   1. the raw pixels the blur of the tile + census apron needs are loaded
//      once (rows/columns lo-1 .. hi+1 at BORDER_REFLECT_101 coordinates);
//   2. the blurred window is built in LDS at clamped coordinates from them;
//   3. each lane walks CT_RPT consecutive rows of its column: every window
//      row is read once and feeds the census words of all the rows whose
//      window holds it (bits appended in row-major order, as the reference).
// Both images in one launch: workgroup z selects (src0, ct0) or (src1, ct1).
//
// MASKED (sgm_set_weighted): CT_pts with WEIGHTED_COST on skips the taps whose
// Gaussian weight is below 0.5 (cost.cpp:115-116), which is the disc weighted_tap_kept; the kept
// taps' bits are appended in the same order, so the word narrows (7 x 9: 50 bits).  CensusBits
// numbers them at compile time; the loops below are unrolled, so a dropped tap costs nothing.
template <int HH, int HWW>
struct CensusBits {
    int k[2 * HH + 1][2 * HWW + 1];  // the tap's bit position (0 = first, MSB); -1: the centre, or dropped
    int nb;
    constexpr CensusBits() : k{}, nb(0) {
        for (int di = 0; di <= 2 * HH; ++di)
            for (int dj = 0; dj <= 2 * HWW; ++dj)
                k[di][dj] = (di != HH || dj != HWW) && weighted_tap_kept(di - HH, dj - HWW) ? nb++ : -1;
    }
};

template <int HH, int HWW, bool MASKED = false>
__global__ __launch_bounds__(256) void census_kernel(const uint8_t *__restrict__ src0,
                                                     const uint8_t *__restrict__ src1, int rpitch,
                                                     int step, int H, int W, int blur,
                                                     uint64_t *__restrict__ ct0,
                                                     uint64_t *__restrict__ ct1) {
    const bool second = __builtin_amdgcn_workgroup_id_z() != 0;
    const uint8_t *__restrict__ src = second ? src1 : src0;
    uint64_t *__restrict__ ct = second ? ct1 : ct0;
    constexpr int TR = CT_TH + 2 * HH, TC = CT_TW + 2 * HWW;
    constexpr int RR = TR + 2, RC = TC + 2;       // raw staging bound
    constexpr int RAW_IT = (RR * RC + 255) / 256;
    __shared__ uint8_t tile[TR][TC];
    __shared__ uint8_t raw[RR][RC];
    const int x0 = bid_x() * CT_TW, y0 = bid_y() * CT_TH;
    const int t = tid_x();
    if (blur) {
        // real rows/columns the clamped window touches, and the raw pixels
        // (one further, reflected) their 3x3 blur reads
        const int ylo = y0 - HH > 0 ? y0 - HH : 0, xlo = x0 - HWW > 0 ? x0 - HWW : 0;
        uint8_t v[RAW_IT];
#pragma unroll
        for (int u = 0; u < RAW_IT; ++u) {
            const int idx = u * 256 + t;
            const int ry = idx / RC, rx = idx - ry * RC;
            const int y = reflect101(clampi(ylo - 1 + ry, -1, H), H);
            const int x = reflect101(clampi(xlo - 1 + rx, -1, W), W);
            v[u] = idx < RR * RC ? src[(size_t)y * rpitch + (size_t)x * step] : 0;
        }
#pragma unroll
        for (int u = 0; u < RAW_IT; ++u) {
            const int idx = u * 256 + t;
            if (idx < RR * RC) (&raw[0][0])[idx] = v[u];
        }
        __syncthreads();
        for (int idx = t; idx < TR * TC; idx += 256) {
            const int ty = idx / TC, tx = idx - ty * TC;
            const int ry = clampi(y0 + ty - HH, 0, H - 1) - ylo;
            const int rx = clampi(x0 + tx - HWW, 0, W - 1) - xlo;
            constexpr int ky[3] = {70, 116, 70};
            int acc = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const uint8_t *row = &raw[ry + r][rx];
                acc += ky[r] * (82 * row[0] + 93 * row[1] + 82 * row[2]);
            }
            const int b = (acc + (1 << 15)) >> 16;  // the pinned blur (top of file)
            tile[ty][tx] = (uint8_t)(b > 255 ? 255 : b);
        }
    } else {
        for (int idx = t; idx < TR * TC; idx += 256) {
            const int ty = idx / TC, tx = idx - ty * TC;
            const int y = clampi(y0 + ty - HH, 0, H - 1), x = clampi(x0 + tx - HWW, 0, W - 1);
            tile[ty][tx] = src[(size_t)y * rpitch + (size_t)x * step];
        }
    }
    __syncthreads();
    const int tx = t & 63, r0 = wave_id() * CT_RPT;
    constexpr CensusBits<HH, HWW> CB{};
    constexpr int NB = MASKED ? CB.nb : (2 * HH + 1) * (2 * HWW + 1) - 1;  // census bits (62 at 7x9)
    static_assert(NB <= 64, "census word");
    constexpr int NHI = NB > 32 ? NB - 32 : 0;            // bits in the high word
    int c[CT_RPT];
#pragma unroll
    for (int p = 0; p < CT_RPT; ++p) c[p] = tile[r0 + p + HH][tx + HWW];
    unsigned hi[CT_RPT], lo[CT_RPT];
#pragma unroll
    for (int p = 0; p < CT_RPT; ++p) hi[p] = lo[p] = 0;
    // window row rr (tile row r0 + rr) is row di = rr - HH - p of pixel p
#pragma unroll
    for (int rr = 0; rr < CT_RPT + 2 * HH; ++rr) {
        int b[2 * HWW + 1];
#pragma unroll
        for (int dj = 0; dj <= 2 * HWW; ++dj) b[dj] = tile[r0 + rr][tx + dj];
#pragma unroll
        for (int p = 0; p < CT_RPT; ++p) {
            const int di = rr - p;  // 0 .. 2HH within the window
            if (di < 0 || di > 2 * HH) continue;
#pragma unroll
            for (int dj = 0; dj <= 2 * HWW; ++dj) {
                if (di == HH && dj == HWW) continue;
                // bit position k (0 = first, MSB) of the reference's order
                const int k = MASKED ? CB.k[di][dj]
                                     : di * (2 * HWW + 1) + dj - (di * (2 * HWW + 1) + dj > HH * (2 * HWW + 1) + HWW ? 1 : 0);
                if (MASKED && k < 0) continue;
                // (c - b) has its sign bit set iff b > c (bytes, no overflow):
                // w << 1 | x >> 31 is one funnel shift (v_alignbit_b32)
                const unsigned x = (unsigned)(c[p] - b[dj]);
                if (k < NHI) hi[p] = (hi[p] << 1) | (x >> 31);
                else lo[p] = (lo[p] << 1) | (x >> 31);
            }
        }
    }
    const int x = x0 + tx;
#pragma unroll
    for (int p = 0; p < CT_RPT; ++p) {
        const int y = y0 + r0 + p;
        if (y < H && x < W) ct[(size_t)y * W + x] = ((uint64_t)hi[p] << 32) | lo[p];
    }
}

// The census of a window other than the default (sgm_set_window):
// census_kernel<HH, HWW> itself, instantiated for every accepted pair of half
// sizes 0 .. 4 (not 0 x 0: no tap; not 4 x 4: 80 bits) and picked from a table.
// The bit order, the hi / lo split and the clamping are the template's, so a
// window of at most 32 bits fills lo only and 5 x 7's 34 bits put 2 in hi.
using CensusFn = void (*)(const uint8_t *, const uint8_t *, int, int, int, int, int, uint64_t *, uint64_t *);
template <int HH, int HWW>
constexpr CensusFn census_fn() {
    if constexpr ((HH == 0 && HWW == 0) || (2 * HH + 1) * (2 * HWW + 1) - 1 > 64)
        return nullptr;
    else
        return census_kernel<HH, HWW>;
}
#define SGM_CENSUS_ROW(HH) \
    { census_fn<HH, 0>(), census_fn<HH, 1>(), census_fn<HH, 2>(), census_fn<HH, 3>(), census_fn<HH, 4>() }
static const CensusFn kCensusTable[5][5] = {SGM_CENSUS_ROW(0), SGM_CENSUS_ROW(1), SGM_CENSUS_ROW(2),
                                            SGM_CENSUS_ROW(3), SGM_CENSUS_ROW(4)};
#undef SGM_CENSUS_ROW

// The masked census of a weighted handle (sgm_set_weighted): an entry for every
// accepted pair of half sizes whose corners lie outside the disc (7 x 9, 9 x 7, 7 x 7, 5 x 9,
// 9 x 5); null where the disc keeps every tap and the unmasked kernel is the masked one.
template <int HH, int HWW>
constexpr CensusFn census_masked_fn() {
    if constexpr (census_fn<HH, HWW>() == nullptr || weighted_bits(HH, HWW) == (2 * HH + 1) * (2 * HWW + 1) - 1)
        return nullptr;
    else
        return census_kernel<HH, HWW, true>;
}
#define SGM_CENSUS_ROW(HH)                                                                                \
    {                                                                                                     \
        census_masked_fn<HH, 0>(), census_masked_fn<HH, 1>(), census_masked_fn<HH, 2>(),                   \
            census_masked_fn<HH, 3>(), census_masked_fn<HH, 4>()                                           \
    }
static const CensusFn kCensusMaskedTable[5][5] = {SGM_CENSUS_ROW(0), SGM_CENSUS_ROW(1), SGM_CENSUS_ROW(2),
                                                  SGM_CENSUS_ROW(3), SGM_CENSUS_ROW(4)};
#undef SGM_CENSUS_ROW

hipError_t launch_census(const uint8_t *src, int pitch, Geom g, Window win, int blur, uint64_t *ct,
                         hipStream_t st, bool bm_rows, const uint8_t *src2, uint64_t *ct2) {
    dim3 grid((g.W + CT_TW - 1) / CT_TW, (g.H + CT_TH - 1) / CT_TH, src2 ? 2 : 1);
    const int rpitch = bm_rows ? pitch : pitch * g.scale;
    if (win.weighted) {
        if (win.eh < 1 || win.ew < 1 || win.eh % 2 == 0 || win.ew % 2 == 0 || win.hh() > 4 || win.hw() > 4)
            return hipErrorInvalidValue;
        if (const CensusFn masked = kCensusMaskedTable[win.hh()][win.hw()]) {
            hipLaunchKernelGGL(masked, grid, dim3(256), 0, st, src, src2, rpitch, g.scale, g.H, g.W, blur, ct, ct2);
            return hipGetLastError();
        }
    }
    const Window def = default_window(g.scale);
    if (win.hh() != def.hh() || win.hw() != def.hw()) {
        if (win.eh < 1 || win.ew < 1 || win.hh() > 4 || win.hw() > 4 || !kCensusTable[win.hh()][win.hw()])
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(kCensusTable[win.hh()][win.hw()], grid, dim3(256), 0, st, src, src2, rpitch, g.scale,
                           g.H, g.W, blur, ct, ct2);
        return hipGetLastError();
    }
    if (g.scale == 1)
        census_kernel<3, 4><<<grid, 256, 0, st>>>(src, src2, rpitch, 1, g.H, g.W, blur, ct, ct2);
    else
        census_kernel<1, 2><<<grid, 256, 0, st>>>(src, src2, rpitch, 2, g.H, g.W, blur, ct, ct2);
    return hipGetLastError();
}

// ------------------------------------------ shifted tables (min_disp)

// sgm_set_min_disp(h, m) searches disparities [m, m + D): with k = m / scale,
// the left view's DSI is today's [0, D) DSI of (ctl, ctr_s), ctr_s[i, x] =
// ctr[i, max(x - k, 0)], and the right view's that of (ctl_s, ctr), ctl_s[i, x]
// = ctl[i, min(x + k, W-1)] (max(x - k - ds, 0) = max(max(x - k, 0) - ds, 0) and
// the same for min), so the cost kernels' staging and padding stay as they
// are.  One word per lane, 256 consecutive words of a row per workgroup: the
// stores are whole cache lines, the loads the same lines k words aside (or the
// row's edge word).  Workgroup z selects the table; a null output is skipped.
__global__ __launch_bounds__(256) void ct_shift_kernel(const uint64_t *__restrict__ ctl,
                                                       const uint64_t *__restrict__ ctr,
                                                       uint64_t *__restrict__ ctl_s,
                                                       uint64_t *__restrict__ ctr_s, int W, int k) {
    const bool right = __builtin_amdgcn_workgroup_id_z() != 0;
    const uint64_t *__restrict__ src = right ? ctr : ctl;
    uint64_t *__restrict__ dst = right ? ctr_s : ctl_s;
    const int x = bid_x() * 256 + tid_x();
    if (dst == nullptr || x >= W) return;
    const size_t row = (size_t)bid_y() * W;
    const int xs = right ? (x - k > 0 ? x - k : 0) : (x + k < W - 1 ? x + k : W - 1);
    dst[row + x] = src[row + xs];
}

hipError_t launch_ct_shift(const uint64_t *ctl, const uint64_t *ctr, uint64_t *ctl_s, uint64_t *ctr_s,
                           int k, Geom g, hipStream_t st) {
    // (k can exceed W: x - k and x + k stay far inside int for every accepted min_disp)
    ct_shift_kernel<<<dim3((g.W + 255) / 256, g.H, 2), 256, 0, st>>>(ctl, ctr, ctl_s, ctr_s, g.W, k);
    return hipGetLastError();
}

// ------------------------------------------------ DSI + horizontal IIR

// One thread per (row, d) chain, R rows per block (R*D threads).  The census
// rows of both images (and the sky row) are staged in LDS once per block,
// padded on both sides with copies of the edge words so the clamped lookups
// of Solver.cpp:143-248 become plain offsets; the raw Hamming DSI (sky
// override :165-178) is produced on the fly and fed straight into the
// in-place horizontal IIR of Solver.cpp:296-330, restated with a register
// history: with h = WIN/2 and LAG = WIN-h-1 the reference writes position
// LAG+t at step t, adds raw[WIN+t] and subtracts the value at position t,
// which is the step-(t-LAG) output once t >= LAG and raw before.
//
// The IIR is one serial chain per (row, d) and a frame has only H*D of them
// (750 waves at KITTI D=128), so a wave's step latency is the kernel time:
// the main loop runs blocks of COSTH_U steps with no branches, their raw
// costs fetched one block ahead.
constexpr int COSTH_MAX_LDS = 64 * 1024;

// The horizontally filtered volume is read once, by vfwd: non-temporal stores
// keep it from evicting the final cost C from the Infinity Cache (default-
// policy stores: cost_h 58 -> 50 us but vfwd and stage A slower, r02 and
// profiles/r03_experiments/inplace_c.txt).
__device__ __forceinline__ void costh_store(float v, float *p) { __builtin_nontemporal_store(v, p); }
constexpr int COSTH_U = 8;

__host__ __device__ constexpr int costh_pad(int D, int scale) { return D / scale + 2 * COSTH_U; }

// The checkpoint pass's store (cost_h_body<..., CK> and cost_ck_body): the
// chain's restart state (HCheckpoint, sgm_cost_iir.h) as 3 floats ds apart.
__device__ __forceinline__ void ck_write(const HFilter<5> &f, float *q, size_t ds) {
    HCheckpoint ck;
    ck.save(f);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k * ds] = ck.v[k];
}

// UNI (D >= 64, one row per wave): the census word every lane of a row needs
// at step j -- cl[j] for the left view, cr[j] for the right -- is a uniform
// scalar load from global memory; only the per-lane shifted row is staged in
// LDS, which halves the staging and keeps 4K rows (3840 px) inside 64 KiB.
// DC: D as a compile-time constant (0: runtime D), so the stores of an
// unrolled block take immediate offsets instead of a 64-bit address add each
// CK > 0 (the strip schedule's checkpoint pass, sgm_vstrip.hip): no volume
// is written; at every output position p = CK * s (2 <= p <= W-3) the state
// before the step that produces p -- the running sum and the values at
// positions p-2, p-1 it will subtract -- goes to out[((i * ck_ns + s) * 3 +
// k) * D + d], k = 0 .. 2.
template <int VIEW, int WIN, bool SKY, bool FILTER, bool UNI, int DC = 0, int CK = 0>
__device__ __forceinline__ void cost_h_body(const uint64_t *__restrict__ ctl,
                                            const uint64_t *__restrict__ ctr,
                                            const uint8_t *__restrict__ sky, int sky_pitch, int H,
                                            int W, int D, int scale, int R,
                                            float *__restrict__ out, int blk, unsigned char *smem,
                                            int ck_ns = 0) {
    static_assert(CK == 0 || (WIN == 5 && FILTER), "checkpoints of the 5-wide filter");
    const int P = costh_pad(D, scale), RS = W + 2 * P;
    constexpr int NS = UNI ? 1 : 2;  // staged census rows per image row
    uint64_t *sl = reinterpret_cast<uint64_t *>(smem);
    uint64_t *sr = sl + (UNI ? 0 : (size_t)R * RS);
    uint8_t *ss = reinterpret_cast<uint8_t *>(sl + (size_t)NS * R * RS);
    const int row0 = blk * R;
    for (int idx = tid_x(); idx < R * RS; idx += R * D) {
        const int r = idx / RS, jp = idx - r * RS, i = row0 + r;
        const int j = clampi(jp - P, 0, W - 1);
        if (i < H) {
            if (!UNI || VIEW == 1) sl[idx] = ctl[(size_t)i * W + j];
            if (!UNI || VIEW == 0) sr[idx] = ctr[(size_t)i * W + j];
            if (SKY) ss[idx] = sky[(size_t)i * sky_pitch + j];
        }
    }
    __syncthreads();
    const int r = UNI ? uniform(tid_x() / D) : tid_x() / D, d = tid_x() - r * D;
    const int i = row0 + r;
    if (i >= H) return;
    const int ds = d / scale;
    // raw(j) reads cl[j (+ds)] and cr[j (-ds)] through the padded rows
    const uint64_t *cl = sl + (size_t)r * RS + P + (VIEW == 1 ? ds : 0);
    const uint64_t *cr = sr + (size_t)r * RS + P - (VIEW == 0 ? ds : 0);
    const uint64_t *cu = (VIEW == 0 ? ctl : ctr) + (size_t)i * W;  // UNI: the uniform row
    const uint8_t *sk = ss + (size_t)r * RS + P;
    float *o = out + (CK ? (size_t)i * ck_ns * 3 * D : (size_t)i * W * D) + d;
    const size_t DS = DC ? (size_t)DC : (size_t)D;  // store stride

    auto word_l = [&](int j) { return UNI && VIEW == 0 ? cu[j < W - 1 ? j : W - 1] : cl[j]; };
    auto word_r = [&](int j) { return UNI && VIEW == 1 ? cu[j < W - 1 ? j : W - 1] : cr[j]; };

    auto raw = [&](int j) -> float {
        const float c = hamming(word_l(j), word_r(j));
        if (SKY) {
            const float sv = d == 0 ? 0.0f : 999999.0f;
            return sk[j] == 255 ? sv : c;
        }
        return c;
    };

    if (!FILTER) {
        for (int j = 0; j < W; ++j) costh_store(raw(j), o + (size_t)j * DS);
        return;
    }
    // The recursion is HFilter<WIN>'s (sgm_cost_iir.h: init, out, advance), written out here with
    // a history array of its own: through the type hipcc schedules the 5-wide chain differently,
    // and the one-view kernel at 375 x 1242 x 128, which here runs in one of two modes (47-48 us
    // or 54-59 us), sat at 56 us in both (paired A/B, profiles/cost_iir_isa.txt section 3).  The
    // header's CPU test and the GPU tests pin both forms to the oracle.
    constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1, U = COSTH_U;
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) sum += raw(k);
    if constexpr (CK == 0) {
#pragma unroll
        for (int p = 0; p < LAG; ++p) costh_store(raw(p), o + (size_t)p * DS);
    }
    const int T = W - 2 * HALF;
    // hist[0] is what step t subtracts: raw[t] for t < LAG, output t-LAG after
    float hist[LAG > 0 ? LAG : 1];
#pragma unroll
    for (int p = 0; p < LAG; ++p) hist[p] = raw(p);
    auto ck_store = [&](int p) {
        if constexpr (CK > 0) {
            if (p % CK == 0) ck_write(HFilter<5>{sum, {hist[0], hist[LAG - 1]}}, o + (size_t)(p / CK) * 3 * DS, DS);
        }
    };
    auto step = [&](int t, float rw) {
        ck_store(LAG + t);
        const float v = div_win<WIN>(sum);
        if constexpr (CK == 0) costh_store(v, o + (size_t)(LAG + t) * DS);
        sum += rw;
        float a;
        if constexpr (LAG == 0) {
            a = v;
        } else {
            a = hist[0];
#pragma unroll
            for (int p = 0; p + 1 < LAG; ++p) hist[p] = hist[p + 1];
            hist[LAG - 1] = v;
        }
        sum -= a;
    };
    // steps t < T-1 also add raw[WIN+t]; the last step only writes.  The
    // next block's census words (and sky bytes) are loaded before the current
    // block's steps run and only turned into costs after them, so the LDS
    // round trips overlap the serial chain.
    int t = 0;
    float cur[U];
    if (T - 1 >= U) {
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = raw(WIN + u);
    }
    for (; t + 2 * U <= T - 1; t += U) {
        uint64_t nl[U], nr[U];
        uint8_t nk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = WIN + t + U + u;
            nl[u] = word_l(j);
            nr[u] = word_r(j);
            if (SKY) nk[u] = sk[j];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) step(t + u, cur[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float c = hamming(nl[u], nr[u]);
            if (SKY) cur[u] = nk[u] == 255 ? (d == 0 ? 0.0f : 999999.0f) : c;
            else cur[u] = c;
        }
    }
    if (t + U <= T - 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) step(t + u, cur[u]);
        t += U;
    }
    for (; t < T - 1; ++t) step(t, raw(WIN + t));
    if constexpr (CK > 0) {
        if (T >= 1) ck_store(LAG + T - 1);
        return;
    }
    if (T >= 1) costh_store(div_win<WIN>(sum), o + (size_t)(LAG + T - 1) * DS);
    for (int p = LAG + T; p < W; ++p) costh_store(raw(p), o + (size_t)p * DS);
}

template <int VIEW, int WIN, bool SKY, bool FILTER, bool UNI, int DC>
__global__ __launch_bounds__(256) void cost_h_kernel(const uint64_t *__restrict__ ctl,
                                                     const uint64_t *__restrict__ ctr,
                                                     const uint8_t *__restrict__ sky,
                                                     int sky_pitch, int H, int W, int D, int scale,
                                                     int R, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cost_h_body<VIEW, WIN, SKY, FILTER, UNI, DC>(ctl, ctr, sky, sky_pitch, H, W, D, scale, R, out,
                                             bid_x(), smem);
}

// Both view slots in one launch (workgroup z = slot): the DSI of
// build_dsi_from_table into out0 and of build_dsi_from_table_beta into out1,
// each with its own sky mask.  A view's H*D chains fill less than the chip at
// KITTI sizes, so the two views' chains run side by side.  Each slot reads its
// own table pair: slot 0 (ctl, ctr_s), slot 1 (ctl_s, ctr) (census_tables,
// sgm_internal.h).  A kernel of its own beside cost_h_kernel, and bare pointer
// parameters in both: as one template over Views<CostSlot, NV> the
// uniform-operand forms lost scalar loads to vector ones
// (profiles/cost_stage_merge_codegen.txt).
template <int WIN, bool SKY, bool FILTER, bool UNI, int DC>
__global__ __launch_bounds__(256) void cost_h2_kernel(const uint64_t *__restrict__ ctl,
                                                      const uint64_t *__restrict__ ctr,
                                                      const uint64_t *__restrict__ ctl_s,
                                                      const uint64_t *__restrict__ ctr_s,
                                                      const uint8_t *__restrict__ sky0,
                                                      const uint8_t *__restrict__ sky1,
                                                      int sky_pitch, int H, int W, int D, int scale,
                                                      int R, float *__restrict__ out0,
                                                      float *__restrict__ out1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (__builtin_amdgcn_workgroup_id_z() == 0)
        cost_h_body<0, WIN, SKY, FILTER, UNI, DC>(ctl, ctr_s, sky0, sky_pitch, H, W, D, scale, R, out0,
                                              bid_x(), smem);
    else
        cost_h_body<1, WIN, SKY, FILTER, UNI, DC>(ctl_s, ctr, sky1, sky_pitch, H, W, D, scale, R, out1,
                                              bid_x(), smem);
}

// Fallback for rows too wide to stage in LDS (W*16 B > 64 KiB): census words
// read straight from global memory.
template <int VIEW, int WIN, bool SKY, bool FILTER>
__global__ __launch_bounds__(256) void cost_h_global_kernel(const uint64_t *__restrict__ ctl,
                                                            const uint64_t *__restrict__ ctr,
                                                            const uint8_t *__restrict__ sky,
                                                            int sky_pitch, int H, int W, int D,
                                                            int scale, float *__restrict__ out) {
    const int rows_per_block = 256 / D;
    const int r = tid_x() / D, d = tid_x() - r * D;
    const int i = bid_x() * rows_per_block + r;
    if (i >= H) return;
    const uint64_t *cl = ctl + (size_t)i * W;
    const uint64_t *cr = ctr + (size_t)i * W;
    const uint8_t *sk = SKY ? sky + (size_t)i * sky_pitch : nullptr;
    const int ds = d / scale;
    float *o = out + (size_t)i * W * D + d;
    auto raw = [&](int j) -> float {
        if (SKY && sk[j] == 255) return d == 0 ? 0.0f : 999999.0f;
        const uint64_t a = VIEW == 0 ? cl[j] : cl[min(j + ds, W - 1)];
        const uint64_t b = VIEW == 0 ? cr[max(j - ds, 0)] : cr[j];
        return hamming(a, b);
    };
    if (!FILTER) {
        for (int j = 0; j < W; ++j) costh_store(raw(j), o + (size_t)j * D);
        return;
    }
    constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1;
    HFilter<WIN> f;  // the recursion: sgm_cost_iir.h
    float first[WIN];
#pragma unroll
    for (int k = 0; k < WIN; ++k) first[k] = raw(k);
    f.init(first);
#pragma unroll
    for (int p = 0; p < LAG; ++p) costh_store(first[p], o + (size_t)p * D);
    const int T = W - 2 * HALF;
    for (int t = 0; t < T; ++t) {
        const float v = f.out();
        costh_store(v, o + (size_t)(LAG + t) * D);
        if (t == T - 1) break;
        f.advance(v, raw(WIN + t));
    }
    for (int p = LAG + T; p < W; ++p) costh_store(raw(p), o + (size_t)p * D);
}

// the staged kernels' form (UNI), rows per block (R = 0: the global-memory
// fallback) and LDS bytes
struct CosthShape {
    bool uni;
    int R;
    size_t smem;
};
static CosthShape costh_shape(Geom g, bool sky) {
    const size_t rs = (size_t)(g.W + 2 * costh_pad(g.D, g.scale));
    const bool uni = g.D >= 64 && rs * (16 + (sky ? 1 : 0)) > (size_t)COSTH_MAX_LDS;
    const size_t row_bytes = rs * ((uni ? 8 : 16) + (sky ? 1 : 0));
    int R = (int)(COSTH_MAX_LDS / row_bytes);
    if (R > 256 / g.D) R = 256 / g.D;
    return {uni, R, (size_t)R * row_bytes};
}

bool cost_h_staged(const CostSlot *s, int nviews, Geom g) {
    return costh_shape(g, s->sky != nullptr).R >= 1 &&
           (nviews == 1 || (s[0].sky == nullptr) == (s[1].sky == nullptr));
}

// f(tags...): each flag as std::true_type or std::false_type, which a generic
// lambda names in constant expressions (as for_width's tags, sgm_bodies.h)
template <class F>
static void for_flags(F &&f) {
    f();
}
template <class F, class... B>
static void for_flags(F &&f, bool b, B... rest) {
    if (b) for_flags([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else for_flags([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

// The staged kernels' form, f(UNI, DC): both census rows staged when they fit
// (faster: LDS reads for both operands), D = 128 as a constant; rows too wide
// for that (4K) stage one and load the uniform operand as scalars
template <class F>
static void for_staged_form(bool uni, int D, F &&f) {
    if (uni) f(std::true_type{}, std::integral_constant<int, 0>{});
    else if (D == 128) f(std::false_type{}, std::integral_constant<int, 128>{});
    else f(std::false_type{}, std::integral_constant<int, 0>{});
}

// whether the slots are a launch's: one of either DSI, or (DSI 0, DSI 1)
static bool slots_ok(const CostSlot *s, int nviews) {
    return nviews == 1 ? (s->dsi == 0 || s->dsi == 1) : (nviews == 2 && s[0].dsi == 0 && s[1].dsi == 1);
}

hipError_t launch_cost_h(const CostSlot *s, int nviews, int sky_pitch, int filter, Geom g, hipStream_t st) {
    if (!slots_ok(s, nviews) || (nviews == 2 && !(filter && cost_h_staged(s, 2, g)))) return hipErrorInvalidValue;
    const CosthShape sh = costh_shape(g, s->sky != nullptr);
    const int rpb = sh.R >= 1 ? sh.R : 256 / g.D;  // rows per block (the fallback: of 256 threads)
    const dim3 grid((g.H + rpb - 1) / rpb, 1, nviews);
    for_flags(
        [&](auto SKY, auto FILTER, auto WIN5) {
            constexpr int WIN = WIN5 ? 5 : 2;
            if (nviews == 2) {  // both slots: staged and filtered (checked above)
                if constexpr (FILTER) {
                    const CensusTables t = census_tables(s, 2);
                    for_staged_form(sh.uni, g.D, [&](auto UNI, auto DC) {
                        cost_h2_kernel<WIN, SKY, FILTER, UNI, DC><<<grid, sh.R * g.D, sh.smem, st>>>(
                            t.ctl, t.ctr, t.ctl_s, t.ctr_s, s[0].sky, s[1].sky, sky_pitch, g.H, g.W, g.D, g.scale,
                            sh.R, s[0].ch, s[1].ch);
                    });
                }
                return;
            }
            for_flags(
                [&](auto RIGHT) {  // one slot: its DSI
                    constexpr int VIEW = RIGHT ? 1 : 0;
                    if (sh.R >= 1) {
                        for_staged_form(sh.uni, g.D, [&](auto UNI, auto DC) {
                            cost_h_kernel<VIEW, WIN, SKY, FILTER, UNI, DC><<<grid, sh.R * g.D, sh.smem, st>>>(
                                s->ctl, s->ctr, s->sky, sky_pitch, g.H, g.W, g.D, g.scale, sh.R, s->ch);
                        });
                    } else {
                        cost_h_global_kernel<VIEW, WIN, SKY, FILTER><<<grid, 256, 0, st>>>(
                            s->ctl, s->ctr, s->sky, sky_pitch, g.H, g.W, g.D, g.scale, s->ch);
                    }
                },
                s->dsi == 1);
        },
        s->sky != nullptr, filter != 0, g.scale == 1);
    return hipGetLastError();
}

// The checkpoint pass's chain (sgm_vstrip.hip): the horizontal IIR (WIN = 5,
// no sky mask), storing only the state at every strip edge.  Its
// bytes are negligible, so the chains' latency is its time: the steps run in
// blocks of one strip (U = kVStripNC) that start at an edge, so the
// checkpoint is the block's first action (no branch), and the next block's
// census words are loaded one block ahead -- the uniform row (UNI) by scalar
// loads: SMEM returns out of order, so its waits are lgkmcnt(0), which hipcc
// placed right before each block.
template <int VIEW, bool UNI>
__device__ __forceinline__ void cost_ck_body(const uint64_t *__restrict__ ctl,
                                             const uint64_t *__restrict__ ctr, int H, int W, int D,
                                             int R, float *__restrict__ out, int blk,
                                             unsigned char *smem, int ns) {
    constexpr int U = kVStripNC;
    const int P = costh_pad(D, 1), RS = W + 2 * P;
    uint64_t *sl = reinterpret_cast<uint64_t *>(smem);
    uint64_t *sr = sl + (UNI ? 0 : (size_t)R * RS);
    const int row0 = blk * R;
    // (cost_h_body's staging loop without the sky row)
    for (int idx = tid_x(); idx < R * RS; idx += R * D) {
        const int r = idx / RS, jp = idx - r * RS, i = row0 + r;
        const int j = clampi(jp - P, 0, W - 1);
        if (i < H) {
            if (!UNI || VIEW == 1) sl[idx] = ctl[(size_t)i * W + j];
            if (!UNI || VIEW == 0) sr[idx] = ctr[(size_t)i * W + j];
        }
    }
    __syncthreads();
    const int r = UNI ? uniform(tid_x() / D) : tid_x() / D, d = tid_x() - r * D;
    const int i = row0 + r;
    if (i >= H) return;
    const uint64_t *cl = sl + (size_t)r * RS + P + (VIEW == 1 ? d : 0);
    const uint64_t *cr = sr + (size_t)r * RS + P - (VIEW == 0 ? d : 0);
    const uint64_t *cu = (VIEW == 0 ? ctl : ctr) + (size_t)i * W;
    float *o = out + (size_t)i * ns * 3 * D + d;
    // the shifted operand (LDS) and the other one (UNI: global) of position
    // j <= W-1 (positions past the row are clamped; their costs feed nothing)
    auto wu = [&](int j) { return UNI ? cu[j] : (VIEW == 0 ? cl[j] : cr[j]); };
    auto ws = [&](int j) { return VIEW == 0 ? cr[j] : cl[j]; };
    auto raw = [&](int j) {
        j = min(j, W - 1);
        return VIEW == 0 ? hamming(wu(j), ws(j)) : hamming(ws(j), wu(j));
    };
    HFilter<5> f;  // the recursion: sgm_cost_iir.h
    float first[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) first[k] = raw(k);
    f.init(first);
    const int T = W - 4;  // steps: output position t+2; steps t < T-1 update
    auto step = [&](float rw) { f.advance(f.out(), rw); };
    auto ck_store = [&](int s) { ck_write(f, o + (size_t)s * 3 * D, (size_t)D); };
    // a step with its conditions (the prologue and the tail): the checkpoint
    // of the strip starting at position t+2, then the update
    auto gstep = [&](int t) {
        if ((t + 2) % U == 0) ck_store((t + 2) / U);
        if (t < T - 1) step(raw(t + 5));
    };
    int t = 0;
    for (; t < U - 2 && t < T; ++t) gstep(t);
    // full blocks b (steps U*b-2 .. U*b+U-3, all updating): U*(b+1) - 2 < T
    int b = 1;
    if (U * (b + 1) - 2 < T) {
        float cur[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = raw(U * b + 3 + u);
        for (; U * (b + 1) - 2 < T; ++b) {
            uint64_t nu[U], nw[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = min(U * (b + 1) + 3 + u, W - 1);
                nu[u] = wu(j);
                nw[u] = ws(j);
            }
            // (scheduling fences: else hipcc pulls each word's hamming up next
            // to its load and waits for it inside the chain)
            __builtin_amdgcn_sched_barrier(0);
            ck_store(b);
#pragma unroll
            for (int u = 0; u < U; ++u) step(cur[u]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = VIEW == 0 ? hamming(nu[u], nw[u]) : hamming(nw[u], nu[u]);
        }
        t = U * b - 2;
    }
    for (; t < T; ++t) gstep(t);
}

// The strip schedule's checkpoint pass (sgm_vstrip.hip): each view slot's
// horizontal IIR state at every strip edge, both slots in one launch
// (workgroup z = slot; dsi0/dsi1: the slot's DSI, 0 left view, 1 right: it
// reads (ctl, ctr_s) or (ctl_s, ctr), as cost_h2_kernel's slots; a one-slot
// launch of DSI 1 is a right-view handle's).
template <bool SKY, bool UNI, int DC>
__global__ __launch_bounds__(256) void cost_ck_kernel(const uint64_t *__restrict__ ctl,
                                                      const uint64_t *__restrict__ ctr,
                                                      const uint64_t *__restrict__ ctl_s,
                                                      const uint64_t *__restrict__ ctr_s,
                                                      const uint8_t *__restrict__ sky0,
                                                      const uint8_t *__restrict__ sky1, int sky_pitch,
                                                      int H, int W, int D, int R, float *__restrict__ out0,
                                                      float *__restrict__ out1, int dsi0, int dsi1, int ns) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const bool z = __builtin_amdgcn_workgroup_id_z() != 0;
    if constexpr (!SKY) {
        if ((z ? dsi1 : dsi0) == 0) cost_ck_body<0, UNI>(ctl, ctr_s, H, W, D, R, z ? out1 : out0, bid_x(), smem, ns);
        else cost_ck_body<1, UNI>(ctl_s, ctr, H, W, D, R, z ? out1 : out0, bid_x(), smem, ns);
    } else if ((z ? dsi1 : dsi0) == 0) {
        cost_h_body<0, 5, SKY, true, UNI, DC, kVStripNC>(ctl, ctr_s, z ? sky1 : sky0, sky_pitch, H, W, D, 1, R,
                                                         z ? out1 : out0, bid_x(), smem, ns);
    } else {
        cost_h_body<1, 5, SKY, true, UNI, DC, kVStripNC>(ctl_s, ctr, z ? sky1 : sky0, sky_pitch, H, W, D, 1, R,
                                                         z ? out1 : out0, bid_x(), smem, ns);
    }
}

hipError_t launch_cost_ck(const CostSlot *s, int nviews, int sky_pitch, Geom g, hipStream_t st) {
    if (!slots_ok(s, nviews) || !vstrip_supported(s, nviews, g)) return hipErrorInvalidValue;
    const CosthShape sh = costh_shape(g, s->sky != nullptr);
    const dim3 grid((g.H + sh.R - 1) / sh.R, 1, nviews);
    const int ns = (int)vstrip_strips(g);
    const CensusTables t = census_tables(s, nviews);
    const CostSlot &b = s[nviews - 1];
    // (census operands straight from global memory instead of the staged
    // rows measured slower: HD256 610 vs 317 us, 4K256 2.33 vs 1.82 ms; one
    // row per block, for more waves per CU, changed nothing:
    // profiles/r06_experiments/r06q_vstrip.txt)
    for_flags(
        [&](auto SKY) {
            for_staged_form(sh.uni, g.D, [&](auto UNI, auto DC) {
                cost_ck_kernel<SKY, UNI, DC><<<grid, sh.R * g.D, sh.smem, st>>>(
                    t.ctl, t.ctr, t.ctl_s, t.ctr_s, s->sky, b.sky, sky_pitch, g.H, g.W, g.D, sh.R, s->ch, b.ch, s->dsi,
                    b.dsi, ns);
            });
        },
        s->sky != nullptr);
    return hipGetLastError();
}

// ------------------------------------------------------ vertical pass

// The vertical IIR (Solver.cpp:333-368) runs fused with the L3 forward pass in
// sgm_pair.hip (vfwd_kernel); without the filter the volume is copied.
__global__ __launch_bounds__(256) void copy_kernel(const float *__restrict__ in,
                                                   float *__restrict__ out, size_t n) {
    const size_t i = (size_t)bid_x() * 256 + tid_x();
    if (i < n) out[i] = in[i];
}

hipError_t launch_copy(const float *in, float *out, Geom g, hipStream_t st) {
    const size_t n = (size_t)g.W * g.D * g.H;
    copy_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(in, out, n);
    return hipGetLastError();
}


}  // namespace sgm
