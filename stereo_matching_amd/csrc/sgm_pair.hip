// sgm_pair.hip -- forward/backward path pairs with checkpoint recompute.
//
// Two opposite directions on the same scanlines (L1/L2 rows, L3/L4 columns,
// L6/L7 wrapped anti-diagonals) are computed by one forward kernel that only
// stores its path state every K steps, and one backward kernel that, per
// K-step segment, recomputes the forward costs from the checkpoint into
// registers (reading each cost once for both directions) and combines
//   S12 = L1 + L2, T = (T5 + L6) + L7, total = ((S12 + L3) + L4) + T
// on the fly -- the reference's association order (SGM.cpp:386-390) -- so no
// single-direction volume is ever written (DESIGN.md "Pairs").
//
// Segments are counted from the END of a chain of n steps: segment 0 covers
// positions [0, r0) with r0 = n - (nseg-1)*K, segment s >= 1 covers
// [r0 + (s-1)K, r0 + sK).  Checkpoint m (0 <= m < nseg-1) is the forward state
// after position r0-1 + mK and seeds segment m+1.  The backward pass therefore
// meets full segments first and the partial one last.
//
// The file holds every aggregation role of the frame schedules but the L8
// sweep (sgm_sweep.hip), with one launcher per role; a
// launch takes the views of r[0 .. nviews) (ViewRoles, sgm_internal.h).
#include "sgm_bodies.h"

namespace sgm {


static inline int chain_len(int family, Geom g) { return family == PAIR_H ? g.W : g.H; }
static inline int num_chains(int family, Geom g) { return family == PAIR_H ? g.H : g.W; }

size_t pair_ckpt_floats(int family, Geom g) {
    const int V = vals_per_lane(g.D);
    const int K = family == PAIR_V ? seg_k_v(V) : seg_k_hd(V);
    const int n = chain_len(family, g);
    const size_t nseg = (size_t)((n + K - 1) / K);
    return (size_t)num_chains(family, g) * nseg * g.D;
}

// ------------------------------------------------------------ kernels
//
// One kernel template per role where the two-view form allocates the
// registers its stand-alone copy did: stage A, the finals, the L8 sweep and
// h_fwd take Views<args, NV> (sgm_device.h); NV = 2 runs both views of a
// two-view frame in one launch, where one view's chains leave the chip
// under-filled or nothing is gained by finishing one view first.  vfwd, stage
// B, the H pair and h_bwd keep a two-view kernel of their own (vfwd2_kernel,
// stage_b2_kernel; hpair_kernel and h_bwd2_kernel always take two views): as
// Views<> instantiations they came out with other VGPR counts
// (profiles/view_merge_codegen.txt).  Each role still has one launcher.

// vfwd_body (sgm_bodies.h): the vertical IIR fused with the L3 forward pass,
// one wave per column.
template <int V, bool FULL, int WIN, int PF, bool BAND = false, bool L3OUT = false>
__global__ __launch_bounds__(64) void vfwd_kernel(const float *__restrict__ in,
                                                  float *__restrict__ out, PairArgs a, Geom g) {
    vfwd_body<V, FULL, WIN, PF, BAND, L3OUT>(in, out, a, g, bid_x(), tid_x());
}

// Both views' vertical passes in one launch, workgroup y = view: W chains per
// view leave about one wave per SIMD at KITTI and two at HD, one launch of 2W
// twice that.  L3OUT: writing C and the whole L3 volume (the slanted
// schedule), else C and the L3 checkpoints (the joint whole-volume one).
template <int V, bool FULL, int WIN, int PF, bool L3OUT>
__global__ __launch_bounds__(64) void vfwd2_kernel(const float *__restrict__ in0, float *__restrict__ out0,
                                                   PairArgs a0, const float *__restrict__ in1,
                                                   float *__restrict__ out1, PairArgs a1, Geom g) {
    const bool vb = __builtin_amdgcn_workgroup_id_y() != 0;
    vfwd_body<V, FULL, WIN, PF, false, L3OUT>(vb ? in1 : in0, vb ? out1 : out0, vb ? a1 : a0, g, bid_x(),
                                              tid_x());
}

template <int FD, int V, bool FULL, int PF>
__global__ __launch_bounds__(64) void pair_fwd_kernel(PairArgs a, Geom g) {
    pair_fwd_body<FD, V, FULL, PF>(a, g, bid_x());
}

template <int FAM, int V, bool FULL, int MODE>
__global__ __launch_bounds__(64) void pair_bwd_kernel(PairArgs a, Geom g) {
    pair_bwd_body<FAM, V, FULL, MODE>(a, g, bid_x());
}

// The final pass of a view: PAIR_V backward (L4, recomputing L3) summed with
// S12 and T, then WTA.  Three waves (pair_split_body): wave 0 recomputes L3
// segments from their checkpoints, wave 1 runs L4 and sums the totals into an
// LDS ring, wave 2 runs the batched WTA on the chunk before.
// D >= 64 run two WTA waves per column (each takes half of a chunk's pixels).
template <int V, bool FULL>
constexpr int final_nwta() { return FULL ? 2 : 1; }
// threads of a final kernel's workgroup: recompute, backward and WTA waves
template <int V, bool FULL>
constexpr int final_block() { return 64 * (2 + final_nwta<V, FULL>()); }

// BAND: one band of the banded backward phase (a.band).  NTC: C by
// non-temporal loads (a.nt_cost: two-view frames, whose views' cost volumes
// alternate in the Infinity Cache; profiles/r06_experiments/r06aa_final_nt.txt)
// NV = 2, both views' final passes in one launch (workgroup z = view): above
// the Infinity Cache nothing is gained by finishing a view before the other
// one starts, and one launch of 2W columns packs the workgroups into fewer
// rounds (HD256: 2 x 1920 columns at 1280 resident workgroups take 3 rounds
// instead of 2 + 2).
// NOT (4-path frames; pair_split_body's): X = (S12 + L3) + L4 goes into the
// LDS ring and the WTA waves consume X as the total: no acc_in loads.
template <int V, bool FULL, int NV, bool BAND, bool NTC, bool NOT>
__global__ __launch_bounds__(256) void pair_final_kernel(Views<PairArgs, NV> views, Geom g) {
    constexpr int K = pair_kv<V>();
    __shared__ __attribute__((aligned(16))) SplitFinalLds<K, V> lds;
    const PairArgs a = views.pick(VIEW_Z);
#ifdef SGM_NO_XCD_COLUMNS
    const int path = bid_x();
#else
    // row-major output maps (one-view frames): a line's columns on one XCD
    const int path = a.sub_cm ? bid_x() : xcd_column(bid_x(), g.W);
#endif
    pair_split_body<PAIR_V, V, FULL, PAIR_FINAL, K, 3, 2, final_nwta<V, FULL>(), BAND, NTC, NOT>(
        a, g, path, wave_id(), lds.s, &lds);
}

// Multi-role stage kernels of the frame schedule: block ranges run different
// (independent) roles, so a latency-bound horizontal role (H chains, few and
// long) overlaps the bandwidth-bound diagonal roles inside one launch.  The
// H blocks come first so they start at once.
//   stage A: L1 forward (ckpt)  |  L5 -> T5         |  L6 forward (ckpt)
//   stage B: L2 backward -> S12 |  L7 backward: T = (T5 + L6) + L7
// ROLES 1 (the forward bands, volumes above the Infinity Cache): the
// diagonal roles only, steps [kb, ke) of each chain (l5.band, d6.band); the
// H pair then runs as its own launch (hpair_kernel) after the last forward
// band -- its whole-row chains would set every band launch's length.
// NV = 2 (stage A, stage B, L8): frames whose two cost volumes fit the 256 MB
// Infinity Cache together (K64), where one view's launches leave most SIMDs
// with a single chain.
template <int V, bool FULL, int NV, int ROLES>
__global__ __launch_bounds__(64) void stage_a_kernel(Views<PairArgs, NV> h1, Views<SweepArgs, NV> l5,
                                                     Views<PairArgs, NV> d6, Geom g) {
    constexpr int PFH = pf_rows<V>(), PFD = pf_cols<V>();
    int b = bid_x();
    if constexpr (ROLES == 1) {
        if (b < g.W) sweep_body<4, V, SWEEP_INIT, FULL, PFD, true>(l5.pick(), g, b);
        else pair_fwd_body<5, V, FULL, PFD, true>(d6.pick(), g, b - g.W);
        return;
    }
    if (b < g.H) {
        // the H chains (few, long) are the launch's critical path
        __builtin_amdgcn_s_setprio(3);
        pair_fwd_body<0, V, FULL, PFH>(h1.pick(), g, b);
        return;
    }
    b -= g.H;
    if (b < g.W) {
        sweep_body<4, V, SWEEP_INIT, FULL, PFD>(l5.pick(), g, b);
        return;
    }
    pair_fwd_body<5, V, FULL, PFD>(d6.pick(), g, b - g.W);
}

// Stage B blocks are two waves: an H block splits its row's L2 pass into a
// recompute wave and a backward wave (pair_split_body); a D2 block runs two
// anti-diagonal L7 chains, one per wave.
// HROWS = false: a banded stage B (d7.band: the diagonal pair's steps
// [kb, ke)) without H rows -- the banded schedule's H pair ran them
// (hpair_kernel).
template <int V, bool FULL, bool HROWS>
__global__ __launch_bounds__(128) void stage_b_kernel(PairArgs h2, PairArgs d7, Geom g) {
    constexpr int K = pair_k<V>();
    __shared__ __attribute__((aligned(16))) SplitLds<K, V> lds;
    const int b = bid_x(), wave = wave_id();
    const int nh = HROWS ? g.H : 0;
    if (HROWS && b < nh) {
        pair_split_body<PAIR_H, V, FULL, PAIR_INIT2, K, 3>(h2, g, b, wave, lds, nullptr);
        return;
    }
    const int path = 2 * (b - nh) + wave;
    if (path < g.W) pair_bwd_body<PAIR_D2, V, FULL, PAIR_ACC, !HROWS>(d7, g, path);
}

// both views' stage B (workgroup y = view)
template <int V, bool FULL>
__global__ __launch_bounds__(128) void stage_b2_kernel(PairArgs h2a, PairArgs d7a, PairArgs h2b,
                                                       PairArgs d7b, Geom g) {
    constexpr int K = pair_k<V>();
    __shared__ __attribute__((aligned(16))) SplitLds<K, V> lds;
    const bool vb = __builtin_amdgcn_workgroup_id_y() != 0;
    const int b = bid_x(), wave = wave_id();
    if (b < g.H) {
        pair_split_body<PAIR_H, V, FULL, PAIR_INIT2, K, 3>(vb ? h2b : h2a, g, b, wave, lds, nullptr);
        return;
    }
    const int path = 2 * (b - g.H) + wave;
    if (path < g.W) pair_bwd_body<PAIR_D2, V, FULL, PAIR_ACC>(vb ? d7b : d7a, g, path);
}

// The H pair (L1 forward, then L2 backward recomputing L1 from the
// checkpoints it has just written -> S12) as its own launch: the forward
// bands' and the slanted schedule's, and the 4-path frames'.  With the
// diagonal roles in the band launches this launch holds only H (per view)
// single-wave chains, about one per SIMD at HD256, so it waits on memory
// latency; both views' rows side by side double the loads in flight.
// NTC = false (4-path frames): default loads, C stays resident for the final
// pass.
// One or two views (workgroup y = view; one view: passed twice).
template <int V, bool FULL, bool NTC>
__global__ __launch_bounds__(64) void hpair_kernel(PairArgs h1a, PairArgs h2a, PairArgs h1b,
                                                   PairArgs h2b, Geom g) {
#ifdef SGM_HPF
    constexpr int PFH = V >= 4 ? SGM_HPF : 2 * SGM_HPF;
#else
    constexpr int PFH = pf_rows<V>();
#endif
    const bool vb = __builtin_amdgcn_workgroup_id_y() != 0;
    const PairArgs h1 = vb ? h1b : h1a;
    const PairArgs h2 = vb ? h2b : h2a;
    // C is read by non-temporal loads (NTC): the H pair runs only above the
    // Infinity Cache, where its two reads of C pass through once each (the
    // top-down pass beside it -2.6%, HD256 frame -1.0%, 4K256 -0.6% paired,
    // profiles/r06_experiments/r06x_hpair_nt.txt)
    pair_fwd_body<0, V, FULL, PFH, false, NTC>(h1, g, bid_x());
    __threadfence();  // this wave's checkpoint stores, before it reads them back
    pair_bwd_body<PAIR_H, V, FULL, PAIR_INIT2, false, NTC>(h2, g, bid_x());
}

// ---------------------------------------------------------- 4-path frames
//
// paths = 4 (the reference's USE_8_PATH off, inc/SGM.h:7): S = ((L1+L2)+L3)+L4
// goes straight into the WTA (SGM.cpp:387-390), so a view needs the H pair and
// a final pass without the T stream (pair_final_kernel's NOT); no diagonal
// role shares their launches.
// C by default loads throughout: it stays in the Infinity Cache from the H
// pair to the final pass where it fits, and non-temporal loads gained nothing
// where it does not (profiles/paths4_alternatives.txt).

// The H pair as two launches (the stage A / stage B H roles on their own):
// L1 forward with checkpoints ...
template <int V, bool FULL, int NV>
__global__ __launch_bounds__(64) void h_fwd_kernel(Views<PairArgs, NV> h1, Geom g) {
    pair_fwd_body<0, V, FULL, pf_rows<V>()>(h1.pick(), g, bid_x());
}

// ... then L2 backward on two waves per row (recompute wave + backward wave,
// pair_split_body) -> S12
template <int V, bool FULL>
__global__ __launch_bounds__(128) void h_bwd2_kernel(PairArgs h2a, PairArgs h2b, Geom g) {
    constexpr int K = pair_k<V>();
    __shared__ __attribute__((aligned(16))) SplitLds<K, V> lds;
    const bool vb = __builtin_amdgcn_workgroup_id_y() != 0;
    pair_split_body<PAIR_H, V, FULL, PAIR_INIT2, K, 3>(vb ? h2b : h2a, g, bid_x(), wave_id(), lds,
                                                       nullptr);
}

// -------------------------------------------------------------- launch

// r[0 .. NV)'s arguments of one role
template <int NV, class A>
static Views<A, NV> views_of(const ViewRoles *r, A ViewRoles::*role) {
    Views<A, NV> v;
    for (int i = 0; i < NV; ++i) v.v[i] = r[i].*role;
    return v;
}

// f(NV) with the view count as a constant
template <class F>
static void for_views(int nviews, F &&f) {
    if (nviews == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}

template <int NV, int ROLES>
static void launch_stage_a_t(const ViewRoles *r, int nblk, Geom g, hipStream_t st) {
    const dim3 grid(nblk, NV);
    for_width(g.D, [&](auto V, auto FULL) {
        stage_a_kernel<V, FULL, NV, ROLES><<<grid, 64, 0, st>>>(
            views_of<NV>(r, &ViewRoles::h1), views_of<NV>(r, &ViewRoles::l5), views_of<NV>(r, &ViewRoles::d6), g);
    });
}

hipError_t launch_stage_a(const ViewRoles *r, int nviews, Geom g, hipStream_t st) {
    for_views(nviews, [&](auto NV) { launch_stage_a_t<NV, 0>(r, g.H + 2 * g.W, g, st); });
    return hipGetLastError();
}

hipError_t launch_stage_a_band(const ViewRoles *r, Geom g, hipStream_t st) {
    launch_stage_a_t<1, 1>(r, 2 * g.W, g, st);
    return hipGetLastError();
}

hipError_t launch_stage_b(const ViewRoles *r, int nviews, Geom g, hipStream_t st) {
    const bool hrows = nviews == 2 || r->d7.band.ke == 0;
    const dim3 grid((hrows ? g.H : 0) + (g.W + 1) / 2, nviews);
    for_width(g.D, [&](auto V, auto FULL) {
        if (nviews == 2) stage_b2_kernel<V, FULL><<<grid, 128, 0, st>>>(r[0].h2, r[0].d7, r[1].h2, r[1].d7, g);
        else if (hrows) stage_b_kernel<V, FULL, true><<<grid, 128, 0, st>>>(r->h2, r->d7, g);
        else stage_b_kernel<V, FULL, false><<<grid, 128, 0, st>>>(r->h2, r->d7, g);
    });
    return hipGetLastError();
}

hipError_t launch_hpair(const ViewRoles *r, int nviews, bool nt_cost, Geom g, hipStream_t st) {
    const dim3 grid(g.H, nviews);
    const ViewRoles &b = r[nviews - 1];
    for_width(g.D, [&](auto V, auto FULL) {
        if (nt_cost) hpair_kernel<V, FULL, true><<<grid, 64, 0, st>>>(r->h1, r->h2, b.h1, b.h2, g);
        else hpair_kernel<V, FULL, false><<<grid, 64, 0, st>>>(r->h1, r->h2, b.h1, b.h2, g);
    });
    return hipGetLastError();
}

hipError_t launch_h_fwd4(const ViewRoles *r, int nviews, Geom g, hipStream_t st) {
    const dim3 grid(g.H, nviews);
    for_width(g.D, [&](auto V, auto FULL) {
        for_views(nviews, [&](auto NV) {
            h_fwd_kernel<V, FULL, NV><<<grid, 64, 0, st>>>(views_of<NV>(r, &ViewRoles::h1), g);
        });
    });
    return hipGetLastError();
}

hipError_t launch_h_bwd4(const ViewRoles *r, int nviews, Geom g, hipStream_t st) {
    const dim3 grid(g.H, nviews);
    for_width(g.D, [&](auto V, auto FULL) {
        h_bwd2_kernel<V, FULL><<<grid, 128, 0, st>>>(r->h2, r[nviews - 1].h2, g);
    });
    return hipGetLastError();
}

template <int FD>
static void launch_fwd_t(const PairArgs &a, Geom g, hipStream_t st) {
    const dim3 grid(FD == 0 ? g.H : g.W);
    for_width(g.D, [&](auto V, auto FULL) {
        constexpr int PF = FD == 0 ? pf_rows<V>() : pf_cols<V>();
        pair_fwd_kernel<FD, V, FULL, PF><<<grid, 64, 0, st>>>(a, g);
    });
}

hipError_t launch_pair_fwd(int family, const PairArgs &a, Geom g, hipStream_t st) {
    // (the production schedule runs PAIR_V's forward pass fused into the
    // vertical cost filter, launch_vfwd; this one starts from a final volume)
    if (family == PAIR_H) launch_fwd_t<0>(a, g, st);
    else if (family == PAIR_V) launch_fwd_t<2>(a, g, st);
    else launch_fwd_t<5>(a, g, st);
    return hipGetLastError();
}

// the two-view vfwd's ring depth: the columns', but for the override of the
// slanted schedule's (L3OUT) four-value kernel
#ifndef VFWD2_PF4
#define VFWD2_PF4 8
#endif
template <int V, bool L3OUT>
constexpr int vfwd2_pf() { return V >= 4 && L3OUT ? VFWD2_PF4 : pf_cols<V>(); }

template <int WIN, int NV, bool BAND, bool L3OUT>
static void launch_vfwd_t(const float *const *in, float *const *out, const PairArgs *a, float *const *l3, Geom g,
                          hipStream_t st) {
    const dim3 grid(g.W, NV);
    PairArgs va[2] = {a[0], a[NV - 1]};
    if (L3OUT) va[0].out = l3[0], va[1].out = l3[NV - 1];
    for_width(g.D, [&](auto V, auto FULL) {
        if constexpr (NV == 2)
            vfwd2_kernel<V, FULL, WIN, vfwd2_pf<V, L3OUT>(), L3OUT><<<grid, 64, 0, st>>>(in[0], out[0], va[0], in[1],
                                                                                       out[1], va[1], g);
        else vfwd_kernel<V, FULL, WIN, pf_cols<V>(), BAND, L3OUT><<<grid, 64, 0, st>>>(in[0], out[0], va[0], g);
    });
}

hipError_t launch_vfwd(const float *const *in, float *const *out, const PairArgs *a, int nviews,
                       float *const *l3, Geom g, hipStream_t st) {
    auto launch = [&](auto WIN) {
        if (nviews == 2 && l3) launch_vfwd_t<WIN, 2, false, true>(in, out, a, l3, g, st);
        else if (nviews == 2) launch_vfwd_t<WIN, 2, false, false>(in, out, a, l3, g, st);
        else if (l3) launch_vfwd_t<WIN, 1, false, true>(in, out, a, l3, g, st);
        else if (a->band.ke > 0) launch_vfwd_t<WIN, 1, true, false>(in, out, a, l3, g, st);
        else launch_vfwd_t<WIN, 1, false, false>(in, out, a, l3, g, st);
    };
    if (g.scale == 1) launch(std::integral_constant<int, 3>{});
    else launch(std::integral_constant<int, 1>{});
    return hipGetLastError();
}

template <int FAM, int MODE>
static void launch_bwd_t(const PairArgs &a, Geom g, hipStream_t st) {
    const dim3 grid(FAM == PAIR_H ? g.H : g.W);
    for_width(g.D, [&](auto V, auto FULL) {
        pair_bwd_kernel<FAM, V, FULL, MODE><<<grid, 64, 0, st>>>(a, g);
    });
}

template <int NV, bool BAND = false, bool NTC = false, bool NOT = false>
static void launch_final_t(const ViewRoles *r, Geom g, hipStream_t st) {
    const dim3 grid(g.W, 1, NV);
    for_width(g.D, [&](auto V, auto FULL) {
        pair_final_kernel<V, FULL, NV, BAND, NTC, NOT><<<grid, final_block<V, FULL>(), 0, st>>>(
            views_of<NV>(r, &ViewRoles::fin), g);
    });
}

hipError_t launch_final(const ViewRoles *r, int nviews, bool paths4, Geom g, hipStream_t st) {
    // (bands and the NTC final are one view's: two views' launch reads neither fin.band nor fin.nt_cost)
    if (paths4 && nviews == 2) launch_final_t<2, false, false, true>(r, g, st);
    else if (paths4) launch_final_t<1, false, false, true>(r, g, st);
    else if (nviews == 2) launch_final_t<2>(r, g, st);
    else if (r->fin.band.ke > 0) launch_final_t<1, true>(r, g, st);
    else if (r->fin.nt_cost) launch_final_t<1, false, true>(r, g, st);
    else launch_final_t<1>(r, g, st);
    return hipGetLastError();
}

hipError_t launch_pair_bwd(int family, int mode, const PairArgs &a, Geom g, hipStream_t st) {
    // the production schedule uses H/INIT2, D2/ACC and V/FINAL
    if (family == PAIR_H && mode == PAIR_INIT2) launch_bwd_t<PAIR_H, PAIR_INIT2>(a, g, st);
    else if (family == PAIR_D2 && mode == PAIR_ACC) launch_bwd_t<PAIR_D2, PAIR_ACC>(a, g, st);
    else if (family == PAIR_V && mode == PAIR_FINAL) {
        ViewRoles r{};
        r.fin = a;
        return launch_final(&r, 1, false, g, st);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace sgm

#ifdef SGM_STAMPS
extern "C" int sgm_debug_stamps_pair(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sgm::sgm_stamps), sizeof(sgm::sgm_stamps)) != hipSuccess)
        return -1;
    if (reset) {
        unsigned long long z[16][3] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(sgm::sgm_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
