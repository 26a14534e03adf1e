// sgm_cost_iir.h -- the reference's two cost filters, cost_horizontal_filter
// (Solver.cpp:296-330) and cost_vertical_filter (Solver.cpp:333-368), as the
// one statement of their arithmetic (DESIGN.md "Numerics").  Both are IIRs that
// filter in place: with h = WIN/2 and LAG = WIN-h-1, step t = 0 .. T-1
// (T = n - 2h) writes position LAG+t,
//
//   sum = x[0] + .. + x[WIN-1]                     (left to right, from 0)
//   x[LAG + t] = sum / WIN                         (correctly rounded)
//   sum += x[WIN + t];  sum -= x[t]                (two roundings; not the last step)
//
// where x[t] is what position t holds by then: the raw value below LAG, the
// step-(t-LAG) output after.  Positions below LAG and from LAG+T on stay raw.
// Every bit-exact map rests on this order of roundings, so the kernels do not
// restate it: they own the memory accesses, the prefetching and the raw border
// positions, and run the arithmetic and its history registers through these
// types (one exception, for a measured reason: cost_h_body, sgm_cost.hip).
// Plain C++ with no HIP in it (g++ compiles it for
// tests/cpp/cost_iir_main.cpp); build with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define SGM_IIR_FN __host__ __device__ __forceinline__
#define SGM_IIR_UNROLL _Pragma("unroll")
#else
#define SGM_IIR_FN inline
#define SGM_IIR_UNROLL
#endif

namespace sgm {

// Correctly rounded x / WIN for the cost filters' window sizes (Solver.cpp:319,
// 357: sum / win_size).  For WIN = 3 and 5, q0 = x*RN(1/WIN) corrected by one
// FMA residual step equals IEEE division bit-for-bit for EVERY non-negative
// finite float (exhaustive GPU check, tools/verify_div.hip; negative x follows
// by symmetry, and -0 cannot occur in the filters); 3 VALU ops instead of the
// ~10-op div_scale/div_fmas/div_fixup sequence.  For WIN = 7 and 9 (the window
// costs' divisors, sgm_window_cost.hip) the same form is proven over the inputs
// a window sum can reach, not over every float (sgm_window_cost_args.h).
template <int WIN>
SGM_IIR_FN float div_win(float x) {
    if constexpr (WIN == 1) {
        return x;
    } else if constexpr (WIN == 2) {
        return x * 0.5f;
    } else if constexpr (WIN == 4) {
        return x * 0.25f;
    } else {
        constexpr float r = 1.0f / WIN;
        const float q0 = x * r;
        const float e = __builtin_fmaf(-q0, (float)WIN, x);
        return __builtin_fmaf(e, r, q0);
    }
}

// ------------------------------------------------------ horizontal filter

// One chain's state before the step that produces position p: the running sum
// and the LAG values at positions p-LAG .. p-1 that the next steps subtract
// (hist[0] first: the raw value below LAG, the output after).
template <int WIN>
struct HFilter {
    static constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1;
    float sum;
    float hist[LAG > 0 ? LAG : 1];

    // the state before step 0, from the chain's first WIN (or more) raw values
    template <int N>
    SGM_IIR_FN void init(const float (&raw)[N]) {
        static_assert(N >= WIN, "the first WIN raw values");
        sum = 0.0f;
SGM_IIR_UNROLL
        for (int k = 0; k < WIN; ++k) sum += raw[k];
SGM_IIR_UNROLL
        for (int p = 0; p < LAG; ++p) hist[p] = raw[p];
    }
    // the value of the position this step produces
    SGM_IIR_FN float out() const { return div_win<WIN>(sum); }
    // every step but the last: out is out(), raw_next the raw value WIN/2 + 1
    // positions ahead of the one produced
    SGM_IIR_FN void advance(float out, float raw_next) {
        sum += raw_next;
        float a;
        if constexpr (LAG == 0) {
            a = out;
        } else {
            a = hist[0];
SGM_IIR_UNROLL
            for (int p = 0; p + 1 < LAG; ++p) hist[p] = hist[p + 1];
            hist[LAG - 1] = out;
        }
        sum -= a;
    }
    // advance() under conditions that are selects, not branches, for a walk
    // that crosses the filtered range's ends: filt, the position is a filtered
    // one (c = out() enters the history; else c is its raw value and nothing
    // moves); upd, it is filtered and not the last (the sum moves on)
    SGM_IIR_FN void advance_if(bool filt, bool upd, float c, float raw_next) {
        float ns = sum + raw_next;
        ns -= LAG == 0 ? c : hist[0];
        sum = upd ? ns : sum;
SGM_IIR_UNROLL
        for (int p = 0; p + 1 < LAG; ++p) hist[p] = filt ? hist[p + 1] : hist[p];
        if constexpr (LAG > 0) hist[LAG - 1] = filt ? c : hist[LAG - 1];
    }
};

// What a chain of the 5-wide filter needs to restart at output position p
// (2 <= p <= W-3): the running sum and the values at positions p-2 and p-1, in
// that order.  The strip schedule's checkpoint pass saves it at every strip
// edge, as v[k] at ((i * strips + s) * 3 + k) * D + d, and the strip pass
// restores it (sgm_vstrip.hip); p = W-3 is restored and never advanced.
struct HCheckpoint {
    float v[3];
    SGM_IIR_FN void save(const HFilter<5> &f) {
        v[0] = f.sum;
        v[1] = f.hist[0];
        v[2] = f.hist[1];
    }
    SGM_IIR_FN void restore(HFilter<5> &f) const {
        f.sum = v[0];
        f.hist[0] = v[1];
        f.hist[1] = v[2];
    }
};

// -------------------------------------------------------- vertical filter

// V chains side by side (a lane's V disparities of one column), WIN = 3 or 1:
// the running sums and the last position's value o1, which is what the next
// step subtracts at LAG = 1 (row 0's raw value before step 0).
template <int WIN, int V>
struct VFilter {
    static constexpr int HALF = WIN / 2, LAG = WIN - HALF - 1;
    static_assert(LAG <= 1, "one value of history");
    float sum[V], o1[V];

    // the state before step 0, from the column's first WIN rows
    SGM_IIR_FN void init(const float (&rows)[WIN][V]) {
SGM_IIR_UNROLL
        for (int v = 0; v < V; ++v) sum[v] = 0.0f;
SGM_IIR_UNROLL
        for (int k = 0; k < WIN; ++k)
SGM_IIR_UNROLL
            for (int v = 0; v < V; ++v) sum[v] += rows[k][v];
SGM_IIR_UNROLL
        for (int v = 0; v < V; ++v) o1[v] = rows[0][v];
    }
    SGM_IIR_FN void out(float (&c)[V]) const {
SGM_IIR_UNROLL
        for (int v = 0; v < V; ++v) c[v] = div_win<WIN>(sum[v]);
    }
    // every step but the last: c is out(), r the raw row WIN/2 + 1 below the
    // one produced
    SGM_IIR_FN void advance(const float (&c)[V], const float (&r)[V]) {
SGM_IIR_UNROLL
        for (int v = 0; v < V; ++v) {
            sum[v] = (sum[v] + r[v]) - (LAG == 0 ? c[v] : o1[v]);
            o1[v] = c[v];
        }
    }
    // The band carry: the state between two rows in two D-vectors, the sums in
    // vector 0 and o1 in vector 1.  ld(dst, k) / st(src, k) move this lane's V
    // floats of vector k.
    template <class LD>
    SGM_IIR_FN void load_carry(LD &&ld) {
        ld(sum, 0);
        ld(o1, 1);
    }
    template <class ST>
    SGM_IIR_FN void store_carry(ST &&st) const {
        st(sum, 0);
        st(o1, 1);
    }
};

}  // namespace sgm
