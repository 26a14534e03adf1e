// sgm_plan.h -- what sgm_create decides about a handle before it allocates
// anything: whether the parameters are served (valid_params) and which schedule
// every frame of the handle runs (plan_handle: enum Schedule and the choices
// behind it, DESIGN.md "Frame schedule").  The one place that holds the
// schedules' measured thresholds.  Every schedule gives bit-identical maps, so
// a slip here fails no parity test and only makes frames slower:
// tests/test_plan_cpu.py pins the choice by size.
// Plain C++ with no HIP in it (the CU count is an argument, the switches a
// struct), so that tests/cpp/plan_main.cpp can run it on the CPU under a
// sanitizer.
#pragma once

#include "../../include/sgm_hip.h"
#include "sgm_geom.h"

#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>

namespace sgm {

// sgm_default_params' values: the reference's constants.
inline void default_params(sgm_params *p, int h, int w, int s, int d) {
    p->height = h;
    p->width = w;
    p->scale = s;
    p->max_disp = d;
    p->p1 = 10;              // SGM.cpp:27
    p->p2 = 100;             // SGM.cpp:28
    p->uniqueness = 0.7f;    // inc/Solver.h:14
    p->lr_max_diff = 1.0f;   // inc/Solver.h:16
    p->blur = 1;             // Solver.cpp:124-125
    p->views = 2;            // SGM.cpp:448-818
    p->post_filter = 0;      // out = LR-checked map (SGM.cpp:818); 1: + post_filter (:821)
    p->lk_refine = 0;        // 1: + LKRefine (SGM.cpp:824, commented out in the reference)
    p->sky_detect = 0;       // 1: masks from SkyAreaDetector::detect on the GPU (node.cpp:80-93)
    p->solver = SGM_SOLVER_SGM;
    p->aux_only = 0;
    p->view = SGM_VIEW_LEFT;
    p->paths = 8;            // USE_8_PATH = true (inc/SGM.h:7)
}

// What sgm_create serves (false: the reason in why).
inline bool valid_params(const sgm_params *p, char *why, size_t n) {
    if (!p) { snprintf(why, n, "params is NULL"); return false; }
    // Solver.cpp:6-10 (d widened to 256), plus the filter windows' minimum size.
    if (p->height <= 0 || p->width <= 0 || p->scale <= 0 || p->max_disp <= 0) {
        snprintf(why, n, "h, w, s, d must be > 0 (Solver.cpp:6)");
        return false;
    }
    if (p->scale != 1 && p->scale != 2) { snprintf(why, n, "scale must be 1 or 2 (Solver.cpp:8)"); return false; }
    if (p->max_disp != 32 && p->max_disp != 64 && p->max_disp != 128 && p->max_disp != 256) {
        snprintf(why, n, "max_disp must be 32, 64, 128 or 256 (Solver.cpp:10, widened)");
        return false;
    }
    const int H = p->height / p->scale, W = p->width / p->scale;
    if (W < 5 || H < 3) { snprintf(why, n, "working size %dx%d below the 5x3 cost window", H, W); return false; }
    if (p->views != 1 && p->views != 2) { snprintf(why, n, "views must be 1 or 2"); return false; }
    if (p->paths != 0 && p->paths != 4 && p->paths != 8) {
        snprintf(why, n, "paths must be 8 (or 0) or 4 (USE_8_PATH, inc/SGM.h:7)");
        return false;
    }
    // SGM.cpp:374-408 keeps the previous pixel's sec_min_d when a pixel has no
    // second distinct cost; that stale index decides a pixel when
    // min/FLT_MAX > UNIQUE_RATIO.  A path cost is at most C + P2 (SGM.cpp:
    // 93-117: L = min(...) + C - minLp <= P2 + C), C at most 999999 (the sky
    // override, Solver.cpp:167-176), so min <= 8 (P2 + 999999); a ratio above
    // that / FLT_MAX can never see the stale index, which this build's WTA
    // does not keep.  Ratios at or below it (0 and negatives included) are
    // rejected.
    if (!(p->uniqueness > 0.0f) ||
        (double)p->uniqueness * FLT_MAX <= 8.0 * ((double)p->p2 + 999999.0)) {
        snprintf(why, n, "uniqueness must be > 8*(p2 + 999999)/FLT_MAX (SGM.cpp:392-408 would read "
                         "the previous pixel's sec_min_d)");
        return false;
    }
    if (p->view != SGM_VIEW_LEFT && p->view != SGM_VIEW_RIGHT) {
        snprintf(why, n, "view must be SGM_VIEW_LEFT or SGM_VIEW_RIGHT");
        return false;
    }
    if (p->view == SGM_VIEW_RIGHT &&
        (p->views != 1 || p->solver != SGM_SOLVER_SGM || p->post_filter || p->lk_refine)) {
        snprintf(why, n, "SGM_VIEW_RIGHT needs views == 1, the SGM solver and no post_filter/lk_refine");
        return false;
    }
    // the sky detector keeps a row of borders (W <= 8192) and the top half of a
    // 64-column strip (H/2 + 2 rows of 68 B <= ~159 KiB) in LDS (sgm_sky.hip)
    if (p->sky_detect && (W > 8192 || (size_t)(H / 2 + 2) * 68 > 160 * 1024 - 1024)) {
        snprintf(why, n, "sky_detect supports working grids up to 8192 x %d", 2 * ((160 * 1024 - 1024) / 68 - 2));
        return false;
    }
    if (p->solver != SGM_SOLVER_SGM && p->solver != SGM_SOLVER_BM) {
        snprintf(why, n, "solver must be SGM_SOLVER_SGM or SGM_SOLVER_BM");
        return false;
    }
    // the path DP's start handling relies on non-negative penalties (SGM.cpp:27-28 uses 10, 100)
    if (p->p1 < 0 || p->p2 < 0) { snprintf(why, n, "p1 and p2 must be >= 0"); return false; }
    if ((size_t)H * W > (size_t)0x7fffffff) { snprintf(why, n, "image too large"); return false; }
    return true;
}

// How run_frame aggregates (DESIGN.md "Frame schedule"): fixed at sgm_create by
// the handle's paths, views, volume size and the SGM_SLANT / SGM_BAND_ROWS
// switches (plan_handle).
enum Schedule {
    SCHED_PATHS4,        // the 4-path passes, both views per launch
    SCHED_SLANT,         // the slanted tiles
    SCHED_JOINT,         // two views whose volumes fit the Infinity Cache together: joint launches
    SCHED_BANDS,         // forward bands, the H pair, backward bands (volumes above the cache)
    SCHED_WHOLE_FINAL2,  // two views above the cache, unbanded: whole-volume passes, one final launch
    SCHED_PER_VIEW       // whole-volume passes, view after view
};

// The environment switches of the plan, as set when the handle is created
// (empty: unset).
struct PlanEnv {
    std::string slant;      // SGM_SLANT: 1/0 forces the slanted schedule on/off (the parity tests run it at every size)
    std::string vstrip;     // SGM_VSTRIP: 0 turns the slanted schedule's strip cost stage off
    std::string band_rows;  // SGM_BAND_ROWS: rows per band (0: whole-volume passes)
    std::string p4_hpair;   // SGM_P4_HPAIR: 1/0 forces the 4-path H pair's split form on/off
};

inline PlanEnv plan_env() {
    const auto get = [](const char *name) {
        const char *e = getenv(name);
        return std::string(e ? e : "");
    };
    return {get("SGM_SLANT"), get("SGM_VSTRIP"), get("SGM_BAND_ROWS"), get("SGM_P4_HPAIR")};
}

struct HandlePlan {
    Geom g;           // the working grid
    int nviews;
    bool paths4;      // params.paths == 4: the 4-path schedule (aggregate4; no bands, no slant)
    bool p4_split;    //   its H pair as forward + two-wave backward launches (SGM_P4_HPAIR)
    bool slant;       // the slanted-tile schedule (sgm_slant.hip, DESIGN.md "Slanted tiles")
    bool slant_forced;  // asked for by SGM_SLANT=1, not chosen by size: a shortage of memory for
                      //   its buffers fails sgm_create instead of falling back (plan_without_slant)
    bool vstrip;      //   its cost stage as checkpoints + strips (sgm_vstrip.hip; SGM_VSTRIP=0: off)
    int band_rows;    // rows per band of the backward phase (0: whole volume)
    Schedule sched;   // the aggregation's schedule (BM and aux_only handles never read it)
    int sub_cm;       // 1: the final passes store column-major sub-pixel maps (two views; the
                      // LR check reads them through LDS tiles); the slanted pass stores row-major
};

// The 256 MB Infinity Cache, against which every rule below holds a volume.
constexpr double kCacheBytes = 256.0 * 1024 * 1024;
inline double vol_bytes(Geom g) { return vol_elems(g) * sizeof(float); }

// The slanted-tile schedule replaces the bands (above the Infinity Cache)
// where it was measured faster (tools/slant_sizes.py,
// profiles/r04_experiments/slant.txt, with the H pair beside the top-down
// pass): at D = 256 once views * W >= 0.5 * NW * CUs, i.e. half a full-height
// tile of work per workgroup (round 6; 0.7 before), at D = 128 from 0.9
// (round 4 at 0.7: HD256 two views -18.6%, 4K256 one view -20%,
// two views -24%, 720p D = 256 two views -9.4%, HD128 two views -9.6%,
// 4K128 two views -18.8%; HD256 one view +2.0%, HD128 one view +24.9%,
// 1056x512 D = 128 two views +10.3%); never at D = 64 (HD64 two views
// +16.8%, 4K64 +4.2%; round 5: +11.4%, +2.2%).  Below that the tile-to-tile
// hand-off chain, not the bytes, sets the passes' time.  At D = 128 the
// threshold is 0.9 tiles per workgroup (below).
inline bool slant_default(Geom g, int nviews, int cus) {
    if (vol_bytes(g) <= kCacheBytes || g.D < 128) return false;
    // round 5 re-sweep with the prioritised receiver (profiles/r05_experiments/
    // r05m_slant_sizes.txt): 720p D = 256 two views (0.71 tiles per
    // workgroup) -6.2%, but 720p D = 128 two views (0.71) +7.7%: at D = 128
    // the crossover lies between 0.71 and HD128's 1.07 (-9.6%).  Round 6's
    // dataflow passes (profiles/r06_experiments/r06c_sizes_sweep.txt,
    // r06f_share_order_sweep.txt) moved D = 256 down: HD256 one view (0.54)
    // -5.0..-9.7%; at D = 128, 720p two views (0.71) stays +5.3%, HD128 one
    // view (0.54) +24%
    return 10LL * nviews * g.W >= (g.D >= 256 ? 5LL : 9LL) * kSlantNW * cus;
}

// Rows per band of the backward phase (stage B's diagonal pair, the L8
// sweep, the final pass) for cost volumes above the 256 MB Infinity Cache:
// about 192 MB of cost volume per band, so that a band's C and T stay in the
// cache from one pass to the next (tools/band_probe.hip: 1.27-1.35x for the
// three passes' streams alone; in the frame HD256 -3.5%, 4K256 -5%; 94-126 MB
// bands gain less).  A volume the cache already holds (K128) loses by it.
// Band edges sit on multiples of 16 rows from the bottom: whole segments of
// every pair family.
// SGM_BAND_ROWS overrides (0: whole-volume passes).
inline int band_rows_for(Geom g, const PlanEnv &env) {
    const double row_bytes = (double)g.W * g.D * sizeof(float);
    int rows;
    if (!env.band_rows.empty()) {
        rows = atoi(env.band_rows.c_str());
    } else {
#ifdef SGM_NO_BANDS
        return 0;
#endif
        if (vol_bytes(g) <= kCacheBytes) return 0;
        rows = (int)(192.0 * 1024 * 1024 / row_bytes);
    }
    rows -= rows % 16;
    return rows <= 0 || rows >= g.H ? 0 : rows;
}

// The aggregation schedule of every frame of a handle (sgm_frame.hip
// frame_maps), from the plan's other choices and the volume's size against the
// Infinity Cache.
inline Schedule schedule_for(const HandlePlan &p) {
    if (p.paths4) return SCHED_PATHS4;
    if (p.slant) return SCHED_SLANT;
    if (p.nviews == 2 && p.band_rows == 0 && 2.0 * vol_bytes(p.g) <= kCacheBytes) return SCHED_JOINT;
    if (p.band_rows > 0) return SCHED_BANDS;
    if (p.nviews == 2 && vol_bytes(p.g) > kCacheBytes) return SCHED_WHOLE_FINAL2;
    return SCHED_PER_VIEW;
}

// What follows from whether the handle runs the slanted schedule: the schedule
// itself and the sub-pixel maps' layout (two views: the final passes write
// column-major maps, whole cache lines, which lr_cm_kernel reads through LDS
// tiles; the slanted pass writes row-major ones).
inline HandlePlan plan_settled(HandlePlan p) {
    p.sched = schedule_for(p);
    p.sub_cm = p.nviews == 2 && !p.slant;
    return p;
}

// The plan of a handle of parameters valid_params accepts, on a device of
// `cus` compute units: the only place that decides any of its fields.
inline HandlePlan plan_handle(const sgm_params &p, int cus, const PlanEnv &env) {
    HandlePlan pl{};
    pl.g = {p.height / p.scale, p.width / p.scale, p.max_disp, p.scale};
    pl.nviews = p.views;
    // (BM and aux_only handles aggregate nothing: paths and SGM_SLANT are ignored)
    const bool aggregates = !p.aux_only && p.solver == SGM_SOLVER_SGM;
    pl.paths4 = p.paths == 4 && aggregates;
    if (pl.paths4) {
        // Its one choice by size, forced either way by SGM_P4_HPAIR
        // (DESIGN.md 5g): the H pair as one launch of one-wave rows (0),
        // or as a forward launch and a backward launch of two-wave rows (1).
        // With fewer rows in the launch than the device has SIMDs each SIMD
        // holds at most one chain and the pair's time is its chain latency,
        // which the two-wave rows cut (K128 one view 299 -> 235 us, two views
        // 376 -> 336, K64 two views 278 -> 189); with more rows the SIMDs are
        // filled either way and the single launch measured faster (HD256 two
        // views 2585 vs 2679 us; profiles/paths4_timing.txt)
        const char e = env.p4_hpair.empty() ? 0 : env.p4_hpair[0];
        pl.p4_split = e == '0' || e == '1' ? e == '1' : (long long)pl.nviews * pl.g.H < 4LL * cus;
    }
    // (a 4-path handle never runs bands, and SGM_SLANT is ignored on it: the
    // tiles are built around L5..L8)
    pl.band_rows = pl.paths4 ? 0 : band_rows_for(pl.g, env);
    const bool asked = !env.slant.empty() && env.slant[0] == '1';
    const bool want = env.slant.empty() ? slant_default(pl.g, pl.nviews, cus) : asked;
    pl.slant = aggregates && !pl.paths4 && want;
    pl.slant_forced = pl.slant && asked;
    pl.vstrip = !(!env.vstrip.empty() && env.vstrip[0] == '0');
    return plan_settled(pl);
}

// The plan again with the slanted schedule off, as SGM_SLANT=0 gives it: what
// sgm_create falls back to when the device cannot hold the schedule's buffers.
inline HandlePlan plan_without_slant(HandlePlan p) {
    p.slant = p.slant_forced = false;
    return plan_settled(p);
}

}  // namespace sgm
