// sgm_frame.hip -- everything that enqueues a frame: the cost stage, the six
// aggregation schedules (DESIGN.md "Frame schedule"), the LR check, post_filter
// and LKRefine.  Which schedule a handle's frames run is decided once, at
// sgm_create, by plan_handle (sgm_plan.h); the frames read it from h->plan.
// Concurrency between independent roles comes from sharing a launch (stage
// A/B), not from streams (the runtime may map streams onto one hardware
// queue): a frame runs on one stream, at 73.5 B of HBM traffic per
// pixel-disparity in the per-view schedule (aggregate).
#include "sgm_handle.h"
#include "sgm_volume_args.h"

#include <stdlib.h>

using sgm::PairArgs;

// What view slot `slot`'s cost stage takes (sgm_internal.h) when it runs DSI
// `dsi` (0: left view, 1: right view) under the mask `sky` (null: none).  With
// cost_slots below, the one place that knows which table of a DSI's pair is
// the min_disp-shifted one (the other image's: d_cts, the tables themselves at
// min_disp = 0) and where the sky words of a masked strip frame sit: after the
// checkpoints in the dead Ch volume, 3/16 + 2/D of its floats at most.
sgm::CostSlot sgm::cost_slot(sgm_handle *h, int slot, int dsi, const uint8_t *sky) {
    sgm::CostSlot s{};
    s.ctl = dsi ? h->d_cts[0] : h->d_ct[0];
    s.ctr = dsi ? h->d_ct[1] : h->d_cts[1];
    s.dsi = dsi;
    s.sky = sky;
    s.ch = h->d_ch[slot];
    if (sky) s.skw = reinterpret_cast<uint64_t *>(h->d_ch[slot] + sgm::vstrip_sky_words_offset(h->g));
    s.c = cost_buf(h, slot);
    s.l3 = h->d_l3[slot];
    return s;
}

// The shifted tables the slots' DSIs read (DSI 0 the right image's, DSI 1 the
// left image's), after a census (or an upload) wrote d_ct; nothing at min_disp = 0
int sgm::shift_tables(sgm_handle *h, const sgm::CostSlot *s, int nviews, hipStream_t st) {
    if (h->min_disp == 0) return SGM_OK;
    bool left = false, right = false;
    for (int v = 0; v < nviews; ++v) (s[v].dsi ? left : right) = true;
    HIPCHK(h, timed(h, "ct_shift", (double)((left ? 1 : 0) + (right ? 1 : 0)) * h->g.H * h->g.W, st, [&] {
               return sgm::launch_ct_shift(h->d_ct[0], h->d_ct[1], left ? h->d_cts[0] : nullptr,
                                           right ? h->d_cts[1] : nullptr, h->min_disp / h->g.scale,
                                           h->g, st);
           }));
    return SGM_OK;
}

// One view's vertical cost filter fused with its L3 forward pass (sgm_handle.h)
int sgm::vfwd_view(sgm_handle *h, int view, const float *in, float *out, double elems, hipStream_t st,
                   sgm::Band band) {
    PairArgs pa = vfwd_args(h, view);
    pa.band = band;
    HIPCHK(h, timed(h, "vfwd", elems, st, [&] { return sgm::launch_vfwd(&in, &out, &pa, 1, nullptr, h->g, st); }));
    return SGM_OK;
}

// The device's CU count: plan_handle's argument (sgm_create) and the slanted
// top-down pass's share of the grid.
int sgm::slant_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}

namespace {

using sgm::CostSlot;
using sgm::ViewRoles;

// The one place that wires the roles (sgm_internal.h) to a view's buffers: C (cost_buf), S12
// (d_s), T (t_buf) and the checkpoints of each pair family.  disp, sub: where
// the final pass leaves its maps; sub_cm: sub and the confidence map beside it
// column-major.  A schedule that has no use for a role ignores it: the 4-path
// passes have no diagonal checkpoints and their final pass reads no acc_in
// (pair_split_body's NOT, sgm_bodies.h); the slanted passes take the pointers
// only.  nt_cost stays 0: only aggregate's one-view final launch sets it.
ViewRoles view_roles(sgm_handle *h, int view, uint16_t *disp, float *sub, int sub_cm) {
    float **ck = h->d_ck[view];
    float *T = t_buf(h, view);
    ViewRoles r{};
    PairArgs pa = pair_args(h);
    pa.cost = cost_buf(h, view);
    r.h1 = pa;
    r.h1.ckpt = ck[sgm::PAIR_H];
    r.h2 = r.h1;
    r.h2.out = h->d_s[view];
    r.d6 = pa;
    r.d6.ckpt = ck[sgm::PAIR_D2];
    r.d7 = r.d6;
    r.d7.acc_in = T;
    r.d7.out = T;
    r.l5 = sweep_args(h);
    r.l5.cost = pa.cost;
    r.l5.acc_out = T;
    r.l8 = r.l5;
    r.l8.acc_in = T;
    r.fin = pa;
    r.fin.ckpt = ck[sgm::PAIR_V];
    r.fin.s_in = h->d_s[view];
    r.fin.acc_in = T;
    r.fin.disp = disp;
    r.fin.sub = sub;
    r.fin.sub_cm = sub_cm;
    r.fin.ratio = h->d_ratio[view];  // (null: confidence off)
    h->ratio_cm[view] = sub_cm != 0;
    return r;
}

// The 8-path aggregation of nv views (r[0 .. nv)), given each one's final cost
// volume and L3 checkpoints (written by vfwd, or by stage_aggregate's PAIR_V
// forward pass), as four launches on one stream:
//   stage A: L1 fwd (ckpt) | L5 -> T5 | L6 fwd (ckpt)
//   stage B: L2 bwd: S12 = L1 + L2 | L7 bwd: T = (T5 + L6) + L7
//   L8:      T += L8
//   final:   L4 bwd recomputing L3: total = ((S12 + L3) + L4) + T -> WTA
// (the reference's order, SGM.cpp:386-390).  T may alias the dead
// horizontally filtered volume.
// nv = 2, each launch takes both views (workgroup y or z = view): for frames
// whose two cost volumes fit the 256 MB Infinity Cache together (K64: 2 x 119
// MB), where one view's launches hold too few chains to fill the chip (the
// reference runs the views back to back, SGM.cpp:32-801; the results are the
// same per view).
// final = false: the caller launches this view's final pass with the other
// view's.
int aggregate(sgm_handle *h, const ViewRoles *r, int nv, hipStream_t st, bool final) {
    const Geom g = h->g;
    const double elems = nv * vol_elems(g);
    HIPCHK(h, timed(h, "stage_a", elems, st, [&] { return sgm::launch_stage_a(r, nv, g, st); }));
    HIPCHK(h, timed(h, "stage_b", elems, st, [&] { return sgm::launch_stage_b(r, nv, g, st); }));
    HIPCHK(h, timed(h, "sweep_L8_acc", elems, st, [&] { return sgm::launch_l8(r, nv, g, st); }));
    if (!final) return SGM_OK;
    // one view of a two-view handle: its final pass is the last read of its
    // C, and the other view's volume follows it into the Infinity Cache, so C
    // goes by non-temporal loads (K128 two views -1.0% paired).  With one view
    // the next frame's stage A loses what the final pass gains, with one C
    // buffer or two used alternately (profiles/r06_experiments/
    // r06aa_final_nt.txt, r06bb_c_alternate.txt), so one-view frames keep
    // default loads
    ViewRoles one = r[0];
    one.fin.nt_cost = h->nviews == 2;
    const ViewRoles *f = nv == 1 ? &one : r;
    HIPCHK(h, timed(h, "pair_bwd_L4_final", elems, st, [&] { return sgm::launch_final(f, nv, false, g, st); }));
    return SGM_OK;
}

// Banded frames (cost volumes above the Infinity Cache): the view's vertical
// filter + L3 forward pass (vfwd, from the horizontally filtered volume T)
// and stage A's diagonal roles run in forward bands first, top band first, so
// that each band's final cost stays in the Infinity Cache from vfwd to L5 and
// L6; the whole H pair follows as its own launch (run_frame: both views' at
// once); then the backward bands (DESIGN.md "Bands").
int forward_bands(sgm_handle *h, int view, const ViewRoles &r, hipStream_t st) {
    const Geom g = h->g;
    const double elems = vol_elems(g);
    ViewRoles b = r;
    // band edges at H - m*BR (multiples of 16 rows from the bottom, as
    // the backward bands): whole segments of every family
    const int H = g.H, FR = h->plan.band_rows;
    const int nb = (H + FR - 1) / FR;
    for (int m = nb - 1; m >= 0; --m) {
        const int rb = H - (m + 1) * FR > 0 ? H - (m + 1) * FR : 0, re = H - m * FR;
        const double be = (double)(re - rb) / H * elems;
        if (int rc = sgm::vfwd_view(h, view, h->d_ch[view], cost_buf(h, view), be, st, {rb, re, h->d_carry[view][2]}))
            return rc;
        b.l5.band = {rb, re, h->d_carry[view][0]};
        b.d6.band = {rb, re, h->d_carry[view][1]};
        HIPCHK(h, timed(h, "stage_a_d", be, st, [&] { return sgm::launch_stage_a_band(&b, g, st); }));
    }
    return SGM_OK;
}

int backward_bands(sgm_handle *h, int view, const ViewRoles &r, hipStream_t st) {
    const Geom g = h->g;
    const double elems = vol_elems(g);
    ViewRoles b = r;
    const int H = g.H, BR = h->plan.band_rows;
    // bottom band first: the backward passes walk up
    for (int kb = 0; kb < H; kb += BR) {
        const int ke = kb + BR < H ? kb + BR : H;
        const double be = (double)(ke - kb) / H * elems;
        b.d7.band = {kb, ke, h->d_carry[view][0]};
        HIPCHK(h, timed(h, "stage_b_d2", be, st, [&] { return sgm::launch_stage_b(&b, 1, g, st); }));
        b.l8.band = {kb, ke, h->d_carry[view][1]};
        b.fin.band = {kb, ke, h->d_carry[view][2]};
        HIPCHK(h, timed(h, "sweep_L8_acc", be, st, [&] { return sgm::launch_l8(&b, 1, g, st); }));
        HIPCHK(h, timed(h, "pair_bwd_L4_final", be, st, [&] { return sgm::launch_final(&b, 1, false, g, st); }));
    }
    return SGM_OK;
}

// The 4-path aggregation (params.paths == 4: the reference's USE_8_PATH off,
// inc/SGM.h:7, SGM.cpp:387-390) of nv views, given each view's final cost
// volume and L3 checkpoints, as whole-volume passes at every size (DESIGN.md
// 5g):
//   H pair: L1 fwd (ckpt), L2 bwd: S12 = L1 + L2
//   final:  L4 bwd recomputing L3: total = (S12 + L3) + L4 -> WTA, sub-pixel
// each with both views in one launch (per-view vfwd and final launches
// measured +5.4% at K128, +7.5% at K64, +2.2% at HD256 on the frame).  No T
// chain, no diagonal checkpoints, no bands, no slanted tiles.
int aggregate4(sgm_handle *h, int nv, const ViewRoles *r, hipStream_t st) {
    const Geom g = h->g;
    const double elems = vol_elems(g);
    if (h->plan.p4_split) {
        HIPCHK(h, timed(h, "hpair4_fwd", nv * elems, st,
                        [&] { return sgm::launch_h_fwd4(r, nv, g, st); }));
        HIPCHK(h, timed(h, "hpair4_bwd", nv * elems, st,
                        [&] { return sgm::launch_h_bwd4(r, nv, g, st); }));
    } else {
        HIPCHK(h, timed(h, "hpair4", nv * elems, st,
                        [&] { return sgm::launch_hpair(r, nv, false, g, st); }));
    }
    HIPCHK(h, timed(h, "final4", nv * elems, st, [&] { return sgm::launch_final(r, nv, true, g, st); }));
    return SGM_OK;
}

// Whole-volume passes over nv views' final volumes and L3 checkpoints: the 4-path handle's, or
// the 8-path aggregation view after view
int aggregate_whole(sgm_handle *h, const ViewRoles *r, int nv, hipStream_t st) {
    if (h->plan.paths4) return aggregate4(h, nv, r, st);
    int rc = SGM_OK;
    for (int v = 0; v < nv && rc == SGM_OK; ++v) rc = aggregate(h, &r[v], 1, st, true);
    return rc;
}

// The frame's view slots: the left view in slot 0 and, with two views, the
// right view in slot 1; a right-view handle (SGM_VIEW_RIGHT) runs the right
// view, DSI 1 under the right mask, in slot 0.
void cost_slots(sgm_handle *h, const uint8_t *sky_l, const uint8_t *sky_r, CostSlot *s) {
    const bool right_only = h->p.view == SGM_VIEW_RIGHT;
    s[0] = sgm::cost_slot(h, 0, right_only ? 1 : 0, right_only ? sky_r : sky_l);
    if (h->nviews == 2) s[1] = sgm::cost_slot(h, 1, 1, sky_r);
}

// View slot `view`'s build_dsi_from_table[_beta] + horizontal IIR (cost_h),
// then the vertical IIR fused with the L3 forward pass (vfwd).
int cost_view(sgm_handle *h, const CostSlot *s, int view, int sky_pitch, hipStream_t st, bool vfwd = true) {
    const double elems = vol_elems(h->g);
    HIPCHK(h, timed(h, "cost_h", elems, st,
                    [&] { return sgm::launch_cost_h(&s[view], 1, sky_pitch, 1, h->g, st); }));
    return vfwd ? sgm::vfwd_view(h, view, s[view].ch, s[view].c, elems, st) : SGM_OK;
}

// BM::process (src/BM.cpp:9-97): census with BM's row decimation, the left
// DSI + both cost filters (the vertical filter's fused L3 checkpoints are
// simply not used), the filtered-cost WTA, then post_filter (:88).
int bm_frame(sgm_handle *h, FrameIO f, hipStream_t st) {
    const Geom g = h->g;
    const double npx = (double)g.H * g.W;
    if (h->p.sky_detect) {
        HIPCHK(h, timed(h, "sky_detect", npx, st, [&] {
                   return sgm::launch_sky_detect(&f.left, f.pitch, h->d_sky, g.W, h->d_sky_scratch, 1,
                                                 g, st);
               }));
        f.sky_l = h->d_sky[0];
        f.sky_pitch = g.W;
    }
    HIPCHK(h, timed(h, census_name(h), 2 * npx, st, [&] {
               return sgm::launch_census(f.left, f.pitch, g, h->win, h->p.blur, h->d_ct[0], st, true, f.right,
                                         h->d_ct[1]);
           }));
    const CostSlot s = sgm::cost_slot(h, 0, 0, f.sky_l);
    if (int rc = cost_view(h, &s, 0, f.sky_pitch, st)) return rc;
    HIPCHK(h, timed(h, "bm_wta", vol_elems(g), st, [&] {
               return sgm::launch_bm_wta(cost_buf(h, 0), h->p.uniqueness, h->d_disp[0], f.out,
                                         f.out_pitch, g, st);
           }));
    if (f.raw && f.raw != h->d_disp[0])  // (the host API passes d_disp[0] itself)
        HIPCHK(h, hipMemcpyAsync(f.raw, h->d_disp[0], (size_t)g.H * g.W * sizeof(uint16_t),
                                 hipMemcpyDeviceToDevice, st));
    if (h->p.post_filter)
        if (int rc = sgm::post_filter(h, f.out, f.out_pitch, st)) return rc;
    // (sgm_set_fill: the hole filling after BM's own post_filter call)
    return h->fill_mode ? sgm::fill_frame(h, f.out, f.out_pitch, st) : SGM_OK;
}

// The slanted-tile schedule of the aggregation (DESIGN.md "Slanted tiles"),
// after the cost stage left each view's horizontally filtered volume in d_ch:
//   vfwd_l3 (per view): vertical IIR -> C, and the full L3 volume
//   slant_down (both views): T56 = L5 + L6 (SGM.cpp:389's first association)
//     into the dead horizontally filtered volume
//   H pair (both views): S12 = L1 + L2
//   slant_up (both views): L4, L7, L8 walking up, total
//     ((S12 + L3) + L4) + ((T56 + L7) + L8), WTA, sub-pixel (row-major maps)
// the top-down pass's share of the CUs (eighths) while the H pair runs
// beside it.  Round 6 (dataflow passes, profiles/r06_experiments/
// r06f_share_order_sweep.txt, best of 3): the top-down pass alone now takes
// 1.9 ms at HD256 (it took the whole 4.7 ms region before), so the share
// that balances the two moved: 4/8 for D = 256 frames below 2e9 elements
// (HD256 V=2 10.83 ms vs 11.12 at 8/8, HD256 V=1, 720p256 V=2), the whole
// chip otherwise (4K256 V=1/V=2, HD128 and 4K128 V=2 within 0.5% of their
// best at 8/8).  Launching the H pair first was no better at any share.
int slant_down_grid_eighths(Geom g, int nviews) {
#ifdef SGM_SLANT_DEBUG
    if (const char *e = getenv("SGM_SLANT_DOWN_EIGHTHS"))  // share sweeps (tools/slant_share.sh)
        if (atoi(e) >= 1 && atoi(e) <= 8) return atoi(e);
#endif
    const double elems = (double)nviews * g.H * g.W * g.D;
    return g.D >= 256 && elems < 2e9 ? 4 : 8;
}

// have_c: the strip pass already wrote C and the L3 volumes (cost_stage)
int slant_views(sgm_handle *h, const ViewRoles *r, hipStream_t st, bool have_c) {
    const Geom g = h->g;
    const int nv = h->nviews;
    const double elems = vol_elems(g);
    sgm::SlantArgs sa{};
    if (!have_c) {  // the views in one launch
        const PairArgs pa[2] = {pair_args(h), pair_args(h)};
        HIPCHK(h, timed(h, "vfwd_l3", nv * elems, st,
                        [&] { return sgm::launch_vfwd(h->d_ch, h->d_c, pa, nv, h->d_l3, g, st); }));
    }
    for (int v = 0; v < nv; ++v) {
        const PairArgs &fin = r[v].fin;
        sa.v[v] = {fin.cost, fin.s_in, h->d_l3[v], fin.acc_in, r[v].d7.out,
                   fin.sub, fin.disp, h->d_gran, fin.ratio};
    }
    sa.ctl = h->d_slant_ctl;
    sa.zero = h->d_zero;
    sa.dummy = h->d_slant_dummy;
    sa.p1 = (float)h->p.p1;
    sa.p2 = (float)h->p.p2;
    sa.uniq = h->p.uniqueness;
    sa.min_disp = h->min_disp;
    sa.nviews = nv;
    sa.err_host = h->d_slant_err;
#ifdef SGM_SLANT_DEBUG
    if (getenv("SGM_SLANT_T56SWEEP")) {  // T56 by the two diagonal sweeps instead
        for (int v = 0; v < nv; ++v) {
            // (L6 accumulates into T5 as the L8 role does: acc_in = acc_out = T)
            HIPCHK(h, sgm::launch_sweep(SGM_DIR_L5, sgm::SWEEP_INIT, r[v].l5, g, st));
            HIPCHK(h, sgm::launch_sweep(SGM_DIR_L6, sgm::SWEEP_ACC, r[v].l8, g, st));
        }
    } else
#endif
    // The H pair and the top-down pass both only read C: the H pair runs on
    // its own stream beside the top-down pass, which keeps half of the CUs
    // (its workgroups are persistent and claim tiles in order, so any grid
    // is correct).  Each is bound by latency as much as by bytes (long H
    // chains; the tile-to-tile hand-off chain), so together they fill the
    // memory system better than one after the other: HD256 13.44 -> 12.72,
    // 4K256 48.03 -> 46.31 ms per frame (profiles/r04_experiments/slant.txt).
    // (profiled as one more entry, "slant_down_hpair": fork to join on the
    // frame's stream, the pair's wall time; the two launches' own entries
    // overlap in time)
    sa.max_grid = slant_down_grid_eighths(g, nv) * sgm::slant_cus() / 8;
#ifdef SGM_SLANT_DEBUG
    // timing probes (wrong maps): SGM_SLANT_SOLO=down|hpair runs that launch
    // alone on all CUs; =seq runs both, one after the other
    if (const char *solo = getenv("SGM_SLANT_SOLO")) {
        sa.max_grid = 0;
        if (strcmp(solo, "hpair") != 0)
            HIPCHK(h, timed(h, "slant_down", nv * elems, st, [&] { return sgm::launch_slant_down(sa, g, st); }));
        if (strcmp(solo, "down") != 0)
            HIPCHK(h, timed(h, "stage_a_h", nv * elems, st,
                            [&] { return sgm::launch_hpair(r, nv, true, g, st); }));
        HIPCHK(h, timed(h, "slant_up", nv * elems, st, [&] { return sgm::launch_slant_up(sa, g, st); }));
        return SGM_OK;
    }
#endif
    HIPCHK(h, timed(h, "slant_down_hpair", nv * elems, st, [&] {
        hipError_t e = hipEventRecord(h->ev_fork, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->st_h, h->ev_fork, 0);
        if (e == hipSuccess)
            e = timed(h, "slant_down", nv * elems, st, [&] { return sgm::launch_slant_down(sa, g, st); });
        if (e == hipSuccess)
            e = timed(h, "stage_a_h", nv * elems, h->st_h,
                      [&] { return sgm::launch_hpair(r, nv, true, g, h->st_h); });
        if (e == hipSuccess) e = hipEventRecord(h->ev_join, h->st_h);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, h->ev_join, 0);
        return e;
    }));
    sa.max_grid = 0;
    HIPCHK(h, timed(h, "slant_up", nv * elems, st, [&] { return sgm::launch_slant_up(sa, g, st); }));
    return SGM_OK;
}

// The cost stage of an SGM frame: the sky masks (sky_detect handles), the
// census of both images, then each view's DSI and its two cost filters, as far
// as the schedule's aggregation expects them: C and the L3 checkpoints
// (whole-volume schedules), the horizontally filtered volumes (bands and the
// slanted tiles run their own vertical pass), or C and the L3 volumes
// (*have_c: the slanted schedule's strip pass).
int cost_stage(sgm_handle *h, FrameIO f, hipStream_t st, bool *have_c) {
    const Geom g = h->g;
    int rc;
    const uint8_t *d_sky_l = f.sky_l, *d_sky_r = f.sky_r;
    int sky_pitch = f.sky_pitch;
    const double npx = (double)g.H * g.W;
    if (h->p.sky_detect) {  // node.cpp:80-93: detect on both inputs, then process with the masks
        // (a right-view handle detects on the right image alone, into d_sky[0])
        const bool right_only = h->p.view == SGM_VIEW_RIGHT;
        const uint8_t *imgs[2] = {right_only ? f.right : f.left, f.right};
        HIPCHK(h, timed(h, "sky_detect", npx, st, [&] {
                   return sgm::launch_sky_detect(imgs, f.pitch, h->d_sky, g.W, h->d_sky_scratch,
                                                 h->nviews, g, st);
               }));
        d_sky_l = h->d_sky[0];
        d_sky_r = right_only ? h->d_sky[0] : h->nviews == 2 ? h->d_sky[1] : nullptr;
        sky_pitch = g.W;
    }
    HIPCHK(h, timed(h, census_name(h), 2 * npx, st, [&] {  // both images, one launch
               return sgm::launch_census(f.left, f.pitch, g, h->win, h->p.blur, h->d_ct[0], st, false,
                                         f.right, h->d_ct[1]);
           }));
    CostSlot s[2] = {};
    cost_slots(h, d_sky_l, d_sky_r, s);
    const int nv = h->nviews;
    if ((rc = sgm::shift_tables(h, s, nv, st)) != SGM_OK) return rc;
    const double elems = nv * vol_elems(g);
    // two views: both DSIs + horizontal IIRs in one launch (a view's H*D
    // serial chains alone leave most SIMDs idle at KITTI sizes)
    const bool joint = nv == 2 && sgm::cost_h_staged(s, 2, g);
    // banded frames run vfwd in forward bands (forward_bands); the slanted
    // schedule runs its own vertical pass
    const bool vfwd_here = h->plan.sched != sgm::SCHED_BANDS && h->plan.sched != sgm::SCHED_SLANT;
    // the slanted schedule's cost stage as checkpoints + strips (sgm_vstrip.hip):
    // C and the L3 volumes in one pass, 9 B per element instead of cost_h's
    // 4 and vfwd_l3's 12
    const bool vstrip = h->plan.slant && h->plan.vstrip && sgm::vstrip_supported(s, nv, g);
    if (vstrip) {
        HIPCHK(h, timed(h, "cost_ck", elems, st, [&] { return sgm::launch_cost_ck(s, nv, sky_pitch, g, st); }));
        // (a masked frame's sky flags go to the strip pass as words)
        for (int v = 0; v < nv; ++v)
            if (s[v].sky)
                HIPCHK(h, timed(h, "sky_words", npx, st,
                                [&] { return sgm::launch_sky_words(s[v].sky, sky_pitch, g, s[v].skw, st); }));
        HIPCHK(h, timed(h, "vstrip", elems, st, [&] {
                   return sgm::launch_vstrip(s, nv, h->d_slant_dummy, (float)h->p.p1, (float)h->p.p2, g, st);
               }));
    } else if (joint) {
        HIPCHK(h, timed(h, "cost_h", elems, st, [&] { return sgm::launch_cost_h(s, 2, sky_pitch, 1, g, st); }));
        if (vfwd_here) {
            // both views' vertical passes in one launch: W chains per view
            // leave the CUs under-filled at KITTI (K64 2 x 69.7 -> 90.7 us,
            // frame -3.9%; K128 two views 177 -> 166 us)
            // (view 1's columns first, view 0's last, as the per-view passes
            // ran: stage A then finds more of view 0 in the cache, K64 stage
            // A -3 us, profiles/r05_experiments/r05s_ab_vfwd2.txt)
            const PairArgs pa[2] = {vfwd_args(h, 1), vfwd_args(h, 0)};
            const float *in[2] = {s[1].ch, s[0].ch};
            float *out[2] = {s[1].c, s[0].c};
            HIPCHK(h, timed(h, "vfwd", elems, st, [&] { return sgm::launch_vfwd(in, out, pa, 2, nullptr, g, st); }));
        }
    } else {
        for (int v = nv - 1; v >= 0; --v)  // (slot 1 first)
            if ((rc = cost_view(h, s, v, sky_pitch, st, vfwd_here)) != SGM_OK) return rc;
    }
    *have_c = vstrip;
    return SGM_OK;
}

// post_filter and LKRefine at the end of a frame (SGM.cpp:821-824); on a handle with fill set
// (sgm_set_fill) the hole filling after them, the frame's last map stage
int finish_frame(sgm_handle *h, const FrameIO &f, hipStream_t st) {
    int rc;
    // with LKRefine next, the post filter's last kernel writes LKRefine's
    // input copy instead of the map (no device copy in between)
    const bool pf_to_lk = h->p.post_filter && h->p.lk_refine;
    if (h->p.post_filter && (rc = sgm::post_filter(h, f.out, f.out_pitch, st, pf_to_lk)))  // SGM.cpp:821
        return rc;
    if (h->p.lk_refine &&  // SGM.cpp:824
        (rc = sgm::lk_refine(h, f.left, f.right, f.pitch, f.out, f.out_pitch, st, pf_to_lk)))
        return rc;
    return h->fill_mode ? sgm::fill_frame(h, f.out, f.out_pitch, st) : SGM_OK;
}

// The views' roles for a frame's maps.  Returns direct_out: one view with a dense output map, whose
// final pass writes the sub-pixel map straight into it (no device copy after the frame); else
// the handle's sub-pixel layout for the LR check.  The raw WTA map, when asked for, is written
// straight into f.raw by the left view's final pass; the right view's is never written.
bool frame_roles(sgm_handle *h, const FrameIO &f, ViewRoles *r) {
    const bool direct_out = h->nviews == 1 && f.out_pitch == h->g.W;
    r[0] = view_roles(h, 0, f.raw, direct_out ? f.out : h->d_sub[0], h->plan.sub_cm);
    if (h->nviews == 2) r[1] = view_roles(h, 1, nullptr, h->d_sub[1], h->plan.sub_cm);
    return direct_out;
}

// The frame from the views' sub-pixel maps on: the LR check, or the one view's map copied where
// the final pass could not write it, then post_filter and LKRefine.
int views_to_out(sgm_handle *h, const FrameIO &f, bool direct_out, hipStream_t st) {
    const Geom g = h->g;
    if (h->nviews == 2) {
        HIPCHK(h, timed(h, "lr", (double)g.H * g.W, st, [&] {
                   // (true-disparity maps: the invalid marker is D + min_disp + 1)
                   return h->plan.sub_cm ? sgm::launch_lr_cm(h->d_sub[0], h->d_sub[1], f.out, f.out_pitch,
                                                        h->p.lr_max_diff, h->gt, st)
                                    : sgm::launch_lr(h->d_sub[0], g.W, h->d_sub[1], g.W, f.out,
                                                     f.out_pitch, h->p.lr_max_diff, h->gt, st);
               }));
    } else if (!direct_out) {
        HIPCHK(h, hipMemcpy2DAsync(f.out, (size_t)f.out_pitch * sizeof(float), h->d_sub[0],
                                   (size_t)g.W * sizeof(float), (size_t)g.W * sizeof(float), g.H,
                                   hipMemcpyDeviceToDevice, st));
    }
    return finish_frame(h, f, st);
}

// The frame's input slot (DESIGN.md "The input slot"): at most one launch, by
// the handle's input stage (sgm_input_stage.h), writes both full-size grey
// images into d_rs (every handle's census reads both), and the sky detector,
// the census, LKRefine and BM read those instead of the caller's images.  An
// input size: node.cpp:75-76's resize (5j); maps: the remap, which resizes too
// (5k); a colour format converts inside either, or with neither as a launch of
// its own (5l).
int input_slot(sgm_handle *h, FrameIO *f, hipStream_t st) {
    const sgm::InputStage &in = h->in;
    const sgm::InputKind kind = in.kind();
    if (kind == sgm::INPUT_NONE) return SGM_OK;
    static const char *const names[] = {nullptr, "resize", "rectify", "gray"};
    const uint8_t *src[2] = {f->left, f->right};
    const int H = h->p.height, W = h->p.width, pitch = f->pitch;
    HIPCHK(h, timed(h, names[kind], 2.0 * H * W, st, [&] {
               switch (kind) {
               case sgm::INPUT_RESIZE:
                   return sgm::launch_resize(src, in.in_rows, in.in_cols, pitch, h->d_rs, H, W, W, 2, st, in.fmt);
               case sgm::INPUT_RECTIFY:
                   return sgm::launch_rectify(src, in.rc_rows, in.rc_cols, pitch, h->d_map, h->d_rs, H, W, W, 2,
                                              st, in.fmt);
               default:
                   return sgm::launch_gray(in.fmt, src, H, W, pitch, h->d_rs, W, 2, st);
               }
           }));
    f->left = h->d_rs[0];
    f->right = h->d_rs[1];
    f->pitch = W;
    h->rs_valid = true;
    return SGM_OK;
}

// Where a volume frame's producers (aggregate_volume's import, window_cost_stage) leave view v's raw
// volume: its C, which the horizontal filter reads and the unfiltered passes aggregate; with the
// vertical filter alone its Ch, vfwd's input.
float *volume_raw_buf(sgm_handle *h, int v) {
    return h->vol_filter == SGM_FILTER_V ? h->d_ch[v] : cost_buf(h, v);
}

// The frame from the cost volume on, given every view's raw volume in volume_raw_buf
// (aggregate_volume's import, or window_cost_stage): frame_maps' wiring
// (frame_roles); stage_aggregate's passes -- the L3 checkpoints from the final
// volume, then aggregate_whole, whatever schedule the handle's frames run --,
// and frame_maps' tail (views_to_out).
int volume_frame(sgm_handle *h, const FrameIO &f, hipStream_t st) {
    const Geom g = h->g;
    const int nv = h->nviews;
    const double elems = vol_elems(g);
    ViewRoles r[2] = {};
    const bool direct_out = frame_roles(h, f, r);
    int rc = SGM_OK;
    // the handle's cost filters (sgm_set_volume_filter), each view's volume on its
    // own as SGM::process filters each DSI it built: the horizontal one over both views in one
    // launch -- in place in C, or with the vertical one to follow into Ch, which vfwd reads --,
    // the vertical one as the census frames run it, fused with the L3 forward pass (vfwd in the
    // place of pair_fwd_L3; alone it finds the raw volumes in Ch: volume_raw_buf)
    const int fl = h->vol_filter;
    if (fl & SGM_FILTER_H) {
        const bool to_ch = (fl & SGM_FILTER_V) != 0;
        const float *in[2] = {cost_buf(h, 0), nv == 2 ? cost_buf(h, 1) : nullptr};
        float *out[2] = {to_ch ? h->d_ch[0] : cost_buf(h, 0), nv == 2 ? (to_ch ? h->d_ch[1] : cost_buf(h, 1)) : nullptr};
        HIPCHK(h, timed(h, "vol_hfilter", nv * elems, st,
                        [&] { return sgm::launch_volume_hfilter(in, out, nv, to_ch, g, st); }));
    }
    for (int v = 0; v < nv; ++v) {
        if (fl & SGM_FILTER_V) {
            if ((rc = sgm::vfwd_view(h, v, h->d_ch[v], cost_buf(h, v), elems, st)) != SGM_OK) return rc;
        } else {
            HIPCHK(h, timed(h, "pair_fwd_L3", elems, st,
                            [&] { return sgm::launch_pair_fwd(sgm::PAIR_V, r[v].fin, g, st); }));
        }
    }
    if ((rc = aggregate_whole(h, r, nv, st)) != SGM_OK) return rc;
    return views_to_out(h, f, direct_out, st);
}

// The cost stage of a frame on a SAD, SSD or CT handle (sgm_set_cost, DESIGN.md
// 5o, 5s): one launch writes the left view's window cost volume into its C; with
// two views the import kernel's right-view role derives the right view's from
// it (the handle's own left buffer as a dense fp32 HWD source), from the raw
// volume: the handle's cost filters (sgm_set_volume_filter) run after it, in
// volume_frame.  No census, no masks.
int window_cost_stage(sgm_handle *h, const FrameIO &f, hipStream_t st) {
    const Geom g = h->g;
    HIPCHK(h, timed(h, window_cost_name(h, h->cost_kind), vol_elems(g), st, [&] {
               return sgm::launch_window_cost(h->cost_kind, f.left, f.right, f.pitch, volume_raw_buf(h, 0),
                                              h->min_disp, g, h->win, h->weights, st);
           }));
    if (h->nviews == 2)
        HIPCHK(h, timed(h, "vol_import", vol_elems(g), st, [&] {
                   return sgm::launch_volume_import(volume_raw_buf(h, 0), sgm::kVolF32, (long long)g.W * g.D, g.D, 1,
                                                    nullptr, volume_raw_buf(h, 1), h->min_disp, g, st);
               }));
    return SGM_OK;
}

// The frame up to its last map stage: the input slot, the solver, the LR check, post_filter and
// LKRefine (run_frame, below, follows it with the output slot).
int frame_maps(sgm_handle *h, FrameIO f, hipStream_t st) {
    const Geom g = h->g;
    const int nv = h->nviews;
    const double elems = vol_elems(g);
    int rc;
    if ((rc = input_slot(h, &f, st)) != SGM_OK) return rc;
    // Everything runs on one stream.  Two-view frames keep each view's cost
    // volume resident in the 256 MB Infinity Cache through its readers by
    // running the views' aggregation back to back (K128: 238.5 MB per view;
    // concurrent views measured 1.627 vs 1.589 ms per pair), unless both
    // volumes fit together (K64: joint launches) or neither fits (HD/4K:
    // bands, or the slanted schedule).
    if (h->p.solver == SGM_SOLVER_BM) return bm_frame(h, f, st);
    if (h->cost_kind != SGM_COST_CENSUS) {  // a window cost instead of the census cost stage
        if ((rc = window_cost_stage(h, f, st)) != SGM_OK) return rc;
        return volume_frame(h, f, st);
    }
    bool have_c = false;
    if ((rc = cost_stage(h, f, st, &have_c)) != SGM_OK) return rc;
    ViewRoles r[2] = {};
    const bool direct_out = frame_roles(h, f, r);
    switch (h->plan.sched) {
    case sgm::SCHED_PATHS4: rc = aggregate4(h, nv, r, st); break;
    case sgm::SCHED_SLANT: rc = slant_views(h, r, st, have_c); break;
    case sgm::SCHED_JOINT: rc = aggregate(h, r, 2, st, true); break;
    case sgm::SCHED_BANDS: {
        // the views' forward bands, then their H pairs in one launch, then
        // each view's backward bands
        for (int v = 0; v < nv; ++v)
            if ((rc = forward_bands(h, v, r[v], st)) != SGM_OK) return rc;
        HIPCHK(h, timed(h, "stage_a_h", nv * elems, st, [&] { return sgm::launch_hpair(r, nv, true, g, st); }));
        for (int v = 0; v < nv; ++v)
            if ((rc = backward_bands(h, v, r[v], st)) != SGM_OK) return rc;
        break;
    }
    case sgm::SCHED_WHOLE_FINAL2:
        // whole-volume passes above the Infinity Cache (SGM_BAND_ROWS=0):
        // nothing is gained by finishing the left view first, so both
        // views' final passes run as one launch (fewer workgroup rounds)
        for (int v = 0; v < 2; ++v)
            if ((rc = aggregate(h, &r[v], 1, st, false)) != SGM_OK) return rc;
        HIPCHK(h, timed(h, "pair_bwd_L4_final", 2.0 * elems, st,
                        [&] { return sgm::launch_final(r, 2, false, g, st); }));
        break;
    case sgm::SCHED_PER_VIEW: rc = aggregate_whole(h, r, nv, st); break;
    }
    if (rc != SGM_OK) return rc;
    return views_to_out(h, f, direct_out, st);
}

}  // namespace

int sgm::stage_aggregate(sgm_handle *h, hipStream_t st) {
    const ViewRoles r = view_roles(h, 0, h->d_disp[0], h->d_sub[0], 0);
    // the L3 checkpoints from the final volume (frames get them from vfwd)
    HIPCHK(h, timed(h, "pair_fwd_L3", vol_elems(h->g), st,
                    [&] { return sgm::launch_pair_fwd(sgm::PAIR_V, r.fin, h->g, st); }));
    return aggregate_whole(h, &r, 1, st);
}

int sgm::filter_volume(sgm_handle *h, float *d_cost, int filters, hipStream_t st) {
    const Geom g = h->g;
    const double elems = vol_elems(g);
    const float *in = d_cost;
    if (filters & SGM_FILTER_H) {
        // alone in place; with the vertical filter to follow into view 0's Ch, as in the frames
        float *out = filters & SGM_FILTER_V ? h->d_ch[0] : d_cost;
        HIPCHK(h, timed(h, "vol_hfilter", elems, st,
                        [&] { return sgm::launch_volume_hfilter(&in, &out, 1, out != d_cost, g, st); }));
        in = out;
    } else if (filters & SGM_FILTER_V) {  // (vfwd's volumes are __restrict__: it reads a copy)
        HIPCHK(h, timed(h, "vol_copy", elems, st, [&] { return sgm::launch_copy(d_cost, h->d_ch[0], g, st); }));
        in = h->d_ch[0];
    }
    // (vfwd's L3 checkpoints land in view 0's, which every frame rewrites)
    return filters & SGM_FILTER_V ? sgm::vfwd_view(h, 0, in, d_cost, elems, st) : SGM_OK;
}

int sgm::aggregate_volume(sgm_handle *h, const sgm_volume &vol, float *d_out, int out_pitch, uint16_t *d_raw,
                          hipStream_t st) {
    const int nv = h->nviews;
    // one launch reads the caller's volume and writes every view's raw volume
    HIPCHK(h, timed(h, "vol_import", nv * vol_elems(h->g), st, [&] {
               return sgm::launch_volume_import(vol.d_cost, vol.dtype, vol.stride_row, vol.stride_col,
                                                vol.stride_disp, volume_raw_buf(h, 0),
                                                nv == 2 ? volume_raw_buf(h, 1) : nullptr, h->min_disp, h->g, st);
           }));
    // (no images: sgm_aggregate_device refuses handles with lk_refine)
    if (int rc = volume_frame(h, {nullptr, nullptr, 0, nullptr, nullptr, 0, d_out, out_pitch, d_raw}, st)) return rc;
    if (h->rp_on && h->rp.outputs) return sgm::reproject_frame(h, d_out, out_pitch, st);
    return SGM_OK;
}

int sgm::run_frame(sgm_handle *h, FrameIO f, hipStream_t st) {
    if (int rc = frame_maps(h, f, st)) return rc;
    // The output slot: with reprojection set, one launch more reads the frame's
    // final map and writes the products the handle was asked for
    if (h->rp_on && h->rp.outputs) return sgm::reproject_frame(h, f.out, f.out_pitch, st);
    return SGM_OK;
}

// post_filter() (Solver.cpp:600-649) in place on a device map (sgm_post.hip):
// median-fill launches until one changes nothing, then the speckle removal.
// The fill works on a separate map and the component kernels write the
// caller's map from it, so they are enqueued before the host reads the fill's
// convergence counter (the GPU keeps working through that round trip); in the
// rare case the fill had not converged, more fill launches run and the
// component kernels are enqueued again.
// to_lk: write the filtered map to d_lk_in (contiguous) instead of d_map, for
// lk_refine(..., staged = true) to read.
int sgm::post_filter(sgm_handle *h, float *d_map, int pitch, hipStream_t st, bool to_lk) {
    const Geom g = h->gt;  // (a true-disparity map: valid <= D + min_disp - 1)
    const int budget = h->pf_launches;
    // The number of median-fill launches depends on a counter read back to
    // the host each round; under stream capture that copy never runs, so a
    // captured graph would replay a fixed, possibly unconverged, fill.  (A
    // launch budget fixes the count and has the device judge it: below.)
    if (!budget) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        HIPCHK(h, hipStreamIsCapturing(st, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return set_err(h, SGM_ERR_INVALID_ARG,
                           "post_filter cannot be captured into a HIP graph (its median-fill launch "
                           "count is read back to the host); capture frames with post_filter = 0 or "
                           "set a launch budget (sgm_set_post_filter_launches)");
    }
    const double dnpx = (double)g.H * g.W;
    float *F = h->d_pf_work;
    HIPCHK(h, timed(h, "post_prep", dnpx, st, [&] {
               return sgm::launch_pf_prep(d_map, pitch, h->d_pf_orig, F, h->d_pf_changes,
                                          kMedianMaxLaunches, g, st);
           }));
    auto components = [&]() -> int {
        HIPCHK(h, timed(h, "post_cc_local", dnpx, st, [&] {
                   return sgm::launch_cc_local(F, h->d_pf_label, h->d_pf_count, h->d_pf_area, g, st);
               }));
        HIPCHK(h, timed(h, "post_cc_merge", dnpx, st,
                        [&] { return sgm::launch_cc_merge(F, h->d_pf_label, g, st); }));
        HIPCHK(h, timed(h, "post_cc_count", dnpx, st, [&] {
                   return sgm::launch_cc_count(h->d_pf_label, h->d_pf_count, h->d_pf_area, 1000 / g.scale,
                                               g, st);
               }));
        // speckle_filter_new(filtered_disp, invalid_disp, SPECKLE_SIZE/scale, SPECKLE_DIS), :645
        HIPCHK(h, timed(h, "post_cc_apply", dnpx, st, [&] {
                   return sgm::launch_cc_apply(F, h->d_pf_label, h->d_pf_area, 1000 / g.scale,
                                               (float)(g.D + 1), to_lk ? h->d_lk_in : d_map,
                                               to_lk ? g.W : pitch, g, st);
               }));
        return SGM_OK;
    };
    int k = 0, rc;
    if (budget) {
        // Fixed budget: exactly `budget` fill launches (those after the proof
        // return at their first instruction), the device's verdict on the
        // last counter, the component kernels once.  Nothing is read back and
        // nothing waits: the call returns after enqueueing and can be captured.
        // (with profiling on, one event pair around the whole sequence: a
        // budget of thousands must not take thousands of pooled events)
        HIPCHK(h, timed(h, "post_median", dnpx, st, [&] {
                   hipError_t e = hipSuccess;
                   for (; k < budget && e == hipSuccess; ++k)
                       e = sgm::launch_median_fill(h->d_pf_orig, F, k, h->d_pf_snap,
                                                   h->d_pf_changes, h->mf_rows, g, st);
                   if (e == hipSuccess)
                       e = sgm::launch_pf_verdict(h->d_pf_changes, budget, h->d_pf_err, st);
                   return e;
               }));
        h->pf_iters = k;
        return components();
    }
    for (;;) {
        // a fill usually settles in 2 launches and the 3rd proves it
        const int batch = k == 0 ? 3 : 2;
        for (int b = 0; b < batch; ++b, ++k)
            HIPCHK(h, timed(h, "post_median", dnpx, st, [&] {
                       return sgm::launch_median_fill(h->d_pf_orig, F, k, h->d_pf_snap,
                                                      h->d_pf_changes, h->mf_rows, g, st);
                   }));
        HIPCHK(h, hipMemcpyAsync(h->h_pf_changes, h->d_pf_changes + k - 1, sizeof(int),
                                 hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipEventRecord(h->ev_pf, st));
        if ((rc = components())) return rc;
        HIPCHK(h, hipEventSynchronize(h->ev_pf));
        if (*h->h_pf_changes == 0) break;
        if (k + 2 > kMedianMaxLaunches)
            return set_err(h, SGM_ERR_HIP, "post_filter: median fill did not converge in %d launches",
                           k);
    }
    h->pf_iters = k;
    return SGM_OK;
}

// LKRefine (sgm_lk.hip) in place on a device map: the kernel reads a
// contiguous copy of the map and writes the refined values back.
// staged: d_lk_in already holds the map (post_filter(..., to_lk = true))
int sgm::lk_refine(sgm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                   float *d_map, int map_pitch, hipStream_t st, bool staged) {
    const Geom g = h->gt;  // (DispValid: 0 < d < D + min_disp)
    const size_t row = (size_t)g.W * sizeof(float);
    if (!staged)
        HIPCHK(h, hipMemcpy2DAsync(h->d_lk_in, row, d_map, (size_t)map_pitch * sizeof(float), row,
                                   g.H, hipMemcpyDeviceToDevice, st));
    HIPCHK(h, timed(h, "lk_refine", (double)g.H * g.W, st, [&] {
               return sgm::launch_lk_refine(d_left, d_right, pitch, h->d_lk_in, d_map, map_pitch, g,
                                            st);
           }));
    return SGM_OK;
}
