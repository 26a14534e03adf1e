// sgm_internal.h -- kernel launchers and their argument structs (one view
// slot's cost stage: CostSlot; one view's aggregation roles: ViewRoles) shared
// by the host side (the C-ABI files, sgm_frame.hip) and the kernel files.  Not
// part of the public interface.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sgm_geom.h"
#include "sgm_gray_args.h"
#include "sgm_rectify_maps.h"
#include "sgm_resize_args.h"
#include "sgm_window_cost_args.h"

namespace sgm {

// Floats of slack after the final cost volume: row-walking prefetch rings may
// read up to 64 positions (x D <= 256) past the last row's end.
constexpr size_t kVolGuard = 64 * 256 + 256;

// Disparities per lane of a wave64 chain (lane l holds d = l*V .. l*V+V-1).
constexpr int vals_per_lane(int D) { return D >= 256 ? 4 : (D >= 128 ? 2 : 1); }

// Segment lengths K (chain steps between checkpoints) of the pair families,
// by values per lane.  The one definition: the kernels' pair_k<V>() /
// pair_kv<V>() (sgm_bodies.h), the checkpoint allocation (pair_ckpt_floats)
// and the guard below all derive from these.  The vertical family's final
// kernel holds five K x V register arrays, so it uses a shorter K to stay at
// <= 128 VGPRs (four waves per SIMD).
constexpr int seg_k_hd(int V) { return V >= 4 ? 8 : 16; }   // PAIR_H, PAIR_D2
constexpr int seg_k_v(int V) { return V >= 4 ? 4 : 8; }     // PAIR_V

// Rows of slack before the T volume read by the final pass (pair_split_body's
// WTA waves load a chunk from its top row; the partial last chunk's top lies
// up to K-1 rows above row 0, K = the vertical family's segment length).
constexpr int t_guard_rows(int D) { return seg_k_v(vals_per_lane(D)) - 1; }

// What a sweep does with its path costs L_r ("Sweeps").
enum SweepMode {
    SWEEP_STORE_L = 0,  // write L_r and minL_r (parity tests)
    SWEEP_INIT = 1,     // acc_out = L_r
    SWEEP_ACC = 2       // acc_out = acc_in + L_r   (acc_in may alias acc_out)
};

// A band of a backward pass: chain steps [kb, ke) of every chain (the rows
// H-ke .. H-1-kb of the walks that start at the bottom row), the chain state
// entering the band read from carry (kb > 0) and the state leaving it written
// there (ke < chain length; carry holds D floats per chain).  ke = 0: the
// whole chain.  The backward phase (stage B's diagonal pair, L8, final) runs
// band by band above the Infinity Cache, so that a band's cost volume and T
// stay cached from one pass to the next (DESIGN.md "Bands").
// Forward passes run bands too (rows [kb, ke) walked down, top band first:
// vfwd, L5, L6), with the same edges.
struct Band {
    int kb, ke;
    float *carry;
};

struct SweepArgs {
    const float *cost;   // HWD
    const float *acc_in; // HWD (ACC: chain state)
    float *acc_out;      // HWD (STORE_L: L_r)
    float *min_out;      // HW  (STORE_L: minL_r)
    float p1, p2;
    Band band;           // backward diagonal sweeps (DIR 6, 7: the L8 pass)
};

// Scanline families fused into forward/backward pairs (DESIGN.md "Pairs"):
// the forward direction stores its path state every K steps (checkpoints),
// the backward kernel recomputes each K-step segment of the forward costs from
// its checkpoint in registers and combines both on the fly.
enum PairFamily {
    PAIR_H = 0,   // L1 (->) forward, L2 (<-) backward, one chain per row
    PAIR_V = 1,   // L3 (down) forward, L4 (up) backward, one chain per column
    PAIR_D2 = 2   // L6 (down-left) forward, L7 (up-right) backward, wrapped anti-diagonals
};
enum PairMode {
    PAIR_INIT2 = 0,  // out = Lf + Lb                         (S12 = L1 + L2)
    PAIR_ACC = 1,    // out = (acc_in + Lf) + Lb              (T = (T5 + L6) + L7)
    PAIR_FINAL = 2   // total = ((s_in + Lf) + Lb) + acc_in   (S + T) -> WTA, sub-pixel
                     // (PAIR_V only: the three-wave final kernels)
};

struct PairArgs {
    const float *cost;
    const float *acc_in;
    const float *s_in;
    float *out;
    float *ckpt;
    uint16_t *disp;      // FINAL: raw WTA map, row-major (null: not wanted)
    float *sub;          // FINAL: sub-pixel map, row-major or (sub_cm) column-major
    int sub_cm;          // 1: sub[col * H + row] (two-view frames: lr_cm_kernel reads it)
    float *ratio;        // FINAL: match confidence min / second-min, in sub's layout
                         // (null: not wanted; sgm_set_confidence)
    int min_disp;        // FINAL: what index 0 stands for (sgm_set_min_disp): the maps
                         // leave as sub + (float)min_disp and disp + min_disp
    const float *zero;   // >= 256 zero floats: the cost of the virtual positions
                         // that align forward passes with their checkpoints
    float p1, p2, uniq;
    Band band;           // backward passes (D2 ACC, V FINAL): steps in whole segments
    int nt_cost;         // V FINAL (whole volume): read C by non-temporal loads -- the
                         // last read of a view's C when the other view's follows
};

// What the aggregation launches of one view take, role by role: the H pair
// (h1 forward, h2 backward), the diagonal pair (d6, d7), the L5 and L8 sweeps
// and the final pass (sgm_frame.hip's view_roles wires them to the buffers).
struct ViewRoles {
    PairArgs h1, h2, d6, d7, fin;
    SweepArgs l5, l8;
};

// floats of checkpoint storage a family needs
size_t pair_ckpt_floats(int family, Geom g);
// single roles (the sgm_stage_* parity entry points)
hipError_t launch_pair_fwd(int family, const PairArgs &a, Geom g, hipStream_t st);
hipError_t launch_pair_bwd(int family, int mode, const PairArgs &a, Geom g, hipStream_t st);
// The launches of the frame schedules (sgm_pair.hip, sgm_sweep.hip), each over
// the nviews (1 or 2) views r[0 .. nviews): one launcher per role, workgroup y
// (the final passes: z) = view.
// Stage A: L1 fwd | L5 -> T5 | L6 fwd; stage B: L2 bwd -> S12 | L7 bwd -> T.
// A banded stage B (r->d7.band, one view) runs no H rows: the banded
// schedule's H pair is its own launch.
hipError_t launch_stage_a(const ViewRoles *r, int nviews, Geom g, hipStream_t st);
hipError_t launch_stage_b(const ViewRoles *r, int nviews, Geom g, hipStream_t st);
// one forward band (r->l5.band, r->d6.band) of stage A's diagonal roles
// (DESIGN.md "Bands")
hipError_t launch_stage_a_band(const ViewRoles *r, Geom g, hipStream_t st);
// T += L8 (one view: launch_sweep's choice of body, bands included)
hipError_t launch_l8(const ViewRoles *r, int nviews, Geom g, hipStream_t st);
// The final pass, total = ((s_in + L3) + L4) + acc_in -> WTA, sub-pixel.  One
// view: banded by r->fin.band, C by non-temporal loads by r->fin.nt_cost.
// paths4 (params.paths == 4): without the T stream (acc_in
// unused), total = (s_in + L3) + L4.
hipError_t launch_final(const ViewRoles *r, int nviews, bool paths4, Geom g, hipStream_t st);
// The whole H pair as one launch (one wave per row: L1 forward, then L2
// backward -> r[v].h2.out); nt_cost: C by non-temporal loads (the banded and
// slanted schedules) or default loads (4-path frames)
hipError_t launch_hpair(const ViewRoles *r, int nviews, bool nt_cost, Geom g, hipStream_t st);
// 4-path frames: the H pair as a forward launch and a two-wave backward
// launch, C by default loads
hipError_t launch_h_fwd4(const ViewRoles *r, int nviews, Geom g, hipStream_t st);
hipError_t launch_h_bwd4(const ViewRoles *r, int nviews, Geom g, hipStream_t st);
// cost_vertical_filter (Solver.cpp:333-368) fused with the L3 forward pass of
// nviews views: in[v] = horizontally filtered volume, out[v] = final cost
// volume; a[v].ckpt takes the L3 checkpoints (l3 null; one view: banded by
// a->band), or l3[v] every row's L3 (the slanted schedule's bottom-up pass
// reads the volume)
hipError_t launch_vfwd(const float *const *in, float *const *out, const PairArgs *a, int nviews,
                       float *const *l3, Geom g, hipStream_t st);

// ----------------------------------------------- slanted tiles (sgm_slant.hip)
// (the tiles' widths kSlantNW, kSlantNWUp: sgm_geom.h)
// Polls before a receiver gives up on a hand-off (a hang guard: seconds).
constexpr unsigned kSlantSpinLimit = 1u << 22;
// Launch bookkeeping of one slanted pass kind, in device memory (zeroed at
// create): tickets claim tiles, the last workgroup out resets tickets/exits
// and advances epoch (the hand-off granules' tag), err counts hang-guard
// give-ups, dead = epoch + 1 of the last launch in which a receiver gave up
// (every later poll of that launch skips its wait, so one dead neighbour
// costs one spin limit, not one per step).
struct SlantCtl {
    unsigned tickets, exits, epoch, err, dead;
};
struct SlantView {
    const float *cost, *s12, *l3, *t56;  // HWD: C, L1+L2, L3, L5+L6 (bottom-up reads)
    float *t56w;                         // HWD: L5+L6 (the top-down pass writes it)
    float *sub;                          // HW sub-pixel map, row-major
    uint16_t *disp;                      // HW raw WTA map (null: not wanted)
    unsigned long long *gran;            // hand-off granules, slant_gran_count
    float *ratio;                        // HW match confidence, row-major (null: not wanted)
};
struct SlantArgs {
    SlantView v[2];
    SlantCtl *ctl;
    const float *zero;  // >= 256 zero floats
    float *dummy;       // >= 259 words: the target of inactive steps' stores
    float p1, p2, uniq;
    int min_disp;       // the bottom-up pass's maps leave as sub + (float)min_disp, disp + min_disp
    int nviews;
    int ntiles, grid;   // set by the launcher
    int max_grid;       // workgroups at most (0: one per CU)
    unsigned *err_host; // host-mapped word set to 1 when a hand-off poll gives up
    unsigned spin_limit;  // polls before giving up (kSlantSpinLimit; SGM_SLANT_DEBUG:
                          // SGM_SLANT_SPIN_LIMIT)
    int stall_tile;       // SGM_SLANT_DEBUG only (SGM_SLANT_STALL): the bottom-up pass's
                          // receiver of this tile of view 0 never accepts a granule, to
                          // exercise the give-up path; -1: none
};
size_t slant_tiles(Geom g, int nw);
// granules (8 B each) of nviews views' hand-offs
size_t slant_gran_count(Geom g, int nviews);
// both views' (a.nviews) bottom-up slanted pass: L4 + L7 + L8 + WTA (ctl[1])
hipError_t launch_slant_up(const SlantArgs &a, Geom g, hipStream_t st);
// both views' top-down slanted pass: T56 = L5 + L6 (ctl[0])
hipError_t launch_slant_down(const SlantArgs &a, Geom g, hipStream_t st);

// bm_rows: BM.cpp:24-25 decimation (rows not strided by the scale); src2/ct2:
// a second image censused in the same launch; win: the handle's matching window
// (sgm_set_window; the default launches census_kernel<3, 4> / <1, 2> as ever; win.weighted:
// the masked census of sgm_set_weighted)
hipError_t launch_census(const uint8_t *src, int pitch, Geom g, Window win, int blur, uint64_t *ct,
                         hipStream_t st, bool bm_rows = false, const uint8_t *src2 = nullptr,
                         uint64_t *ct2 = nullptr);
// BM's WTA (BM.cpp:53-85) over the filtered cost: raw disparity + its float copy
hipError_t launch_bm_wta(const float *cost, float uniq, uint16_t *disp, float *out, int out_pitch,
                         Geom g, hipStream_t st);
// The census tables shifted by k = min_disp / scale columns (sgm_set_min_disp):
// ctl_s[i, x] = ctl[i, min(x + k, W-1)], ctr_s[i, x] = ctr[i, max(x - k, 0)], one
// launch for both (a null output is skipped).  The left view's DSI of the
// search range [m, m + D) is the [0, D) DSI of (ctl, ctr_s), the right view's
// that of (ctl_s, ctr); with min_disp = 0 the shifted tables are the tables.
hipError_t launch_ct_shift(const uint64_t *ctl, const uint64_t *ctr, uint64_t *ctl_s, uint64_t *ctr_s,
                           int k, Geom g, hipStream_t st);
// What one view slot's cost stage takes (sgm_frame.hip's cost_slot wires it to
// the buffers; slot = the view's index in a frame's buffers).
struct CostSlot {
    const uint64_t *ctl, *ctr;  // the census table pair its DSI reads, resolved: DSI 0 the left
                                // table and the shifted right one, DSI 1 the shifted left one
                                // and the right one (launch_ct_shift; min_disp = 0: the tables)
    int dsi;                    // 0: build_dsi_from_table (left view), 1: ..._beta (right view)
    const uint8_t *sky;         // working-grid sky mask (null: no mask)
    float *ch;                  // the horizontally filtered volume, or the strip schedule's
                                // checkpoints, which reuse it
    uint64_t *skw;              // strips: the mask as one word per pixel (launch_sky_words), null as sky
    float *c, *l3;              // strips: the final cost C and the L3 volume
};
// The kernels that take both slots (cost_h2_kernel, cost_ck_kernel,
// vstrip_kernel) take the four tables and pick a DSI's pair themselves, (ctl,
// ctr_s) for DSI 0 and (ctl_s, ctr) for DSI 1: the slots' pairs, put back.  One
// slot fills its own DSI's pair; nothing reads the other.  With one slot ctl ==
// ctl_s and ctr == ctr_s (as the tables and their shifted ones are at min_disp
// = 0), and the kernels take all four as __restrict__: they may only ever be
// read.
struct CensusTables {
    const uint64_t *ctl, *ctr, *ctl_s, *ctr_s;
};
inline CensusTables census_tables(const CostSlot *s, int nviews) {
    const CostSlot &b = s[nviews - 1];
    return {s->ctl, b.ctr, b.ctl, s->ctr};
}
// The cost stage's launches, each over the nviews (1 or 2) slots s[0 .. nviews)
// of a frame, workgroup z (the strip pass: y) = slot.  Two slots are the frames'
// (DSI 0, DSI 1); they share a launch when cost_h_staged says so: rows that fit
// the staged kernels and both sky masks or neither.
bool cost_h_staged(const CostSlot *s, int nviews, Geom g);
// DSI + horizontal IIR into s[v].ch (filter = 0: the raw DSI; one slot only).
// One slot whose rows do not fit the staged kernel runs the global-memory one.
hipError_t launch_cost_h(const CostSlot *s, int nviews, int sky_pitch, int filter, Geom g,
                         hipStream_t st);
// The strip schedule of the slanted frames' cost stage (sgm_vstrip.hip):
// a checkpoint pass of the horizontal IIR (launch_cost_ck, sgm_cost.hip),
// then one pass writing C and the L3 volume (launch_vstrip).  kVStripNC
// columns per strip; checkpoints: H x strips x 3 x D floats per view.
#ifndef VSTRIP_NC
#define VSTRIP_NC 16
#endif
constexpr int kVStripNC = VSTRIP_NC;
size_t vstrip_strips(Geom g);
size_t vstrip_ck_floats(Geom g);
// scale 1 and cost_h_staged
bool vstrip_supported(const CostSlot *s, int nviews, Geom g);
// the checkpoints into s[v].ch
hipError_t launch_cost_ck(const CostSlot *s, int nviews, int sky_pitch, Geom g, hipStream_t st);
// dummy: >= 256 floats, the target of idle stores
hipError_t launch_vstrip(const CostSlot *s, int nviews, float *dummy, float p1, float p2, Geom g,
                         hipStream_t st);
// the sky mask as 0/1 words (the strip pass stages 8-byte words only), kept
// in the Ch buffer after the checkpoints (offset in floats)
size_t vstrip_sky_words_offset(Geom g);
hipError_t launch_sky_words(const uint8_t *sky, int pitch, Geom g, uint64_t *out, hipStream_t st);
hipError_t launch_copy(const float *in, float *out, Geom g, hipStream_t st);
hipError_t launch_sweep(int dir, int mode, const SweepArgs &a, Geom g, hipStream_t st);
// post_filter (sgm_post.hip)
size_t post_snapshot_floats(Geom g);
int median_rows_default(Geom g);
hipError_t launch_median_fill(const float *orig, float *F, int iter, float *snap, int *changes,
                              int rows, Geom g, hipStream_t st);
hipError_t launch_pf_prep(const float *map, int pitch, float *orig, float *F, int *changes,
                          int nchanges, Geom g, hipStream_t st);
// fixed-budget fill: stores n to *err_host (host-mapped) when changes[n-1] != 0
hipError_t launch_pf_verdict(const int *changes, int n, unsigned *err_host, hipStream_t st);
hipError_t launch_cc_local(const float *F, int *L, int *cnt, int *area, Geom g, hipStream_t st);
hipError_t launch_cc_merge(const float *F, int *L, Geom g, hipStream_t st);
hipError_t launch_cc_count(int *L, const int *cnt, int *area, int max_size, Geom g,
                           hipStream_t st);
hipError_t launch_cc_apply(const float *F, const int *L, const int *area, int max_size,
                           float value, float *out, int out_pitch, Geom g, hipStream_t st);
// LKRefine (sgm_lk.hip): left/right full-size images (decimated by g.scale on
// the fly), din the working-grid map, dout (pitched) the refined map.
hipError_t launch_lk_refine(const uint8_t *left, const uint8_t *right, int pitch, const float *din,
                            float *dout, int out_pitch, Geom g, hipStream_t st);
// SkyAreaDetector::detect (sgm_sky.hip) on nviews (1 or 2) images at once:
// img[v] full-size (decimated by g.scale), mask[v] on the working grid;
// scratch of nviews * sky_scratch_bytes(g) bytes.
size_t sky_scratch_bytes(Geom g);
hipError_t launch_sky_detect(const uint8_t *const *img, int pitch, uint8_t *const *mask,
                             int mask_pitch, void *scratch, int nviews, Geom g, hipStream_t st);
// The node's cv::resize (node.cpp:75-76; sgm_resize.hip) of nviews
// (1 or 2) u8 images of one size in one launch: src[v] src_rows x src_cols
// (src_pitch bytes) -> dst[v] dst_rows x dst_cols (dst_pitch bytes, padding untouched).
// fmt: the source's pixel format (SGM_PIX_*; a colour source is converted to
// grey tap by tap), dst is always one channel.
hipError_t launch_resize(const uint8_t *const *src, int src_rows, int src_cols, int src_pitch,
                         uint8_t *const *dst, int dst_rows, int dst_cols, int dst_pitch, int nviews,
                         hipStream_t st, int fmt = 0);
// The rectification remap (sgm_rectify.hip) of nviews (1 or 2) u8
// images of one size in one launch: src[v] src_rows x src_cols (src_pitch
// bytes) sampled through map[v] (dst_rows x dst_cols packed entries of two
// words, sgm_rectify_maps.h) -> dst[v] (dst_pitch bytes, padding untouched).
// fmt: the source's pixel format, as launch_resize's.
hipError_t launch_rectify(const uint8_t *const *src, int src_rows, int src_cols, int src_pitch,
                          const uint32_t *const *map, uint8_t *const *dst, int dst_rows, int dst_cols,
                          int dst_pitch, int nviews, hipStream_t st, int fmt = 0);
// Colour to grey (sgm_gray.hip) of nviews (1 or 2) images of one
// size in one launch: src[v] rows x cols pixels of a colour format fmt
// (src_pitch bytes) -> dst[v] rows x cols u8 (dst_pitch bytes, padding untouched).
hipError_t launch_gray(int fmt, const uint8_t *const *src, int rows, int cols, int src_pitch,
                       uint8_t *const *dst, int dst_pitch, int nviews, hipStream_t st);
// reprojection through Q (sgm_reproject.hip): the products whose pointers are not
// null, pitches in elements; invalid: the map's invalid marker; form: the XYZ store form (0 | 1)
hipError_t launch_reproject(const double *q, const float *disp, int pitch, float *xyz, int xyz_pitch,
                            float *depth, int depth_pitch, uint16_t *depth16, int depth16_pitch,
                            float invalid, float max_range, float depth_scale, int form, Geom g,
                            hipStream_t st);
// A caller's cost volume (sgm_volume.hip) into dense fp32 HWD volumes in one launch:
// src of dtype SGM_VOL_* with element (i, j, d) at src[i * stride_row + j * stride_col + d * stride_disp]
// (strides in elements, one of stride_col and stride_disp is 1: sgm_volume_args.h) -> dst_l, the
// re-layout, and dst_r, C_R[i, j, d] = C_L[i, min(j + (d + min_disp) / scale, W - 1), d]; a null
// destination is skipped.  The destinations must not overlap the source.
hipError_t launch_volume_import(const void *src, int dtype, long long stride_row, long long stride_col,
                                long long stride_disp, float *dst_l, float *dst_r, int min_disp, Geom g,
                                hipStream_t st);
// cost_horizontal_filter(COST_WIN_W / scale) (Solver.cpp:296-330) over nviews (1 or 2) dense fp32 HWD
// volumes in one launch (sgm_volume_filter.hip): in[v] -> out[v], in place where
// out[v] == in[v] (else the volumes must not overlap); nt: the output by non-temporal stores (a
// volume read once, as Ch by vfwd).  g.W >= 5 / g.scale.
hipError_t launch_volume_hfilter(const float *const *in, float *const *out, int nviews, bool nt, Geom g,
                                 hipStream_t st);
// the steps of one prefetched block of its main loop (the widths around it: tests)
int volume_filter_block();
// The SAD (kind 1) or SSD (kind 2) window cost of two grey images (sgm_window_cost.hip, DESIGN.md
// 5o) as the dense fp32 HWD left volume, one launch: left, right of g.H * g.scale rows and g.W *
// g.scale columns, pitch bytes per row, read decimated by g.scale and not blurred.  win.weighted
// (sgm_set_weighted): the weighted producer, with weights = window_weights' table of
// win (host memory, copied into the launch's arguments); else weights is not read.
hipError_t launch_window_cost(int kind, const uint8_t *left, const uint8_t *right, int pitch, float *dst,
                              int min_disp, Geom g, Window win, const float *weights, hipStream_t st);
// consumers (sgm_consumers.hip): Solver::colormap and the node's point cloud
// (min_disp: the map is in true disparity; the colours are those of disp - min_disp over g.D)
hipError_t launch_colormap(const float *disp, int pitch, uint8_t *bgr, int bgr_pitch, int min_disp,
                           Geom g, hipStream_t st);
hipError_t launch_point_cloud(const float *disp, int pitch, const uint8_t *img, int img_pitch,
                              float fx, float fy, float cx, float cy, double baseline,
                              float max_range, int *counts, double *xyz, uint8_t *pixel,
                              int *total, Geom g, hipStream_t st);
hipError_t launch_lr(const float *fl, int fl_pitch, const float *fr, int fr_pitch, float *out,
                     int out_pitch, float lr, Geom g, hipStream_t st);
// the same LR check on COLUMN-major maps fl_cm, fr_cm (x[col * H + row], as
// the two-view frame's final passes write them), row-major out
hipError_t launch_lr_cm(const float *fl_cm, const float *fr_cm, float *out, int out_pitch, float lr,
                        Geom g, hipStream_t st);
// the match-confidence map of a view to a caller's pitched row-major buffer:
// src column-major (cm: src[col * H + row], as the two-view final passes
// store it beside sub) or row-major
hipError_t launch_ratio_out(const float *src, int cm, float *out, int out_pitch, Geom g,
                            hipStream_t st);
// in place: disp = D + 1 where ratio > max_ratio
hipError_t launch_confidence_filter(float *disp, int pitch, const float *ratio, int ratio_pitch,
                                    float max_ratio, Geom g, hipStream_t st);

}  // namespace sgm
