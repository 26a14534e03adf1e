// sgm_create.hip -- the handle's lifetime and settings (include/sgm_hip.h): sgm_create, sgm_destroy, the setters.
// sgm_create checks the parameters and plans the handle (valid_params,
// plan_handle: sgm_plan.h) before it allocates; the plan sizes the buffers and
// is the schedule of every frame.
// All device memory is allocated at sgm_create (the reference allocates its
// scratch in the constructors, Solver.cpp:18-27 and SGM.cpp:7-24), apart from
// the maps the setters switch on and off; all of it is on the handle's ledger.
#include "sgm_handle.h"
#include "sgm_window_cost_args.h"

#include <stdlib.h>
#include <new>

using namespace sgm;

namespace {

// Frees what the handle owns (it is deleted next): every dalloc still on the
// ledger, then the host-pinned buffers, streams and events.
void free_all(sgm_handle *h) {
    h->mem.free_all();
    void *pinned[] = {h->h_pf_changes, h->h_pf_err, h->h_slant_err, h->h_pin};
    for (void *p : pinned)
        if (p) (void)hipHostFree(p);
    if (h->st) (void)hipStreamDestroy(h->st);
    if (h->st_h) (void)hipStreamDestroy(h->st_h);
    hipEvent_t evs[] = {h->ev_pf, h->ev_last, h->ev_fork, h->ev_join};
    for (auto e : evs) if (e) (void)hipEventDestroy(e);
    for (auto &p : h->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : h->ev_pool) (void)hipEventDestroy(e);
    h->pending.clear();
    h->ev_pool.clear();
}

// sgm_create's steps, in its order; each returns an rc, with the reason in
// h->err where there is one.  (The order of the device allocations is kept as
// it ever was: inputs, per-view buffers, common buffers, the slanted
// schedule's.)

int create_streams(sgm_handle *h) {
    if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) return SGM_ERR_HIP;
    hipEvent_t *evs[] = {&h->ev_pf, &h->ev_last};
    for (auto e : evs) {
        // stream-to-stream ordering on this device needs no system-scope
        // fence (L2 writeback/invalidate); the post filter's host
        // readback (ev_pf) keeps it
        const unsigned fl = hipEventDisableTiming | (e == &h->ev_pf ? 0u : hipEventDisableSystemFence);
        if (hipEventCreateWithFlags(e, fl) != hipSuccess) return SGM_ERR_HIP;
    }
    return SGM_OK;
}

// Every handle's input buffers: the staged images, the sky masks, the census tables.
int alloc_inputs(sgm_handle *h) {
    const size_t npx = (size_t)h->g.H * h->g.W, nin = (size_t)h->p.height * h->p.width;
    for (int v = 0; v < 2; ++v) {
        if (int rc = dalloc(h, &h->d_in[v], nin)) return rc;
        if (int rc = dalloc(h, &h->d_sky[v], npx)) return rc;
        if (int rc = dalloc(h, &h->d_ct[v], npx)) return rc;
        h->d_cts[v] = h->d_ct[v];  // (min_disp = 0: the tables themselves)
    }
    return SGM_OK;
}

// Each view's volumes, maps, checkpoints and band carries (aux_only handles:
// the side stages' maps alone).
int alloc_views(sgm_handle *h) {
    const Geom g = h->g;
    const size_t npx = (size_t)g.H * g.W, nvol = npx * g.D;
    const bool paths4 = h->plan.paths4;
    for (int v = 0; v < (h->p.aux_only ? 0 : h->nviews); ++v) {
        // the final pass addresses T (which reuses d_ch) in chunks from
        // their top row, which for the partial last chunk lies up to K-1
        // rows above row 0: d_ch carries that guard in front; the
        // row-walking passes prefetch up to PF positions past the end of
        // the last row of C (never consumed): both carry kVolGuard behind
        const size_t guard = (size_t)sgm::t_guard_rows(g.D) * g.W * g.D;
        if (int rc = dalloc(h, &h->d_ch_base[v], guard + nvol + sgm::kVolGuard)) return rc;
        h->d_ch[v] = h->d_ch_base[v] + guard;
        if (int rc = dalloc(h, &h->d_c[v], nvol + sgm::kVolGuard)) return rc;
        if (int rc = dalloc(h, &h->d_s[v], nvol)) return rc;
        if (int rc = dalloc(h, &h->d_disp[v], npx)) return rc;
        if (int rc = dalloc(h, &h->d_sub[v], npx)) return rc;
        // (a 4-path handle has no diagonal pair and never runs bands)
        for (int f = 0; f < 3; ++f)
            if (!(paths4 && f == sgm::PAIR_D2))
                if (int rc = dalloc(h, &h->d_ck[v][f], sgm::pair_ckpt_floats(f, g))) return rc;
        // slot 2 also holds vfwd's forward-band state (3 D-vectors per column)
        for (int f = 0; f < 3 && !paths4; ++f)
            if (int rc = dalloc(h, &h->d_carry[v][f], (size_t)g.W * g.D * (f == 2 ? 3 : 1))) return rc;
    }
    if (h->p.aux_only) {  // the side stages' maps (stage_lr, the raw map copy)
        for (int v = 0; v < 2; ++v) {
            if (int rc = dalloc(h, &h->d_disp[v], npx)) return rc;
            if (int rc = dalloc(h, &h->d_sub[v], npx)) return rc;
        }
    } else if (h->nviews == 1) {  // stage_lr needs a second sub-pixel map
        if (int rc = dalloc(h, &h->d_sub[1], npx)) return rc;
    }
    return SGM_OK;
}

// What every handle has beside them: the output map, the zero page, the
// scratch of the post filter, LKRefine, the sky detector and the point cloud.
int alloc_common(sgm_handle *h) {
    const size_t npx = (size_t)h->g.H * h->g.W;
    int rc = dalloc(h, &h->d_cloud_counts, (size_t)h->g.H + 1);
    if (!rc) rc = dalloc(h, &h->d_out, npx);
    if (!rc) rc = dalloc(h, &h->d_min, npx);
    if (!rc) rc = dalloc(h, &h->d_zero, 256);
    if (!rc) rc = dalloc(h, &h->d_pf_orig, npx);
    if (!rc) rc = dalloc(h, &h->d_pf_work, npx);
    if (!rc) rc = dalloc(h, &h->d_pf_label, npx);
    if (!rc) rc = dalloc(h, &h->d_pf_count, npx);
    if (!rc) rc = dalloc(h, &h->d_pf_area, npx);
    if (!rc) rc = dalloc(h, &h->d_pf_snap, sgm::post_snapshot_floats(h->g));
    if (!rc) rc = dalloc(h, &h->d_lk_in, npx);
    if (!rc) rc = dalloc(h, &h->d_sky_scratch, 2 * sgm::sky_scratch_bytes(h->g));
    if (!rc) rc = dalloc(h, &h->d_pf_changes, (size_t)kMedianMaxLaunches);
    if (rc) return rc;
    if (hipHostMalloc((void **)&h->h_pf_changes, sizeof(int), hipHostMallocDefault) != hipSuccess)
        return set_err(h, SGM_ERR_HIP, "hipHostMalloc of the post-filter counter failed");
    if (hipHostMalloc((void **)&h->h_pf_err, sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&h->d_pf_err, h->h_pf_err, 0) != hipSuccess)
        return set_err(h, SGM_ERR_HIP, "hipHostMalloc of the post filter's verdict word failed");
    *h->h_pf_err = 0;
    return SGM_OK;
}

// The slanted schedule's buffers (plan.slant), last: its two large ones, the L3
// volumes and the hand-off granules (about 28 GB for a 4K256 pair, whose whole
// handle is about 80 GB: INTEGRATION.md 5), come after every other buffer, so
// that the fallback covers any shortage they cause.  Where the schedule was
// chosen by size, not asked for (plan.slant_forced), and the device cannot hold
// them, the handle is planned again without it -- the banded schedule,
// bit-identical maps, no extra volume -- instead of failing sgm_create.
int alloc_slant(sgm_handle *h) {
    if (!h->plan.slant) return SGM_OK;
    const size_t nvol = (size_t)h->g.H * h->g.W * h->g.D;
    int rc = SGM_OK;
    Ledger::Group large(h->mem);  // (not committed: freed as the function returns)
    for (int v = 0; v < h->nviews && !rc; ++v) rc = dalloc(h, &h->d_l3[v], nvol);
    if (!rc) rc = dalloc(h, &h->d_gran, sgm::slant_gran_count(h->g, h->nviews));
#ifdef SGM_SLANT_DEBUG
    if (!rc && getenv("SGM_SLANT_NO_MEMORY"))  // (tests the fallback below)
        rc = set_err(h, SGM_ERR_HIP, "hipMalloc: out of memory (forced, SGM_SLANT_NO_MEMORY)");
#endif
    if (!rc) large.commit();
    if (rc && !h->plan.slant_forced) {
        (void)hipGetLastError();  // (the failed hipMalloc's error is not the next launch's)
        h->err[0] = 0;
        h->plan = sgm::plan_without_slant(h->plan);
        return SGM_OK;
    }
    if (!rc) rc = dalloc(h, &h->d_slant_ctl, 2);
    if (!rc) rc = dalloc(h, &h->d_slant_dummy, 512);
    if (rc) return rc;
    if (hipHostMalloc((void **)&h->h_slant_err, sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&h->d_slant_err, h->h_slant_err, 0) != hipSuccess)
        return set_err(h, SGM_ERR_HIP, "hipHostMalloc of the slanted schedule's hang-guard word failed");
    *h->h_slant_err = 0;
    // (the H pair's stream beside the top-down pass, its fork and join)
    if (hipStreamCreateWithFlags(&h->st_h, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess)
        return set_err(h, SGM_ERR_HIP, "creating the slanted schedule's H-pair stream failed");
    return SGM_OK;
}

// What has to read as zero before the first frame.
int clear_buffers(sgm_handle *h) {
    if (hipMemset(h->d_zero, 0, 256 * sizeof(float)) != hipSuccess)
        return set_err(h, SGM_ERR_HIP, "hipMemset of the zero page failed");
    if (h->plan.slant &&
        (hipMemset(h->d_gran, 0, sgm::slant_gran_count(h->g, h->nviews) * sizeof(unsigned long long)) != hipSuccess ||
         hipMemset(h->d_slant_ctl, 0, 2 * sizeof(sgm::SlantCtl)) != hipSuccess))
        return set_err(h, SGM_ERR_HIP, "hipMemset of the slanted schedule's hand-off state failed");
    return SGM_OK;
}

// SGM_CONFIDENCE=1: handles start with the confidence maps on (timing the
// feature's cost under tools that create their own handles, tools/ab_env.sh)
int start_confidence(sgm_handle *h) {
    const char *e = getenv("SGM_CONFIDENCE");
    if (!e || *e != '1' || h->p.aux_only || h->p.solver != SGM_SOLVER_SGM) return SGM_OK;
    return sgm_set_confidence(h, 1) != SGM_OK ? SGM_ERR_OUT_OF_MEMORY : SGM_OK;
}

}  // namespace

extern "C" {

int sgm_default_params(sgm_params *p, int h, int w, int s, int d) {
    if (!p) return SGM_ERR_INVALID_ARG;
    sgm::default_params(p, h, w, s, d);
    return SGM_OK;
}

int sgm_create(const sgm_params *p, int device, sgm_handle **out) {
    if (!out) return SGM_ERR_INVALID_ARG;
    *out = nullptr;
    char why[256];
    if (!valid_params(p, why, sizeof(why))) {
        fprintf(stderr, "sgm_create: %s\n", why);
        return SGM_ERR_INVALID_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SGM_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(device);

    sgm_handle *h = new (std::nothrow) sgm_handle();
    if (!h) return SGM_ERR_OUT_OF_MEMORY;
    h->p = *p;
    h->device = device;
    h->plan = plan_handle(*p, slant_cus(), plan_env());
    h->g = h->plan.g;
    h->gt = h->g;  // (min_disp = 0 until sgm_set_min_disp)
    h->nviews = h->plan.nviews;
    h->win_h = sgm::kWinH;  // (the reference's window until sgm_set_window)
    h->win_w = sgm::kWinW;
    h->win = sgm::default_window(h->g.scale);
    h->mf_rows = sgm::median_rows_default(h->g);

    int rc = create_streams(h);
    if (!rc) rc = alloc_inputs(h);
    if (!rc) rc = alloc_views(h);
    if (!rc) rc = alloc_common(h);
    if (!rc) rc = alloc_slant(h);  // (may leave the slanted schedule: h->plan is final after it)
    if (!rc) rc = clear_buffers(h);
    if (!rc) rc = start_confidence(h);
    if (rc) {
        fprintf(stderr, "sgm_create: %s\n", h->err[0] ? h->err : "HIP stream/event creation failed");
        free_all(h);
        delete h;
        return rc;
    }
    *out = h;
    return SGM_OK;
}

int sgm_destroy(sgm_handle *h) {
    if (!h) return SGM_ERR_INVALID_ARG;
    {
        DeviceGuard guard(h->device);
        (void)hipDeviceSynchronize();
        free_all(h);
    }
    delete h;
    return SGM_OK;
}

// ---- settings.  A setter that allocates does so as one group on the ledger: all of its buffers or none,
// the setting as it was.  (The input stage's: sgm_input.hip; the fill's and the reprojection's beside their kernels.)

const char *sgm_last_error(const sgm_handle *h) { return h ? h->err : "null handle"; }

int sgm_get_size(const sgm_handle *h, int *rows, int *cols, int *max_disp) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (rows) *rows = h->g.H;
    if (cols) *cols = h->g.W;
    if (max_disp) *max_disp = h->g.D;
    return SGM_OK;
}

size_t sgm_device_bytes(const sgm_handle *h) { return h ? h->mem.sum : 0; }

void *sgm_get_stream(const sgm_handle *h) { return h ? (void *)h->st : nullptr; }

int sgm_get_invalid_disp(const sgm_handle *h, int *invalid) {
    if (!h || !invalid) return SGM_ERR_INVALID_ARG;
    *invalid = h->gt.D + 1;
    return SGM_OK;
}

int sgm_set_post_filter_launches(sgm_handle *h, int n) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (n < 0 || n > kMedianMaxLaunches)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_post_filter_launches: n must be 0 (adaptive) or 1..%d, got %d",
                       kMedianMaxLaunches, n);
    if (!h->d_pf_changes || !h->d_pf_err)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_post_filter_launches: the handle has no post-filter buffers");
    h->pf_launches = n;
    return SGM_OK;
}

int sgm_set_min_disp(sgm_handle *h, int m) {
    if (!h) return SGM_ERR_INVALID_ARG;
    // The shifted census tables move by whole working-grid columns, and the
    // raw u16 map must hold the invalid marker D + m + 1
    if (m < 0) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_min_disp: min_disp must be >= 0, got %d", m);
    if (m % h->g.scale != 0)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_min_disp: min_disp must be a multiple of scale (the tables shift by "
                       "min_disp / scale columns)");
    if ((long long)h->g.D + m + 1 > 65535)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_min_disp: max_disp + min_disp + 1 must fit the raw u16 map (<= 65535)");
    if (h->p.solver == SGM_SOLVER_BM && m != 0)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_min_disp: not supported by the BM solver");
    // (frames in flight still read the tables and the handle's geometry)
    return change_setting(h, "sgm_set_min_disp", m == h->min_disp, [&]() -> int {
        // each image's shifted table (16 B per pixel for both; frames write the
        // ones their views read, sgm_stage_cost its view's); at 0 the tables
        // themselves, nothing allocated.  (aux_only handles compute no cost.)
        const bool want = m != 0 && !h->p.aux_only, have = h->d_cts[0] != h->d_ct[0];
        if (want && !have) {
            uint64_t *t[2] = {nullptr, nullptr};
            Ledger::Group both(h->mem);
            for (auto &q : t)
                if (int rc = dalloc(h, &q, (size_t)h->g.H * h->g.W)) return rc;
            both.commit();
            h->d_cts[0] = t[0];
            h->d_cts[1] = t[1];
        } else if (!want && have) {
            for (int v = 0; v < 2; ++v) {
                dfree(h, &h->d_cts[v]);
                h->d_cts[v] = h->d_ct[v];
            }
        }
        h->min_disp = m;
        h->gt.D = h->g.D + m;
        return SGM_OK;
    });
}

int sgm_set_window(sgm_handle *h, int win_h, int win_w) {
    if (!h) return SGM_ERR_INVALID_ARG;
    // (a weighted handle takes odd effective windows only: weighted_refusal)
    if (const char *why = h->win.weighted ? sgm::weighted_refusal(win_h, win_w, h->g.scale)
                                          : sgm::window_refusal(win_h, win_w, h->g.scale))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_window: %s, got (%d, %d) at scale %d", why, win_h, win_w,
                       h->g.scale);
    // (frames enqueued so far keep the launches they were given; the wait keeps the setter's
    // contract that of sgm_set_min_disp.  Nothing is allocated: the tables are words whatever
    // the window, and the window costs stage in LDS)
    return change_setting(h, "sgm_set_window", win_h == h->win_h && win_w == h->win_w, [&]() -> int {
        h->win_h = win_h;
        h->win_w = win_w;
        const bool weighted = h->win.weighted;
        h->win = sgm::window_of(win_h, win_w, h->g.scale);
        h->win.weighted = weighted;
        if (weighted) sgm::window_weights(h->win, h->weights);
        return SGM_OK;
    });
}

int sgm_get_window(const sgm_handle *h, int *win_h, int *win_w) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (win_h) *win_h = h->win_h;
    if (win_w) *win_w = h->win_w;
    return SGM_OK;
}

int sgm_set_weighted(sgm_handle *h, int enable) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (enable)
        if (const char *why = sgm::weighted_refusal(h->win_h, h->win_w, h->g.scale))
            return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_weighted: %s, the window is (%d, %d) at scale %d", why,
                           h->win_h, h->win_w, h->g.scale);
    // (as sgm_set_window: frames enqueued so far keep their launches; nothing is allocated, the
    // table travels in the producer's arguments and the census's mask is compiled in)
    return change_setting(h, "sgm_set_weighted", (enable != 0) == h->win.weighted, [&]() -> int {
        h->win.weighted = enable != 0;
        if (enable) sgm::window_weights(h->win, h->weights);
        return SGM_OK;
    });
}

int sgm_get_weighted(const sgm_handle *h, int *enabled) {
    if (!h || !enabled) return SGM_ERR_INVALID_ARG;
    *enabled = h->win.weighted ? 1 : 0;
    return SGM_OK;
}

int sgm_get_window_weights(sgm_handle *h, float *w, int max, int *count) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!h->win.weighted)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_get_window_weights: the handle is not weighted (sgm_set_weighted)");
    const int n = h->win.eh * h->win.ew;
    if (w && max < n)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_get_window_weights: the table has %d entries, max is %d", n, max);
    if (w) memcpy(w, h->weights, (size_t)n * sizeof(float));
    if (count) *count = n;
    return SGM_OK;
}

int sgm_set_confidence(sgm_handle *h, int enable) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only || h->p.solver != SGM_SOLVER_SGM)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_confidence: BM and aux_only handles run no aggregated WTA");
    // (frames in flight still store through, or read, the maps)
    const bool unchanged = (enable != 0) == (h->d_ratio[0] != nullptr);
    return change_setting(h, "sgm_set_confidence", unchanged, [&]() -> int {
        const size_t npx = (size_t)h->g.H * h->g.W;
        if (!enable) {
            for (int v = 0; v < 2; ++v) dfree(h, &h->d_ratio[v]);
            return SGM_OK;
        }
        Ledger::Group maps(h->mem);
        for (int v = 0; v < h->nviews; ++v) {
            if (int rc = dalloc(h, &h->d_ratio[v], npx)) return rc;
            // (a map no frame has written yet reads as zeros)
            if (hipMemset(h->d_ratio[v], 0, npx * sizeof(float)) != hipSuccess)
                return set_err(h, SGM_ERR_HIP, "hipMemset of the confidence map failed");
            h->ratio_cm[v] = false;
        }
        maps.commit();
        return SGM_OK;
    });
}

int sgm_set_cost(sgm_handle *h, int kind) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (kind != SGM_COST_CENSUS && !sgm::window_cost_kind(kind))
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_cost: kind must be SGM_COST_CENSUS, SGM_COST_SAD, SGM_COST_SSD or SGM_COST_CT, got %d",
                       kind);
    if (h->p.aux_only || h->p.solver != SGM_SOLVER_SGM)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_cost: BM and aux_only handles run no SGM frames");
    if (h->p.view == SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_cost: a SGM_VIEW_RIGHT handle (the window costs build the left view's volume)");
    if (h->p.sky_detect)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_cost: a sky_detect handle (sky masks have no meaning in build_dsi)");
    // (a host-side switch the next frame reads: every frame handle already holds the buffers of
    // the whole-volume passes, and frames enqueued so far keep the launches they were given)
    h->cost_kind = kind;
    return SGM_OK;
}

int sgm_get_cost(const sgm_handle *h, int *kind) {
    if (!h || !kind) return SGM_ERR_INVALID_ARG;
    *kind = h->cost_kind;
    return SGM_OK;
}

int sgm_window_cost_tile_cols(void) { return sgm::kWinCostTileCols; }

int sgm_set_volume_filter(sgm_handle *h, int filters) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (filters & ~(SGM_FILTER_H | SGM_FILTER_V))
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_volume_filter: filters must be 0 or SGM_FILTER_H | SGM_FILTER_V bits, got %d", filters);
    if (h->p.aux_only || h->p.solver != SGM_SOLVER_SGM)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_volume_filter: BM and aux_only handles run no volume frames");
    if (h->p.view == SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_volume_filter: a SGM_VIEW_RIGHT handle (volume frames start from the left view's)");
    // (a host-side switch the next volume frame reads, as sgm_set_cost: the filters work in the
    // C and Ch volumes every frame handle holds)
    h->vol_filter = filters;
    return SGM_OK;
}

int sgm_get_volume_filter(const sgm_handle *h, int *filters) {
    if (!h || !filters) return SGM_ERR_INVALID_ARG;
    *filters = h->vol_filter;
    return SGM_OK;
}

int sgm_volume_filter_block(void) { return sgm::volume_filter_block(); }

int sgm_vstrip_cols(void) { return sgm::kVStripNC; }

int sgm_set_profiling(sgm_handle *h, int enable) {
    if (!h) return SGM_ERR_INVALID_ARG;
    h->profiling = enable ? 1 : 0;
    return SGM_OK;
}

#ifdef SGM_SLANT_DEBUG
// hang-guard give-ups of the slanted passes (SlantCtl::err), read and cleared
int sgm_debug_slant_err(sgm_handle *h, unsigned *down, unsigned *up) {
    if (!h || !h->d_slant_ctl) return SGM_ERR_INVALID_ARG;
    sgm::SlantCtl c[2];
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(c, h->d_slant_ctl, sizeof(c), hipMemcpyDeviceToHost));
    *down = c[0].err;
    *up = c[1].err;
    c[0].err = c[1].err = 0;
    HIPCHK(h, hipMemcpy(h->d_slant_ctl, c, sizeof(c), hipMemcpyHostToDevice));
    return SGM_OK;
}
#endif

}  // extern "C"
