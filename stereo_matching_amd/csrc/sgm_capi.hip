// sgm_capi.hip -- the C-ABI of libsgm_hip.so (include/sgm_hip.h).
//
// sgm_create / sgm_destroy and the setters, the extern "C" entry points and the
// sgm_stage_* functions of the parity tests.  The input stage's part of the
// C-ABI is in sgm_input.hip; what a frame enqueues is in sgm_frame.hip.
// sgm_create checks the parameters and plans the handle (valid_params,
// plan_handle: sgm_plan.h) before it allocates; the plan sizes the buffers and
// is the schedule of every frame.
// All device memory is allocated at sgm_create (the reference allocates its
// scratch in the constructors, Solver.cpp:18-27 and SGM.cpp:7-24), apart from
// the maps the setters switch on and off.
#include "sgm_handle.h"
#include "sgm_volume_args.h"
#include "sgm_window_cost_args.h"

#include <stdlib.h>
#include <new>

using namespace sgm;

namespace {

// Frees what the handle owns (it is deleted next): every dalloc still on the
// list, then the host-pinned buffers, streams and events.
void free_all(sgm_handle *h) {
    for (void *p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
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
    const size_t nvol = (size_t)h->g.H * h->g.W * h->g.D, ng = sgm::slant_gran_count(h->g, h->nviews);
    int rc = SGM_OK;
    for (int v = 0; v < h->nviews && !rc; ++v) rc = dalloc(h, &h->d_l3[v], nvol);
    if (!rc) rc = dalloc(h, &h->d_gran, ng);
#ifdef SGM_SLANT_DEBUG
    if (!rc && getenv("SGM_SLANT_NO_MEMORY"))  // (tests the fallback below)
        rc = set_err(h, SGM_ERR_HIP, "hipMalloc: out of memory (forced, SGM_SLANT_NO_MEMORY)");
#endif
    if (rc && !h->plan.slant_forced) {
        for (int v = 0; v < 2; ++v) dfree(h, &h->d_l3[v], nvol);
        dfree(h, &h->d_gran, ng);
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

// Pinned staging for the host-buffer API: user rows are packed into pinned
// memory on the CPU, so every host<->device transfer is one contiguous DMA
// (pageable 2-D copies went through the runtime's staging path at a fraction
// of PCIe bandwidth).  Layout: left | right | sky_l | sky_r | out f32 | raw u16.
// (left, right: the images a frame takes, at the input stage's size and format)
int ensure_pinned(sgm_handle *h) {
    const size_t nin = (size_t)h->in.rows(h->p.height) * h->in.row_bytes(h->p.width);
    const size_t npx = (size_t)h->g.H * h->g.W;
    const size_t need = 2 * nin + 2 * npx + npx * sizeof(float) + npx * sizeof(uint16_t) + 64;
    if (h->h_pin && h->h_pin_bytes >= need) return SGM_OK;
    if (h->h_pin) (void)hipHostFree(h->h_pin);
    h->h_pin = nullptr;
    HIPCHK(h, hipHostMalloc((void **)&h->h_pin, need, hipHostMallocDefault));
    h->h_pin_bytes = need;
    return SGM_OK;
}

int copy_in_image(sgm_handle *h, uint8_t *dst, const uint8_t *src, int pitch) {
    HIPCHK(h, hipMemcpy2DAsync(dst, (size_t)h->p.width, src, (size_t)pitch, (size_t)h->p.width,
                               (size_t)h->p.height, hipMemcpyHostToDevice, h->st));
    return SGM_OK;
}

void pack_rows(uint8_t *dst, const uint8_t *src, size_t row_bytes, int rows, size_t pitch) {
    if (pitch == row_bytes) {
        memcpy(dst, src, row_bytes * rows);
        return;
    }
    for (int i = 0; i < rows; ++i) memcpy(dst + i * row_bytes, src + i * pitch, row_bytes);
}

// The slanted passes' hang guard (sgm_slant.hip): a receiver that polls a
// neighbouring tile's hand-off for seconds gives up, and that frame's maps
// are wrong.  It sets a host-mapped word; the next call on the handle (or
// sgm_process, after its own frame) reports it and clears it.
// The fixed-budget post filter (sgm_set_post_filter_launches) reports the
// same way through a word of its own (every handle has one): its verdict
// kernel sets it when the budget's last fill launch still changed a tile.
int check_frame_err(sgm_handle *h) {
    // read and clear in one step: a give-up stored by a frame still running
    // between a plain read and a plain clear would be lost
    const bool slant = h->h_slant_err && __atomic_exchange_n(h->h_slant_err, 0u, __ATOMIC_ACQ_REL);
    // (the verdict kernel stores the budget that was not enough: 1..4096)
    const unsigned fill = h->h_pf_err ? __atomic_exchange_n(h->h_pf_err, 0u, __ATOMIC_ACQ_REL) : 0u;
    if (!slant && !fill) return SGM_OK;
    if (!fill)
        return set_err(h, SGM_ERR_HIP, "slanted aggregation: a tile hand-off timed out; that frame's maps are invalid");
    return set_err(h, SGM_ERR_HIP,
                   "post_filter: median fill not proven in %u launches "
                   "(sgm_set_post_filter_launches); that frame's map is invalid%s",
                   fill, slant ? "; slanted aggregation: a tile hand-off timed out too" : "");
}

}  // namespace

// Waits for the last call's work: on a caller's stream its end was recorded
// in ev_last; on the handle's own stream, that stream (the H pair's stream
// is joined into the frame's stream before the bottom-up pass).
int wait_last(sgm_handle *h) {
    if (h->last_st && h->last_recorded) HIPCHK(h, hipEventSynchronize(h->ev_last));
    else if (!h->last_st || h->last_st == h->st) HIPCHK(h, hipStreamSynchronize(h->st));
    else HIPCHK(h, hipDeviceSynchronize());  // a caller's stream whose end could not be recorded
    return SGM_OK;
}

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

const char *sgm_last_error(const sgm_handle *h) { return h ? h->err : "null handle"; }

int sgm_get_size(const sgm_handle *h, int *rows, int *cols, int *max_disp) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (rows) *rows = h->g.H;
    if (cols) *cols = h->g.W;
    if (max_disp) *max_disp = h->g.D;
    return SGM_OK;
}

size_t sgm_device_bytes(const sgm_handle *h) { return h ? h->bytes : 0; }

void *sgm_get_stream(const sgm_handle *h) { return h ? (void *)h->st : nullptr; }

int sgm_check(sgm_handle *h) {
    if (!h) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    if (int rc = wait_last(h)) return rc;
    return check_frame_err(h);
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

// the view slot holding `view`'s maps (-1: the handle does not compute it)
static int view_slot(const sgm_handle *h, int view) {
    if (view != SGM_VIEW_LEFT && view != SGM_VIEW_RIGHT) return -1;
    if (h->nviews == 2) return view == SGM_VIEW_RIGHT ? 1 : 0;
    return view == h->p.view ? 0 : -1;  // (a right-view handle runs in slot 0)
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
        const size_t npx = (size_t)h->g.H * h->g.W;
        // each image's shifted table (16 B per pixel for both; frames write the
        // ones their views read, sgm_stage_cost its view's); at 0 the tables
        // themselves, nothing allocated.  (aux_only handles compute no cost.)
        const bool want = m != 0 && !h->p.aux_only, have = h->d_cts[0] != h->d_ct[0];
        if (want && !have) {
            uint64_t *t[2] = {nullptr, nullptr};
            int rc = dalloc(h, &t[0], npx);
            if (!rc) rc = dalloc(h, &t[1], npx);
            if (rc) {
                for (auto &q : t) dfree(h, &q, npx);
                return rc;
            }
            h->d_cts[0] = t[0];
            h->d_cts[1] = t[1];
        } else if (!want && have) {
            for (int v = 0; v < 2; ++v) {
                dfree(h, &h->d_cts[v], npx);
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
            for (int v = 0; v < 2; ++v) dfree(h, &h->d_ratio[v], npx);
            return SGM_OK;
        }
        for (int v = 0; v < h->nviews; ++v) {
            int rc = dalloc(h, &h->d_ratio[v], npx);
            // (a map no frame has written yet reads as zeros)
            if (!rc && hipMemset(h->d_ratio[v], 0, npx * sizeof(float)) != hipSuccess)
                rc = set_err(h, SGM_ERR_HIP, "hipMemset of the confidence map failed");
            if (rc) {
                for (int w = 0; w < 2; ++w) dfree(h, &h->d_ratio[w], npx);
                return rc;
            }
            h->ratio_cm[v] = false;
        }
        return SGM_OK;
    });
}

int sgm_confidence_device(sgm_handle *h, int view, float *d_ratio, int pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_ratio || pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_confidence_device: bad pointer or pitch");
    const int slot = view_slot(h, view);
    if (slot < 0)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_confidence_device: the handle does not compute view %d", view);
    if (!h->d_ratio[slot])
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_confidence_device: confidence is off (sgm_set_confidence)");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "confidence_out", (double)h->g.H * h->g.W, st, [&] {
               return sgm::launch_ratio_out(h->d_ratio[slot], h->ratio_cm[slot] ? 1 : 0, d_ratio, pitch,
                                            h->g, st);
           }));
    return SGM_OK;
}

int sgm_stage_confidence(sgm_handle *h, int view, float *ratio) {
    if (!h || !ratio) return SGM_ERR_INVALID_ARG;
    // staged through the post filter's working map (dead between calls)
    if (int rc = sgm_confidence_device(h, view, h->d_pf_work, h->g.W, nullptr)) return rc;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipMemcpyAsync(ratio, h->d_pf_work, (size_t)h->g.H * h->g.W * sizeof(float),
                             hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_confidence_filter_device(sgm_handle *h, float *d_disp, int pitch, const float *d_ratio,
                                 int ratio_pitch, float max_ratio, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_disp || !d_ratio || pitch < h->g.W || ratio_pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_confidence_filter_device: bad pointer or pitch");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "confidence_filter", (double)h->g.H * h->g.W, st, [&] {
               return sgm::launch_confidence_filter(d_disp, pitch, d_ratio, ratio_pitch, max_ratio, h->gt,
                                                    st);
           }));
    return SGM_OK;
}

int sgm_stage_confidence_filter(sgm_handle *h, float *disp, const float *ratio, float max_ratio) {
    if (!h || !disp || !ratio) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    HIPCHK(h, hipMemcpyAsync(h->d_out, disp, npx * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(h->d_pf_work, ratio, npx * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, sgm::launch_confidence_filter(h->d_out, h->g.W, h->d_pf_work, h->g.W, max_ratio, h->gt,
                                            h->st));
    HIPCHK(h, hipMemcpyAsync(disp, h->d_out, npx * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_post_filter_proved_at(sgm_handle *h, int *launch) {
    if (!h || !launch) return SGM_ERR_INVALID_ARG;
    *launch = 0;
    DeviceGuard guard(h->device);
    if (int rc = wait_last(h)) return rc;
    if (h->pf_iters <= 0) return SGM_OK;  // no post filter yet
    // (a query, not part of a frame: the counters are read synchronously)
    std::vector<int> c((size_t)h->pf_iters);
    HIPCHK(h, hipMemcpy(c.data(), h->d_pf_changes, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < c.size(); ++k)
        if (c[k] == 0) {
            *launch = (int)k + 1;
            break;
        }
    return SGM_OK;
}

// The checks a frame's arguments pass before anything is enqueued (host or device pointers alike);
// `fn`: the entry point's name, for the message.
static int check_frame_args(sgm_handle *h, const char *fn, const uint8_t *left, const uint8_t *right, int pitch,
                            const uint8_t *sky_l, const uint8_t *sky_r, int sky_pitch, const float *out,
                            int out_pitch) {
    if (!left || !right || !out || pitch < h->in.row_bytes(h->p.width) || out_pitch < h->g.W ||
        ((sky_l || sky_r) && sky_pitch < h->g.W))
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: bad pointer or pitch", fn);
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "%s: handle created with aux_only", fn);
    if (h->cost_kind != SGM_COST_CENSUS && (sky_l || sky_r))
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: sky masks have no meaning with a SAD or SSD cost (sgm_set_cost)",
                       fn);
    return SGM_OK;
}

int sgm_process_device(sgm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                       const uint8_t *d_sky_l, const uint8_t *d_sky_r, int sky_pitch,
                       float *d_out, int out_pitch, uint16_t *d_raw_disp, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (int rc = check_frame_err(h)) return rc;
    if (int rc = check_frame_args(h, "sgm_process_device", d_left, d_right, pitch, d_sky_l, d_sky_r, sky_pitch, d_out,
                                  out_pitch))
        return rc;
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    return run_frame(h, {d_left, d_right, pitch, d_sky_l, d_sky_r, sky_pitch, d_out, out_pitch, d_raw_disp},
                     scope.st);
}

int sgm_process(sgm_handle *h, const uint8_t *left, const uint8_t *right, int pitch,
                const uint8_t *sky_l, const uint8_t *sky_r, int sky_pitch, float *out,
                int out_pitch, uint16_t *raw_disp) {
    if (!h) return SGM_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_frame_args(h, "sgm_process", left, right, pitch, sky_l, sky_r, sky_pitch, out, out_pitch))) return rc;
    if ((rc = check_frame_err(h))) return rc;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    if ((rc = ensure_pinned(h))) return rc;
    // (a handle that stages, sgm_input_stage.h, takes the raw images in its staging buffers and
    // the frame resizes, remaps or converts them; in_w: their bytes per row)
    const int in_h = h->in.rows(h->p.height), in_w = h->in.row_bytes(h->p.width);
    uint8_t *const *d_in = h->in.stages(h->p.aux_only) ? h->d_raw : h->d_in;
    const size_t nin = (size_t)in_h * in_w, npx = (size_t)h->g.H * h->g.W;
    uint8_t *pl = h->h_pin, *pr = pl + nin, *psl = pr + nin, *psr = psl + npx;
    float *pout = reinterpret_cast<float *>(psr + npx + (16 - (size_t)(psr + npx) % 16) % 16);
    uint16_t *praw = reinterpret_cast<uint16_t *>(pout + npx);
    pack_rows(pl, left, in_w, in_h, pitch);
    pack_rows(pr, right, in_w, in_h, pitch);
    HIPCHK(h, hipMemcpyAsync(d_in[0], pl, nin, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(d_in[1], pr, nin, hipMemcpyHostToDevice, h->st));
    if (sky_l) {
        pack_rows(psl, sky_l, h->g.W, h->g.H, sky_pitch);
        HIPCHK(h, hipMemcpyAsync(h->d_sky[0], psl, npx, hipMemcpyHostToDevice, h->st));
    }
    if (sky_r) {
        pack_rows(psr, sky_r, h->g.W, h->g.H, sky_pitch);
        HIPCHK(h, hipMemcpyAsync(h->d_sky[1], psr, npx, hipMemcpyHostToDevice, h->st));
    }
    const FrameIO f = {d_in[0], d_in[1], in_w, sky_l ? h->d_sky[0] : nullptr,
                       sky_r ? h->d_sky[1] : nullptr, h->g.W, h->d_out, h->g.W,
                       raw_disp ? h->d_disp[0] : nullptr};
    if ((rc = run_frame(h, f, h->st))) return rc;
    HIPCHK(h, hipMemcpyAsync(pout, h->d_out, npx * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (raw_disp)
        HIPCHK(h, hipMemcpyAsync(praw, h->d_disp[0], npx * sizeof(uint16_t), hipMemcpyDeviceToHost,
                                 h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if ((rc = check_frame_err(h))) return rc;
    for (int i = 0; i < h->g.H; ++i)
        memcpy(out + (size_t)i * out_pitch, pout + (size_t)i * h->g.W, h->g.W * sizeof(float));
    if (raw_disp) memcpy(raw_disp, praw, npx * sizeof(uint16_t));
    return SGM_OK;
}

// The volume entry points take no hipStreamLegacy: a call's end recorded on the legacy stream is an
// event the next call on another stream would wait on; that wait crashed the host in torch's HIP
// runtime (sgm_hip.h).  `fn`: the entry point's name, for the message.
static int refuse_legacy_stream(sgm_handle *h, const char *fn, void *stream) {
    if (stream != (void *)hipStreamLegacy) return SGM_OK;
    return set_err(h, SGM_ERR_INVALID_ARG,
                   "%s: hipStreamLegacy is not accepted; pass a created stream, or NULL for the handle's own", fn);
}

// The checks a caller's volume passes before anything is enqueued (sgm_volume_args.h); `fn`: the
// entry point's name, for the message.
static int check_volume(sgm_handle *h, const char *fn, const sgm_volume *vol, void *stream) {
    if (!vol || !vol->d_cost) return set_err(h, SGM_ERR_INVALID_ARG, "%s: NULL volume", fn);
    if (int rc = refuse_legacy_stream(h, fn, stream)) return rc;
    char why[256];
    if (!sgm::volume_layout(vol->dtype, vol->stride_row, vol->stride_col, vol->stride_disp, h->g.H, h->g.W,
                            h->g.D, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: %s", fn, why);
    if ((uintptr_t)vol->d_cost % (uintptr_t)sgm::volume_elem_bytes(vol->dtype))
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: d_cost is not aligned to its element type", fn);
    return SGM_OK;
}

int sgm_volume_import_device(sgm_handle *h, const sgm_volume *vol, int view, float *d_dst, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (int rc = check_volume(h, "sgm_volume_import_device", vol, stream)) return rc;
    if (!d_dst || (uintptr_t)d_dst % sizeof(float))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_volume_import_device: d_dst is NULL or not a float pointer");
    if (view != SGM_VIEW_LEFT && view != SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_volume_import_device: view must be SGM_VIEW_LEFT or SGM_VIEW_RIGHT");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "vol_import", vol_elems(h->g), st, [&] {
               return sgm::launch_volume_import(vol->d_cost, vol->dtype, vol->stride_row, vol->stride_col,
                                                vol->stride_disp, view == SGM_VIEW_LEFT ? d_dst : nullptr,
                                                view == SGM_VIEW_RIGHT ? d_dst : nullptr, h->min_disp, h->g, st);
           }));
    return SGM_OK;
}

int sgm_aggregate_device(sgm_handle *h, const sgm_volume *vol, float *d_out, int out_pitch, uint16_t *d_raw,
                         void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (int rc = check_frame_err(h)) return rc;
    if (h->p.aux_only)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_aggregate_device: handle created with aux_only (no cost volumes)");
    if (h->p.solver != SGM_SOLVER_SGM)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_aggregate_device: a BM handle aggregates nothing");
    if (h->p.view == SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_aggregate_device: a SGM_VIEW_RIGHT handle (the volume is the left view's)");
    if (h->p.lk_refine)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_aggregate_device: params.lk_refine needs images; run sgm_lk_refine_device afterwards");
    if (int rc = check_volume(h, "sgm_aggregate_device", vol, stream)) return rc;
    if (!d_out || out_pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_aggregate_device: d_out is NULL or out_pitch below cols");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    return aggregate_volume(h, *vol, d_out, out_pitch, d_raw, scope.st);
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

int sgm_window_cost_device(sgm_handle *h, int kind, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                           float *d_dst, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (const char *why = sgm::window_cost_refusal(kind, d_left, d_right, pitch, h->p.width, d_dst))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_window_cost_device: %s", why);
    if (int rc = refuse_legacy_stream(h, "sgm_window_cost_device", stream)) return rc;
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, window_cost_name(h, kind), vol_elems(h->g), st, [&] {
               return sgm::launch_window_cost(kind, d_left, d_right, pitch, d_dst, h->min_disp, h->g, h->win,
                                              h->weights, st);
           }));
    return SGM_OK;
}

int sgm_stage_window_cost(sgm_handle *h, int kind, const uint8_t *left, const uint8_t *right, int pitch,
                          float *cost) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (const char *why = sgm::window_cost_refusal(kind, left, right, pitch, h->p.width, cost))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_window_cost: %s", why);
    DeviceGuard guard(h->device);
    int rc;
    const size_t nvol = (size_t)h->g.H * h->g.W * h->g.D;
    {
        StreamScope scope(h, nullptr);
        if ((rc = copy_in_image(h, h->d_in[0], left, pitch))) return rc;
        if ((rc = copy_in_image(h, h->d_in[1], right, pitch))) return rc;
    }
    // (an aux_only handle has no cost buffer: a temporary of the call's own)
    StreamTemp<float> d_cost(h->st);
    HIPCHK(h, hipMallocAsync((void **)&d_cost.p, nvol * sizeof(float), h->st));
    if ((rc = sgm_window_cost_device(h, kind, h->d_in[0], h->d_in[1], h->p.width, d_cost.p, nullptr))) return rc;
    HIPCHK(h, hipMemcpyAsync(cost, d_cost.p, nvol * sizeof(float), hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

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

int sgm_filter_volume_device(sgm_handle *h, float *d_cost, int filters, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_cost || (uintptr_t)d_cost % 16)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_filter_volume_device: d_cost is NULL or not 16-byte aligned");
    if (filters < 1 || filters > (SGM_FILTER_H | SGM_FILTER_V))
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_filter_volume_device: filters must be SGM_FILTER_H, SGM_FILTER_V or both, got %d", filters);
    if (int rc = refuse_legacy_stream(h, "sgm_filter_volume_device", stream)) return rc;
    if (h->p.aux_only)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_filter_volume_device: handle created with aux_only (no Ch volume to filter through)");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    return sgm::filter_volume(h, d_cost, filters, scope.st);
}

int sgm_stage_filter_volume(sgm_handle *h, float *cost, int filters) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!cost) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_filter_volume: NULL volume");
    if (h->p.aux_only)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_filter_volume: handle created with aux_only (no cost volumes)");
    DeviceGuard guard(h->device);
    const size_t nvol = (size_t)h->g.H * h->g.W * h->g.D;
    {  // staged in view 0's C
        StreamScope scope(h, nullptr);
        HIPCHK(h, hipMemcpyAsync(h->d_c[0], cost, nvol * sizeof(float), hipMemcpyHostToDevice, h->st));
    }
    if (int rc = sgm_filter_volume_device(h, h->d_c[0], filters, nullptr)) return rc;
    HIPCHK(h, hipMemcpyAsync(cost, h->d_c[0], nvol * sizeof(float), hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
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

int sgm_set_profiling(sgm_handle *h, int enable) {
    if (!h) return SGM_ERR_INVALID_ARG;
    h->profiling = enable ? 1 : 0;
    return SGM_OK;
}

int sgm_get_profile(sgm_handle *h, sgm_kernel_stat *out, int max, int *count) {
    if (!h) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    for (auto &p : h->pending) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, p.a, p.b));
        h->stats[p.cls].launches += 1;
        h->stats[p.cls].total_ms += ms;
        h->stat_elems[p.cls] += p.elems;
        h->ev_pool.push_back(p.a);
        h->ev_pool.push_back(p.b);
    }
    h->pending.clear();
    int n = 0;
    for (size_t k = 0; k < h->stats.size(); ++k) {
        sgm_kernel_stat &st = h->stats[k];
        if (st.launches == 0) continue;
        st.elems = h->stat_elems[k] / st.launches;  // banded launches differ in size
        if (out && n < max) out[n] = st;
        ++n;
    }
    if (count) *count = out ? (n < max ? n : max) : n;
    for (auto &st : h->stats) { st.launches = 0; st.total_ms = 0; }
    for (auto &e : h->stat_elems) e = 0.0;
    return SGM_OK;
}

// -------------------------------------------------------------- stages

int sgm_stage_census(sgm_handle *h, const uint8_t *img, int pitch, uint64_t *ct) {
    if (!h || !img || !ct || pitch < h->p.width) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    int rc;
    if ((rc = copy_in_image(h, h->d_in[0], img, pitch))) return rc;
    HIPCHK(h, sgm::launch_census(h->d_in[0], h->p.width, h->g, h->win, h->p.blur, h->d_ct[0], h->st));
    HIPCHK(h, hipMemcpyAsync(ct, h->d_ct[0], (size_t)h->g.H * h->g.W * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_get_invalid_disp(const sgm_handle *h, int *invalid) {
    if (!h || !invalid) return SGM_ERR_INVALID_ARG;
    *invalid = h->gt.D + 1;
    return SGM_OK;
}

int sgm_stage_cost(sgm_handle *h, const uint64_t *ctl, const uint64_t *ctr, const uint8_t *sky,
                   int view, int filters, float *cost) {
    if (!h || !ctl || !ctr || !cost || (view != 0 && view != 1)) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "stage needs cost volumes (aux_only)");
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W, nvol = npx * h->g.D;
    HIPCHK(h, hipMemcpyAsync(h->d_ct[0], ctl, npx * 8, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(h->d_ct[1], ctr, npx * 8, hipMemcpyHostToDevice, h->st));
    if (sky) HIPCHK(h, hipMemcpyAsync(h->d_sky[0], sky, npx, hipMemcpyHostToDevice, h->st));
    // (min_disp: the view's shift applied to the tables as handed in)
    const sgm::CostSlot s = sgm::cost_slot(h, 0, view, sky ? h->d_sky[0] : nullptr);
    if (int rc = shift_tables(h, &s, 1, h->st)) return rc;
    HIPCHK(h, sgm::launch_cost_h(&s, 1, h->g.W, filters & 1, h->g, h->st));
    const float *res = h->d_ch[0];
    if (filters & 2) {  // the frame's own vfwd, in place when the frames run it so
        if (int rc = sgm::vfwd_view(h, 0, res, cost_buf(h, 0), (double)nvol, h->st)) return rc;
        res = cost_buf(h, 0);
    }
    HIPCHK(h, hipMemcpyAsync(cost, res, nvol * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_stage_path(sgm_handle *h, int dir, const float *cost, float *L, float *minL) {
    if (!h || !cost || !L || dir < 0 || dir > 7) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "stage needs cost volumes (aux_only)");
    if (h->plan.paths4 && dir >= SGM_DIR_L5)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_path: a 4-path handle serves L1..L4 only");
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W, nvol = npx * h->g.D;
    HIPCHK(h, hipMemcpyAsync(h->d_c[0], cost, nvol * 4, hipMemcpyHostToDevice, h->st));
    SweepArgs a = sweep_args(h);
    a.cost = h->d_c[0];
    a.acc_out = h->d_s[0];
    a.min_out = h->d_min;
    HIPCHK(h, sgm::launch_sweep(dir, sgm::SWEEP_STORE_L, a, h->g, h->st));
    HIPCHK(h, hipMemcpyAsync(L, h->d_s[0], nvol * 4, hipMemcpyDeviceToHost, h->st));
    if (minL) HIPCHK(h, hipMemcpyAsync(minL, h->d_min, npx * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_stage_aggregate(sgm_handle *h, const float *cost, uint16_t *disp, float *sub) {
    if (!h || !cost) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "stage needs cost volumes (aux_only)");
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W, nvol = npx * h->g.D;
    HIPCHK(h, hipMemcpyAsync(h->d_c[0], cost, nvol * 4, hipMemcpyHostToDevice, h->st));
    if (int rc = stage_aggregate(h, h->st)) return rc;
    if (disp) HIPCHK(h, hipMemcpyAsync(disp, h->d_disp[0], npx * 2, hipMemcpyDeviceToHost, h->st));
    if (sub) HIPCHK(h, hipMemcpyAsync(sub, h->d_sub[0], npx * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_lr_check_device(sgm_handle *h, const float *d_fl, int fl_pitch, const float *d_fr,
                        int fr_pitch, float *d_out, int out_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    const int W = h->g.W;
    if (!d_fl || !d_fr || !d_out || fl_pitch < W || fr_pitch < W || out_pitch < W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_lr_check_device: bad pointer or pitch");
    if (d_out == d_fr)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_lr_check_device: d_out must not alias d_fr");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "lr", (double)h->g.H * W, st, [&] {
               return sgm::launch_lr(d_fl, fl_pitch, d_fr, fr_pitch, d_out, out_pitch,
                                     h->p.lr_max_diff, h->gt, st);
           }));
    return SGM_OK;
}

int sgm_post_filter_device(sgm_handle *h, float *d_disp, int pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_disp || pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_post_filter_device: bad pointer or pitch");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    return post_filter(h, d_disp, pitch, scope.st);
}

int sgm_lk_refine_device(sgm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                         float *d_disp, int disp_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_left || !d_right || !d_disp || pitch < h->p.width || disp_pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_lk_refine_device: bad pointer or pitch");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    return lk_refine(h, d_left, d_right, pitch, d_disp, disp_pitch, scope.st);
}

int sgm_stage_lk_refine(sgm_handle *h, const uint8_t *left, const uint8_t *right, int pitch,
                        float *disp) {
    if (!h || !left || !right || !disp || pitch < h->p.width) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    int rc;
    if ((rc = copy_in_image(h, h->d_in[0], left, pitch))) return rc;
    if ((rc = copy_in_image(h, h->d_in[1], right, pitch))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_out, disp, npx * 4, hipMemcpyHostToDevice, h->st));
    if ((rc = lk_refine(h, h->d_in[0], h->d_in[1], h->p.width, h->d_out, h->g.W, h->st))) return rc;
    HIPCHK(h, hipMemcpyAsync(disp, h->d_out, npx * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_sky_detect_device(sgm_handle *h, const uint8_t *d_img, int pitch, uint8_t *d_mask,
                          int mask_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_img || !d_mask || pitch < h->p.width || mask_pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_sky_detect_device: bad pointer or pitch");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "sky_detect", (double)h->g.H * h->g.W, st, [&] {
               return sgm::launch_sky_detect(&d_img, pitch, &d_mask, mask_pitch, h->d_sky_scratch,
                                             1, h->g, st);
           }));
    return SGM_OK;
}

int sgm_stage_sky_detect(sgm_handle *h, const uint8_t *img, int pitch, uint8_t *mask) {
    if (!h || !img || !mask || pitch < h->p.width) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    int rc;
    if ((rc = copy_in_image(h, h->d_in[0], img, pitch))) return rc;
    if ((rc = sgm_sky_detect_device(h, h->d_in[0], h->p.width, h->d_sky[0], h->g.W, h->st)))
        return rc;
    HIPCHK(h, hipMemcpyAsync(mask, h->d_sky[0], npx, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

int sgm_colormap_device(sgm_handle *h, const float *d_disp, int pitch, uint8_t *d_bgr,
                        int bgr_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_disp || !d_bgr || pitch < h->g.W || bgr_pitch < 3 * h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_colormap_device: bad pointer or pitch");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "colormap", (double)h->g.H * h->g.W, st, [&] {
               return sgm::launch_colormap(d_disp, pitch, d_bgr, bgr_pitch, h->min_disp, h->g, st);
           }));
    return SGM_OK;
}

int sgm_point_cloud_device(sgm_handle *h, const float *d_disp, int pitch, const uint8_t *d_img,
                           int img_pitch, const sgm_camera *cam, double *d_xyz,
                           uint8_t *d_pixel, int *d_count, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_disp || !d_img || !cam || !d_xyz || !d_pixel || !d_count || pitch < h->g.W ||
        img_pitch < h->g.W)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_point_cloud_device: bad pointer or pitch");
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "point_cloud", (double)h->g.H * h->g.W, st, [&] {
               return sgm::launch_point_cloud(d_disp, pitch, d_img, img_pitch, cam->fx, cam->fy,
                                              cam->cx, cam->cy, cam->baseline, cam->max_range,
                                              h->d_cloud_counts, d_xyz, d_pixel, d_count, h->gt,
                                              st);
           }));
    return SGM_OK;
}

int sgm_stage_colormap(sgm_handle *h, const float *disp, uint8_t *bgr) {
    if (!h || !disp || !bgr) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    int rc;
    {
        // staging: the map in d_out, the BGR image in a stream-ordered temporary
        StreamTemp<uint8_t> d_bgr(h->st);
        HIPCHK(h, hipMallocAsync((void **)&d_bgr.p, 3 * npx, h->st));
        HIPCHK(h, hipMemcpyAsync(h->d_out, disp, npx * 4, hipMemcpyHostToDevice, h->st));
        rc = sgm_colormap_device(h, h->d_out, h->g.W, d_bgr.p, 3 * h->g.W, h->st);
        if (!rc) HIPCHK(h, hipMemcpyAsync(bgr, d_bgr.p, 3 * npx, hipMemcpyDeviceToHost, h->st));
    }
    HIPCHK(h, hipStreamSynchronize(h->st));
    return rc;
}

int sgm_stage_point_cloud(sgm_handle *h, const float *disp, const uint8_t *img, int img_pitch,
                          const sgm_camera *cam, double *xyz, uint8_t *pixel, int *count) {
    if (!h || !disp || !img || !cam || !xyz || !pixel || !count || img_pitch < h->g.W)
        return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    const int rows_used = h->g.H;  // the node reads img(i, j) at working-grid indices
    int rc;
    {
        // (declared last to first: the scope's end frees d_img, d_pix, d_xyz, d_n in this order)
        StreamTemp<int> d_n(h->st);
        StreamTemp<double> d_xyz(h->st);
        StreamTemp<uint8_t> d_pix(h->st), d_img(h->st);
        HIPCHK(h, hipMallocAsync((void **)&d_img.p, (size_t)rows_used * img_pitch, h->st));
        HIPCHK(h, hipMallocAsync((void **)&d_pix.p, npx, h->st));
        HIPCHK(h, hipMallocAsync((void **)&d_xyz.p, 3 * npx * sizeof(double), h->st));
        HIPCHK(h, hipMallocAsync((void **)&d_n.p, sizeof(int), h->st));
        HIPCHK(h, hipMemcpyAsync(d_img.p, img, (size_t)rows_used * img_pitch, hipMemcpyHostToDevice,
                                 h->st));
        HIPCHK(h, hipMemcpyAsync(h->d_out, disp, npx * 4, hipMemcpyHostToDevice, h->st));
        rc = sgm_point_cloud_device(h, h->d_out, h->g.W, d_img.p, img_pitch, cam, d_xyz.p, d_pix.p,
                                    d_n.p, h->st);
        if (!rc) {
            HIPCHK(h, hipMemcpyAsync(count, d_n.p, sizeof(int), hipMemcpyDeviceToHost, h->st));
            HIPCHK(h, hipStreamSynchronize(h->st));
            HIPCHK(h, hipMemcpyAsync(xyz, d_xyz.p, 3 * (size_t)*count * sizeof(double),
                                     hipMemcpyDeviceToHost, h->st));
            HIPCHK(h, hipMemcpyAsync(pixel, d_pix.p, (size_t)*count, hipMemcpyDeviceToHost, h->st));
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->st));
    return rc;
}

int sgm_stage_post_filter(sgm_handle *h, float *disp) {
    if (!h || !disp) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    HIPCHK(h, hipMemcpyAsync(h->d_out, disp, npx * 4, hipMemcpyHostToDevice, h->st));
    int rc = post_filter(h, h->d_out, h->g.W, h->st);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(disp, h->d_out, npx * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    // synchronous: a fixed-budget fill that was not proven is this call's error
    return check_frame_err(h);
}

int sgm_stage_lr(sgm_handle *h, const float *fl, const float *fr, float *out) {
    if (!h || !fl || !fr || !out) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    StreamScope scope(h, nullptr);
    const size_t npx = (size_t)h->g.H * h->g.W;
    HIPCHK(h, hipMemcpyAsync(h->d_sub[0], fl, npx * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(h->d_sub[1], fr, npx * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, sgm::launch_lr(h->d_sub[0], h->g.W, h->d_sub[1], h->g.W, h->d_out, h->g.W,
                             h->p.lr_max_diff, h->gt, h->st));
    HIPCHK(h, hipMemcpyAsync(out, h->d_out, npx * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return SGM_OK;
}

}  // extern "C"
