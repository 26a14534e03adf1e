// sgm_capi.hip -- the C-ABI of libsgm_hip.so (include/sgm_hip.h): the entry points that enqueue work.
// The frame (sgm_process, sgm_process_device), the volume entry points and the
// _device entry point of every stage, sgm_check and the profiler's readout.
// The handle's lifetime and settings are in sgm_create.hip,
// the sgm_stage_* round trips in sgm_stages.hip, the input stage's part of the
// C-ABI in sgm_input.hip; what a frame enqueues is in sgm_frame.hip.
#include "sgm_handle.h"
#include "sgm_volume_args.h"
#include "sgm_window_cost_args.h"

using namespace sgm;

// Pinned staging for the host-buffer API: user rows are packed into pinned
// memory on the CPU, so every host<->device transfer is one contiguous DMA
// (pageable 2-D copies went through the runtime's staging path at a fraction
// of PCIe bandwidth).  Layout: left | right | sky_l | sky_r | out f32 | raw u16.
// (left, right: the images a frame takes, at the input stage's size and format)
static int ensure_pinned(sgm_handle *h) {
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

static void pack_rows(uint8_t *dst, const uint8_t *src, size_t row_bytes, int rows, size_t pitch) {
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

int sgm_check(sgm_handle *h) {
    if (!h) return SGM_ERR_INVALID_ARG;
    DeviceGuard guard(h->device);
    if (int rc = wait_last(h)) return rc;
    return check_frame_err(h);
}

// the view slot holding `view`'s maps (-1: the handle does not compute it)
static int view_slot(const sgm_handle *h, int view) {
    if (view != SGM_VIEW_LEFT && view != SGM_VIEW_RIGHT) return -1;
    if (h->nviews == 2) return view == SGM_VIEW_RIGHT ? 1 : 0;
    return view == h->p.view ? 0 : -1;  // (a right-view handle runs in slot 0)
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

}  // extern "C"
