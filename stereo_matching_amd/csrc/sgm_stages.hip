// sgm_stages.hip -- the sgm_stage_* functions of the parity tests (include/sgm_hip.h): one stage on
// host buffers, each a round trip (Staging, sgm_handle.h) through the staging buffers named in it and the launch
// or _device entry point the frames use.  (The input stage's, the fill's, the reprojection's: beside their setters.)
#include "sgm_handle.h"
#include "sgm_window_cost_args.h"

using namespace sgm;

extern "C" {

int sgm_stage_census(sgm_handle *h, const uint8_t *img, int pitch, uint64_t *ct) {
    if (!h || !img || !ct || pitch < h->p.width) return SGM_ERR_INVALID_ARG;
    Staging s(h);
    s.up_rows(h->d_in[0], img, h->p.width, h->p.height, pitch);
    STAGE_HIP(s, sgm::launch_census(h->d_in[0], h->p.width, h->g, h->win, h->p.blur, h->d_ct[0], h->st));
    s.down(ct, h->d_ct[0], (size_t)h->g.H * h->g.W * sizeof(uint64_t));
    return s.finish();
}

int sgm_stage_cost(sgm_handle *h, const uint64_t *ctl, const uint64_t *ctr, const uint8_t *sky,
                   int view, int filters, float *cost) {
    if (!h || !ctl || !ctr || !cost || (view != 0 && view != 1)) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "stage needs cost volumes (aux_only)");
    const size_t npx = (size_t)h->g.H * h->g.W, nvol = npx * h->g.D;
    Staging s(h);
    s.up(h->d_ct[0], ctl, npx * 8);
    s.up(h->d_ct[1], ctr, npx * 8);
    if (sky) s.up(h->d_sky[0], sky, npx);
    // (min_disp: the view's shift applied to the tables as handed in)
    const sgm::CostSlot slot = sgm::cost_slot(h, 0, view, sky ? h->d_sky[0] : nullptr);
    s.run([&] { return shift_tables(h, &slot, 1, h->st); });
    STAGE_HIP(s, sgm::launch_cost_h(&slot, 1, h->g.W, filters & 1, h->g, h->st));
    const float *res = h->d_ch[0];
    if (filters & 2) {  // the frame's own vfwd, in place when the frames run it so
        s.run([&] { return sgm::vfwd_view(h, 0, res, cost_buf(h, 0), (double)nvol, h->st); });
        res = cost_buf(h, 0);
    }
    s.down(cost, res, nvol * 4);
    return s.finish();
}

int sgm_stage_path(sgm_handle *h, int dir, const float *cost, float *L, float *minL) {
    if (!h || !cost || !L || dir < 0 || dir > 7) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "stage needs cost volumes (aux_only)");
    if (h->plan.paths4 && dir >= SGM_DIR_L5)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_path: a 4-path handle serves L1..L4 only");
    const size_t npx = (size_t)h->g.H * h->g.W, nvol = npx * h->g.D;
    Staging s(h);
    s.up(h->d_c[0], cost, nvol * 4);
    SweepArgs a = sweep_args(h);
    a.cost = h->d_c[0];
    a.acc_out = h->d_s[0];
    a.min_out = h->d_min;
    STAGE_HIP(s, sgm::launch_sweep(dir, sgm::SWEEP_STORE_L, a, h->g, h->st));
    s.down(L, h->d_s[0], nvol * 4);
    if (minL) s.down(minL, h->d_min, npx * 4);
    return s.finish();
}

int sgm_stage_aggregate(sgm_handle *h, const float *cost, uint16_t *disp, float *sub) {
    if (!h || !cost) return SGM_ERR_INVALID_ARG;
    if (h->p.aux_only) return set_err(h, SGM_ERR_INVALID_ARG, "stage needs cost volumes (aux_only)");
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    s.up(h->d_c[0], cost, npx * h->g.D * 4);
    s.run([&] { return stage_aggregate(h, h->st); });
    if (disp) s.down(disp, h->d_disp[0], npx * 2);
    if (sub) s.down(sub, h->d_sub[0], npx * 4);
    return s.finish();
}

int sgm_stage_lr(sgm_handle *h, const float *fl, const float *fr, float *out) {
    if (!h || !fl || !fr || !out) return SGM_ERR_INVALID_ARG;
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    s.up(h->d_sub[0], fl, npx * 4);
    s.up(h->d_sub[1], fr, npx * 4);
    const int W = h->g.W;
    STAGE_HIP(s, sgm::launch_lr(h->d_sub[0], W, h->d_sub[1], W, h->d_out, W, h->p.lr_max_diff, h->gt, h->st));
    s.down(out, h->d_out, npx * 4);
    return s.finish();
}

int sgm_stage_post_filter(sgm_handle *h, float *disp) {
    if (!h || !disp) return SGM_ERR_INVALID_ARG;
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    s.up(h->d_out, disp, npx * 4);
    s.run([&] { return post_filter(h, h->d_out, h->g.W, h->st); });
    s.down(disp, h->d_out, npx * 4);
    if (int rc = s.finish()) return rc;
    // synchronous: a fixed-budget fill that was not proven is this call's error
    return check_frame_err(h);
}

int sgm_stage_lk_refine(sgm_handle *h, const uint8_t *left, const uint8_t *right, int pitch,
                        float *disp) {
    if (!h || !left || !right || !disp || pitch < h->p.width) return SGM_ERR_INVALID_ARG;
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    s.up_rows(h->d_in[0], left, h->p.width, h->p.height, pitch);
    s.up_rows(h->d_in[1], right, h->p.width, h->p.height, pitch);
    s.up(h->d_out, disp, npx * 4);
    s.run([&] { return lk_refine(h, h->d_in[0], h->d_in[1], h->p.width, h->d_out, h->g.W, h->st); });
    s.down(disp, h->d_out, npx * 4);
    return s.finish();
}

int sgm_stage_sky_detect(sgm_handle *h, const uint8_t *img, int pitch, uint8_t *mask) {
    if (!h || !img || !mask || pitch < h->p.width) return SGM_ERR_INVALID_ARG;
    Staging s(h);
    s.up_rows(h->d_in[0], img, h->p.width, h->p.height, pitch);
    s.run([&] { return sgm_sky_detect_device(h, h->d_in[0], h->p.width, h->d_sky[0], h->g.W, h->st); });
    s.down(mask, h->d_sky[0], (size_t)h->g.H * h->g.W);
    return s.finish();
}

int sgm_stage_colormap(sgm_handle *h, const float *disp, uint8_t *bgr) {
    if (!h || !disp || !bgr) return SGM_ERR_INVALID_ARG;
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    // staging: the map in d_out, the BGR image in a stream-ordered temporary
    uint8_t *d_bgr = s.temp<uint8_t>(3 * npx);
    s.up(h->d_out, disp, npx * 4);
    s.run([&] { return sgm_colormap_device(h, h->d_out, h->g.W, d_bgr, 3 * h->g.W, h->st); });
    s.down(bgr, d_bgr, 3 * npx);
    return s.finish();
}

int sgm_stage_point_cloud(sgm_handle *h, const float *disp, const uint8_t *img, int img_pitch,
                          const sgm_camera *cam, double *xyz, uint8_t *pixel, int *count) {
    if (!h || !disp || !img || !cam || !xyz || !pixel || !count || img_pitch < h->g.W)
        return SGM_ERR_INVALID_ARG;
    const size_t npx = (size_t)h->g.H * h->g.W;
    const size_t nimg = (size_t)h->g.H * img_pitch;  // the node reads img(i, j) at working-grid indices
    Staging s(h);
    uint8_t *d_img = s.temp<uint8_t>(nimg), *d_pix = s.temp<uint8_t>(npx);
    double *d_xyz = s.temp<double>(3 * npx);
    int *d_n = s.temp<int>(1);
    s.up(d_img, img, nimg);
    s.up(h->d_out, disp, npx * 4);
    s.run([&] { return sgm_point_cloud_device(h, h->d_out, h->g.W, d_img, img_pitch, cam, d_xyz, d_pix, d_n, h->st); });
    s.down(count, d_n, sizeof(int));
    s.sync();
    const size_t n = s.rc ? 0 : (size_t)*count;  // (it sizes the two downloads; after an error they are skipped)
    s.down(xyz, d_xyz, 3 * n * sizeof(double));
    s.down(pixel, d_pix, n);
    return s.finish();
}

int sgm_stage_confidence(sgm_handle *h, int view, float *ratio) {
    if (!h || !ratio) return SGM_ERR_INVALID_ARG;
    Staging s(h);
    // staged through the post filter's working map (dead between calls)
    s.run([&] { return sgm_confidence_device(h, view, h->d_pf_work, h->g.W, nullptr); });
    s.down(ratio, h->d_pf_work, (size_t)h->g.H * h->g.W * sizeof(float));
    return s.finish();
}

int sgm_stage_confidence_filter(sgm_handle *h, float *disp, const float *ratio, float max_ratio) {
    if (!h || !disp || !ratio) return SGM_ERR_INVALID_ARG;
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    s.up(h->d_out, disp, npx * 4);
    s.up(h->d_pf_work, ratio, npx * 4);
    STAGE_HIP(s, sgm::launch_confidence_filter(h->d_out, h->g.W, h->d_pf_work, h->g.W, max_ratio, h->gt, h->st));
    s.down(disp, h->d_out, npx * 4);
    return s.finish();
}

int sgm_stage_window_cost(sgm_handle *h, int kind, const uint8_t *left, const uint8_t *right, int pitch,
                          float *cost) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (const char *why = sgm::window_cost_refusal(kind, left, right, pitch, h->p.width, cost))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_window_cost: %s", why);
    const size_t nvol = (size_t)h->g.H * h->g.W * h->g.D;
    Staging s(h);
    s.up_rows(h->d_in[0], left, h->p.width, h->p.height, pitch);
    s.up_rows(h->d_in[1], right, h->p.width, h->p.height, pitch);
    // (an aux_only handle has no cost buffer: a temporary of the call's own)
    float *d_cost = s.temp<float>(nvol);
    s.run([&] { return sgm_window_cost_device(h, kind, h->d_in[0], h->d_in[1], h->p.width, d_cost, nullptr); });
    s.down(cost, d_cost, nvol * sizeof(float));
    return s.finish();
}

int sgm_stage_filter_volume(sgm_handle *h, float *cost, int filters) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!cost) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_filter_volume: NULL volume");
    if (h->p.aux_only)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_filter_volume: handle created with aux_only (no cost volumes)");
    const size_t nvol = (size_t)h->g.H * h->g.W * h->g.D;
    Staging s(h);
    s.up(h->d_c[0], cost, nvol * sizeof(float));  // staged in view 0's C
    s.run([&] { return sgm_filter_volume_device(h, h->d_c[0], filters, nullptr); });
    s.down(cost, h->d_c[0], nvol * sizeof(float));
    return s.finish();
}

}  // extern "C"
