// sgm_input.hip -- the input stage's part of the C-ABI (include/sgm_hip.h): the resize (node.cpp:
// 75-76), the rectifying remap and the grey conversion, each as a setter, a _device launch, its host
// round trip and the last frame's image.  The handle's state and its shape
// questions are in sgm_input_stage.h, the frame's one launch in sgm_frame.hip (input_slot).
#include "sgm_handle.h"

#include <new>

using namespace sgm;

namespace {

// Frees the maps and the masks and switches the remap off (the images follow in fit_input_buffers).
void rectify_free_maps(sgm_handle *h) {
    for (int v = 0; v < 2; ++v) {
        dfree(h, &h->d_map[v]);
        std::vector<uint8_t>().swap(h->valid[v]);
    }
    h->in.rc_rows = h->in.rc_cols = 0;
}

// Makes d_rs and d_raw fit the handle's input stage as it stands: on a handle that stages, the two
// full-size grey images the frame's first launch writes and the host API's staging of the two raw
// images at their size and format; else neither.  Buffers that fit already are kept.  On a failed
// allocation every stage is switched off and the handle runs as it did at sgm_create.
int fit_input_buffers(sgm_handle *h) {
    const bool staged = h->in.stages(h->p.aux_only);
    const size_t nfull = (size_t)h->p.height * h->p.width;
    const size_t nraw = h->in.raw_bytes(h->p.height, h->p.width, h->p.aux_only);
    int rc = SGM_OK;
    h->rs_valid = false;
    for (int v = 0; v < 2 && !rc; ++v) {
        if (!staged) dfree(h, &h->d_rs[v]);
        else if (!h->d_rs[v]) rc = dalloc(h, &h->d_rs[v], nfull);
    }
    if (!rc && nraw != h->raw_bytes) {
        for (int v = 0; v < 2; ++v) dfree(h, &h->d_raw[v]);
        h->raw_bytes = 0;
        for (int v = 0; v < 2 && !rc; ++v) rc = dalloc(h, &h->d_raw[v], nraw);
        if (!rc) h->raw_bytes = nraw;
    }
    if (rc) {  // (not a group's rollback: what the handle held before goes too)
        for (int v = 0; v < 2; ++v) {
            dfree(h, &h->d_raw[v]);
            dfree(h, &h->d_rs[v]);
        }
        h->raw_bytes = 0;
        rectify_free_maps(h);
        h->in = InputStage();
    }
    return rc;
}

// The last frame's full-size grey image under each stage's name: its getter and download, the
// setting that switches it on, what the getter says when that is off or no frame has filled it.
struct StageImage {
    const char *get, *stage;
    int InputStage::*on;
    const char *off, *stale;
};
const StageImage kResized = {
    "sgm_get_resized", "sgm_stage_resized", &InputStage::in_rows,
    "sgm_get_resized: no input size is set (sgm_set_input_size)",
    "sgm_get_resized: no frame has run since the input size was set"};
const StageImage kRectified = {
    "sgm_get_rectified", "sgm_stage_rectified", &InputStage::rc_rows,
    "sgm_get_rectified: no maps are set (sgm_set_rectify)",
    "sgm_get_rectified: no frame has run since the maps were set"};
const StageImage kInputGray = {
    "sgm_get_input_gray", "sgm_stage_input_gray", &InputStage::fmt,
    "sgm_get_input_gray: the input format is grey (sgm_set_input_format): the frame reads the caller's images",
    "sgm_get_input_gray: no frame has run since the format was set"};

// sgm_get_*: the device image of `view` and its pitch.
int get_image(sgm_handle *h, const StageImage &t, int view, const uint8_t **d_img, int *pitch) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_img || !pitch) return set_err(h, SGM_ERR_INVALID_ARG, "%s: NULL pointer", t.get);
    if (!(h->in.*t.on)) return set_err(h, SGM_ERR_INVALID_ARG, "%s", t.off);
    // (every frame handle's census reads both images, so the first launch writes both)
    if (view != SGM_VIEW_LEFT && view != SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: the handle reads no image of view %d", t.get, view);
    if (!h->rs_valid) return set_err(h, SGM_ERR_INVALID_ARG, "%s", t.stale);
    *d_img = h->d_rs[view];
    *pitch = h->p.width;
    return SGM_OK;
}

// sgm_stage_*: a host copy of it.
int download_image(sgm_handle *h, const StageImage &t, int view, uint8_t *img) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!img) return set_err(h, SGM_ERR_INVALID_ARG, "%s: NULL pointer", t.stage);
    const uint8_t *d_img = nullptr;
    int pitch = 0;
    if (int rc = get_image(h, t, view, &d_img, &pitch)) return rc;
    Staging s(h);
    s.down(img, d_img, (size_t)h->p.height * h->p.width);
    return s.finish();
}

}  // namespace

extern "C" {

// ---- input resize

int sgm_set_input_size(sgm_handle *h, int src_rows, int src_cols) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!input_size_ok(src_rows, src_cols, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_input_size: %s", why);
    if (h->p.aux_only && src_rows)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_input_size: an aux_only handle runs no frames (sgm_resize_device "
                       "takes its sizes per call)");
    if (h->in.rc_rows && src_rows)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_input_size: rectification maps are set (sgm_set_rectify): one input "
                       "stage at a time, and the remap resizes too");
    if (!input_bytes_ok(h->in.fmt, src_rows, src_cols, h->p.height, h->p.width))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_input_size: image too large: %d x %d at %d bytes per pixel",
                       src_rows, src_cols, h->in.bpp());
    const bool unchanged = src_rows == h->in.in_rows && src_cols == h->in.in_cols;
    return change_setting(h, "sgm_set_input_size", unchanged, [&] {
        h->in.in_rows = src_rows;
        h->in.in_cols = src_cols;
        return fit_input_buffers(h);
    });
}

int sgm_get_input_size(const sgm_handle *h, int *src_rows, int *src_cols) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (src_rows) *src_rows = h->in.in_rows;
    if (src_cols) *src_cols = h->in.in_cols;
    return SGM_OK;
}

int sgm_get_resized(sgm_handle *h, int view, const uint8_t **d_img, int *pitch) {
    return get_image(h, kResized, view, d_img, pitch);
}
int sgm_stage_resized(sgm_handle *h, int view, uint8_t *img) { return download_image(h, kResized, view, img); }

int sgm_resize_device(sgm_handle *h, const uint8_t *d_src, int src_rows, int src_cols, int src_pitch,
                      uint8_t *d_dst, int dst_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!d_src || !d_dst) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_resize_device: NULL pointer");
    if (!resize_src_ok(src_rows, src_cols, src_pitch, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_resize_device: %s", why);
    if (dst_pitch < h->p.width)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_resize_device: dst_pitch %d below the width %d",
                       dst_pitch, h->p.width);
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "resize", (double)h->p.height * h->p.width, st, [&] {
               return sgm::launch_resize(&d_src, src_rows, src_cols, src_pitch, &d_dst, h->p.height,
                                         h->p.width, dst_pitch, 1, st);
           }));
    return SGM_OK;
}

int sgm_stage_resize(sgm_handle *h, const uint8_t *src, int src_rows, int src_cols, int src_pitch,
                     uint8_t *dst) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!src || !dst) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_resize: NULL pointer");
    if (!resize_src_ok(src_rows, src_cols, src_pitch, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_resize: %s", why);
    Staging s(h);  // (the source in a temporary, the result in d_in[0])
    uint8_t *d_src = s.temp<uint8_t>((size_t)src_rows * src_cols);
    s.up_rows(d_src, src, src_cols, src_rows, src_pitch);
    s.run([&] { return sgm_resize_device(h, d_src, src_rows, src_cols, src_cols, h->d_in[0], h->p.width, h->st); });
    s.down(dst, h->d_in[0], (size_t)h->p.height * h->p.width);
    return s.finish();
}

// ---- rectification

int sgm_set_rectify(sgm_handle *h, int src_rows, int src_cols, const float *map_x_l, const float *map_y_l,
                    const float *map_x_r, const float *map_y_r, int map_pitch) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    const float *const maps[4] = {map_x_l, map_y_l, map_x_r, map_y_r};
    if (!rectify_args_ok(src_rows, src_cols, maps, map_pitch, h->p.width, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_rectify: %s", why);
    if (h->in.in_rows && src_rows)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_rectify: an input size is set (sgm_set_input_size): one input stage at "
                       "a time, and the remap resizes too");
    if (!input_bytes_ok(h->in.fmt, src_rows, src_cols, h->p.height, h->p.width))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_rectify: image too large: %d x %d at %d bytes per pixel",
                       src_rows, src_cols, h->in.bpp());
    return change_setting(h, "sgm_set_rectify", !src_rows && !h->in.rc_rows, [&]() -> int {
        rectify_free_maps(h);  // (what an earlier call allocated)
        int rc = fit_input_buffers(h);
        if (rc || !src_rows) return rc;
        const size_t nfull = (size_t)h->p.height * h->p.width;
        std::vector<uint32_t> packed;
        try {
            packed.resize(2 * nfull);
            for (int v = 0; v < 2; ++v) h->valid[v].resize(nfull);
        } catch (const std::bad_alloc &) {
            rc = set_err(h, SGM_ERR_OUT_OF_MEMORY, "sgm_set_rectify: out of host memory");
        }
        Ledger::Group both(h->mem);
        for (int v = 0; v < 2 && !rc; ++v) {
            rectify_convert(maps[2 * v], maps[2 * v + 1], map_pitch, h->p.height, h->p.width, src_rows,
                            src_cols, packed.data(), h->valid[v].data());
            if ((rc = dalloc(h, &h->d_map[v], 2 * nfull))) break;
            if (hipMemcpy(h->d_map[v], packed.data(), 2 * nfull * sizeof(uint32_t), hipMemcpyHostToDevice) !=
                hipSuccess)
                rc = set_err(h, SGM_ERR_HIP, "sgm_set_rectify: the upload of the packed map failed");
        }
        if (rc) {  // (off again: the group frees the maps, and the handle runs as before)
            for (auto &mask : h->valid) std::vector<uint8_t>().swap(mask);
            return rc;
        }
        both.commit();
        // (an aux_only handle runs no frames: it keeps the maps for sgm_remap_device alone)
        h->in.rc_rows = src_rows;
        h->in.rc_cols = src_cols;
        return fit_input_buffers(h);
    });
}

int sgm_get_rectify(const sgm_handle *h, int *src_rows, int *src_cols) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (src_rows) *src_rows = h->in.rc_rows;
    if (src_cols) *src_cols = h->in.rc_cols;
    return SGM_OK;
}

int sgm_remap_device(sgm_handle *h, int view, const uint8_t *d_src, int src_pitch, uint8_t *d_dst,
                     int dst_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!d_src || !d_dst) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_remap_device: NULL pointer");
    if (!h->in.rc_rows)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_remap_device: no maps are set (sgm_set_rectify)");
    if (!rectify_call_ok(view, src_pitch, h->in.rc_cols, dst_pitch, h->p.width, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_remap_device: %s", why);
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "rectify", (double)h->p.height * h->p.width, st, [&] {
               return sgm::launch_rectify(&d_src, h->in.rc_rows, h->in.rc_cols, src_pitch, &h->d_map[view],
                                          &d_dst, h->p.height, h->p.width, dst_pitch, 1, st);
           }));
    return SGM_OK;
}

int sgm_stage_remap(sgm_handle *h, int view, const uint8_t *src, int src_pitch, uint8_t *dst) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!src || !dst) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_remap: NULL pointer");
    if (!h->in.rc_rows)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_remap: no maps are set (sgm_set_rectify)");
    if (!rectify_call_ok(view, src_pitch, h->in.rc_cols, h->p.width, h->p.width, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_remap: %s", why);
    Staging s(h);  // (the source in a temporary, the result in d_in[0])
    uint8_t *d_src = s.temp<uint8_t>((size_t)h->in.rc_rows * h->in.rc_cols);
    s.up_rows(d_src, src, h->in.rc_cols, h->in.rc_rows, src_pitch);
    s.run([&] { return sgm_remap_device(h, view, d_src, h->in.rc_cols, h->d_in[0], h->p.width, h->st); });
    s.down(dst, h->d_in[0], (size_t)h->p.height * h->p.width);
    return s.finish();
}

int sgm_get_rectified(sgm_handle *h, int view, const uint8_t **d_img, int *pitch) {
    return get_image(h, kRectified, view, d_img, pitch);
}
int sgm_stage_rectified(sgm_handle *h, int view, uint8_t *img) { return download_image(h, kRectified, view, img); }

int sgm_stage_rectify_valid(sgm_handle *h, int view, uint8_t *mask) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!mask) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_rectify_valid: NULL pointer");
    if (!h->in.rc_rows)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_rectify_valid: no maps are set (sgm_set_rectify)");
    if (view != SGM_VIEW_LEFT && view != SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_rectify_valid: view must be 0 (left) or 1 (right), got %d",
                       view);
    memcpy(mask, h->valid[view].data(), h->valid[view].size());
    return SGM_OK;
}

// ---- colour input

int sgm_set_input_format(sgm_handle *h, int fmt) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!input_format_ok(fmt, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_input_format: %s", why);
    if (h->p.aux_only && fmt != SGM_PIX_GRAY8)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_input_format: an aux_only handle runs no frames (sgm_gray_device takes "
                       "its format per call)");
    const int rows = h->in.rows(h->p.height), cols = h->in.cols(h->p.width);
    if (!input_bytes_ok(fmt, rows, cols, h->p.height, h->p.width))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_input_format: image too large: %d x %d at %d bytes per pixel",
                       rows, cols, sgm::pix_bpp(fmt));
    return change_setting(h, "sgm_set_input_format", fmt == h->in.fmt, [&] {
        h->in.fmt = fmt;
        return fit_input_buffers(h);
    });
}

int sgm_get_input_format(const sgm_handle *h, int *fmt) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (fmt) *fmt = h->in.fmt;
    return SGM_OK;
}

int sgm_gray_device(sgm_handle *h, int fmt, const uint8_t *d_src, int rows, int cols, int src_pitch,
                    uint8_t *d_dst, int dst_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!d_src || !d_dst) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_gray_device: NULL pointer");
    if (!gray_call_ok(fmt, rows, cols, src_pitch, dst_pitch, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_gray_device: %s", why);
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    hipStream_t st = scope.st;
    HIPCHK(h, timed(h, "gray", (double)rows * cols, st, [&] {
               return sgm::launch_gray(fmt, &d_src, rows, cols, src_pitch, &d_dst, dst_pitch, 1, st);
           }));
    return SGM_OK;
}

int sgm_stage_gray(sgm_handle *h, int fmt, const uint8_t *src, int rows, int cols, int src_pitch,
                   uint8_t *dst) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!src || !dst) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_gray: NULL pointer");
    if (!gray_call_ok(fmt, rows, cols, src_pitch, cols, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_gray: %s", why);
    const size_t row = (size_t)cols * sgm::pix_bpp(fmt);
    Staging s(h);  // (the source and the result, of any size, in temporaries)
    uint8_t *d_src = s.temp<uint8_t>(row * rows), *d_dst = s.temp<uint8_t>((size_t)rows * cols);
    s.up_rows(d_src, src, row, rows, src_pitch);
    s.run([&] { return sgm_gray_device(h, fmt, d_src, rows, cols, (int)row, d_dst, cols, h->st); });
    s.down(dst, d_dst, (size_t)rows * cols);
    return s.finish();
}

int sgm_get_input_gray(sgm_handle *h, int view, const uint8_t **d_img, int *pitch) {
    return get_image(h, kInputGray, view, d_img, pitch);
}
int sgm_stage_input_gray(sgm_handle *h, int view, uint8_t *img) { return download_image(h, kInputGray, view, img); }

}  // extern "C"
