/*
 * sgm_hip.h -- C-ABI of libsgm_hip.so, the MI355X-native semi-global matcher.
 *
 * This library replaces the reference's dormant CUDA backend (gpu_sgm/,
 * class GPU_SGM, gpu_sgm/inc/SGM.cuh:23-62) and the CPU hot path it mirrors
 * (class SGM : Solver, inc/SGM.h:10-26, inc/Solver.h:23-70).  Plain C: plain
 * pointers and sizes, no STL, no OpenCV, no torch types.  The C++ class
 * surface with the reference's signatures (include/sgm_amd/SGM.h) and the
 * Python mirror (stereo_matching_amd/) are thin layers over these entry
 * points; INTEGRATION.md shows how the ROS node binds it.
 *
 * Semantics follow src/SGM.cpp / src/Solver.cpp bit-for-bit:
 * float32 costs, P1=10, P2=100, uniqueness 0.7, LR threshold 1.0, invalid
 * disparity D+1.  The reference's domain d in {32,64,128} (Solver.cpp:10) is
 * widened to 256; raw WTA disparities are therefore uint16 (the reference's
 * uchar would wrap D+1 = 257).
 *
 * Threading: a handle is bound to one device and is not thread-safe (one
 * frame at a time, like the reference object, Solver.h:29-30).  Use one
 * handle per device/thread.
 *
 * Stream arguments: NULL = the handle's own stream, created non-blocking (so
 * NOT ordered with the legacy default stream); hipStreamLegacy ((void *)1)
 * = the legacy default stream; otherwise a hipStream_t.
 *
 * Streams: every call on a handle uses the handle's device scratch (cost
 * volumes, checkpoints, post-filter and LKRefine buffers), so the library
 * orders calls made on different streams: a call whose stream differs from
 * the previous call's first makes its stream wait for the previous call's
 * work.  A call on a caller's stream records an event on that stream as it
 * returns (so the library keeps no caller stream past the call that used
 * it; a rocprof trace shows the record as a ~5 us gap before the next
 * kernel); calls on the handle's own stream (NULL, sgm_get_stream) record
 * nothing.  Device entry points return after
 * enqueueing; with post_filter they do so unless a launch budget is set
 * (sgm_set_post_filter_launches): without one the median fill blocks the
 * calling host thread on an event once per two fill launches to read a
 * convergence counter (sgm_post_filter_device, and sgm_process_device with
 * params.post_filter), so those calls are not fully asynchronous and cannot
 * be captured into a HIP graph; with one they enqueue a fixed number of fill
 * launches, return, and the device's verdict is read by sgm_check.
 */
#ifndef SGM_HIP_H
#define SGM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGM_HIP_VERSION 2  /* 2: sgm_params ends with `paths` */

/* Status codes (the reference only asserts, Solver.cpp:6-10; GPU errors were
 * printed and ignored, gpu_sgm/inc/cuda_inc.cuh:4-9 -- here they are returned). */
enum {
    SGM_OK = 0,
    SGM_ERR_INVALID_ARG = 1,   /* a reference assert would have fired */
    SGM_ERR_OUT_OF_MEMORY = 2,
    SGM_ERR_HIP = 3,           /* HIP runtime error; see sgm_last_error() */
    SGM_ERR_NO_DEVICE = 4
};

/* Path directions, numbered like the reference's L1..L8 (src/SGM.cpp:81-369). */
enum {
    SGM_DIR_L1 = 0, /* left -> right        */
    SGM_DIR_L2 = 1, /* right -> left        */
    SGM_DIR_L3 = 2, /* top -> down          */
    SGM_DIR_L4 = 3, /* down -> top          */
    SGM_DIR_L5 = 4, /* left-top -> right-down  */
    SGM_DIR_L6 = 5, /* right-top -> left-down  */
    SGM_DIR_L7 = 6, /* left-down -> right-top  */
    SGM_DIR_L8 = 7  /* right-down -> left-top  */
};

/* Matching algorithm: the Solver subclasses of the reference (node.cpp:49-50). */
enum {
    SGM_SOLVER_SGM = 0,  /* class SGM (inc/SGM.h:10-26, src/SGM.cpp) */
    SGM_SOLVER_BM = 1    /* class BM (inc/BM.h:6-19, src/BM.cpp): filtered-cost WTA, left view */
};

typedef struct sgm_params {
    int height;        /* input image rows (before decimation)      Solver(h,..) */
    int width;         /* input image cols                           Solver(.,w,..) */
    int scale;         /* 1 or 2: decimation (Solver.cpp:8,12-13; SGM.cpp:40-61) */
    int max_disp;      /* D in {32,64,128,256} (Solver.cpp:10, widened)          */
    int p1;            /* 10  (SGM.cpp:27) */
    int p2;            /* 100 (SGM.cpp:28) */
    float uniqueness;  /* 0.7 UNIQUE_RATIO (inc/Solver.h:14); must exceed 8*(p2+999999)/FLT_MAX
                          (about 2e-32): at or below it the reference's WTA would read the
                          previous pixel's sec_min_d (SGM.cpp:392-408), so sgm_create rejects it */
    float lr_max_diff; /* 1.0 LR_CHECK_DIS (inc/Solver.h:16) */
    int blur;          /* 1: pre-blur as Solver.cpp:124-125 (pinned formula); 0: off */
    int views;         /* 2: left+right views + LR check (SGM.cpp:32-818); 1: left view only */
    int post_filter;   /* 1: sgm_process[_device] output is post_filter()ed on the GPU
                          (Solver.cpp:600-649, what get_disp() returns, SGM.cpp:821);
                          0 (default): the LR-checked map (filtered_disp at SGM.cpp:818) */
    int lk_refine;     /* 1: then LKRefine on the GPU (LKSubPixelImpl.cpp:13-235; the call
                          at SGM.cpp:824 is commented out in the reference); 0 (default) */
    int sky_detect;    /* 1: the sky masks of both views come from SkyAreaDetector::detect
                          run on the GPU over the input images (node.cpp:80-93), replacing
                          any masks passed in; 0 (default): masks as passed (or none).
                          Working grid up to 8192 columns and 4784 rows */
    int solver;        /* SGM_SOLVER_SGM (default) or SGM_SOLVER_BM.  BM: out = the raw
                          WTA disparity as float (BM.cpp:53-85; post_filter()ed when
                          post_filter is set, BM.cpp:88), raw_disp = the same as u16;
                          views, lk_refine and the right sky mask are unused */
    int aux_only;      /* 1: a light handle for the per-frame side stages only (sky detector,
                          post_filter, LKRefine, colormap, point cloud): no cost volumes are
                          allocated and sgm_process[_device] refuse; 0 (default) */
    int view;          /* with views == 1: SGM_VIEW_LEFT (default), the left view
                          (SGM.cpp:32-445, disp/filtered_disp); or SGM_VIEW_RIGHT, the right
                          view alone (SGM.cpp:448-801: build_dsi_from_table_beta, the same
                          8 paths, disp_beta/filtered_disp_beta), so that a pair's two views
                          can run on two GPUs and meet in sgm_lr_check_device.
                          A right-view handle has no post_filter/lk_refine (they follow the
                          LR check on the left view's GPU) and uses sky_r (or the right image's
                          detected mask) */
    int paths;         /* aggregation paths per view: 8 (default; 0 means 8, so zero-initialised
                          structs keep working) or 4, the reference's USE_8_PATH = false
                          (inc/SGM.h:7): SGM.cpp:15,241,387-390,619,765,847 drop L5..L8 and
                          S = ((L1+L2)+L3)+L4 goes straight into WTA, uniqueness, sub-pixel and
                          the LR check.  Any other value: sgm_create returns
                          SGM_ERR_INVALID_ARG.  A 4-path handle holds no diagonal checkpoints,
                          band carries or slanted-tile buffers and always runs whole-volume
                          passes (SGM_SLANT and SGM_BAND_ROWS are ignored).  BM and aux_only
                          handles ignore the field */
} sgm_params;

enum { SGM_VIEW_LEFT = 0, SGM_VIEW_RIGHT = 1 };

/* Camera of the point cloud (CamIntrinsics, inc/utils.h:14-20, plus the two
 * constants of node.cpp:122-123). */
typedef struct sgm_camera {
    float fx, fy, cx, cy;
    double baseline;   /* 0.5 in node.cpp:123 */
    float max_range;   /* 100 in node.cpp:122 */
} sgm_camera;

typedef struct sgm_handle sgm_handle;

/* Fills p with the reference defaults for SGM(h, w, s, d) (node.cpp:49). */
int sgm_default_params(sgm_params *p, int h, int w, int s, int d);

/* Allocates every device buffer up front, as the reference constructors do
 * (Solver.cpp:18-27, SGM.cpp:7-24).  device = HIP ordinal.  Where the
 * slanted-tile schedule is chosen by size (HD/4K at D >= 128) and the device
 * cannot hold its extra buffers (a full L3 volume per view and the hand-off
 * granules, ~80 GB for a 4K256 pair), the handle takes the banded schedule
 * instead (the same maps, bit for bit); with SGM_SLANT=1 the allocation
 * failure is returned. */
int sgm_create(const sgm_params *p, int device, sgm_handle **out);
int sgm_destroy(sgm_handle *h);
const char *sgm_last_error(const sgm_handle *h);
/* Working (decimated) size: rows = height/scale, cols = width/scale. */
int sgm_get_size(const sgm_handle *h, int *rows, int *cols, int *max_disp);
/* ---- minimum disparity: search [m, m + D) instead of [0, D) ----
 *
 * A property of the handle (like sgm_set_confidence; sgm_params and
 * SGM_HIP_VERSION are unchanged), normally set once, right after sgm_create;
 * m = 0 is every handle's default and runs exactly as before (OpenCV SGBM's
 * minDisparity).  With m set, index d of every cost volume stands for
 * disparity m + d: the left view's DSI (Solver.cpp:143-194) reads
 * ctR[i, max(j - (d+m)/s, 0)], the right view's (:197-248)
 * ctL[i, min(j + (d+m)/s, W-1)]; filters, paths, aggregation, WTA,
 * uniqueness, sub-pixel and the confidence quotient run unchanged on those
 * volumes, and every map that leaves the library is in TRUE disparity: sub =
 * index-space value + (float)m (one fp32 add, every pixel), raw = index + m,
 * so the invalid marker is D + m + 1.  The LR check, post_filter, LKRefine,
 * the confidence filter, the colormap and the point cloud (in frames and as
 * device or stage calls on any handle set to the same m, aux_only included)
 * work on such maps as the reference's functions do when called with D + m
 * for D.  The sky override stays in index space: a sky pixel wins index 0
 * and so reports disparity m, not 0.
 * SGM_ERR_INVALID_ARG, with a message, for m < 0, m not a multiple of scale,
 * D + m + 1 > 65535 (the raw u16 map), and any m != 0 on a BM handle (BM has
 * no staged oracle to derive the definition from).  Allocates (m != 0) or
 * frees (m = 0) two shifted census tables, 16 B per pixel together, counted in
 * the handle's device bytes; a frame then runs one small launch more.
 * Synchronises the handle's last work first; call it outside stream capture,
 * and re-capture graphs afterwards. */
int sgm_set_min_disp(sgm_handle *h, int m);
/* The value that marks an invalid pixel in every float map of this handle:
 * max_disp + min_disp + 1 (D + 1 by default, Solver.cpp:21). */
int sgm_get_invalid_disp(const sgm_handle *h, int *invalid);

/* ---- input resize: the node's cv::resize(img, img, Size(w, h)) (node.cpp:75-76) ----
 *
 * cv::resize of an 8-bit one-channel image with the default INTER_LINEAR, in
 * OpenCV's fixed-point form, pinned as DESIGN.md 5j states it (an exact half
 * size is the 2x2 mean (a + b + c + d + 2) >> 2; otherwise 11-bit weights per
 * axis from fx = (float)((dx + 0.5) * scale_x - 0.5), clamped at the borders)
 * and bit-exact against tests/resize_recipe.py.  Parity with a particular
 * OpenCV build is not pinned at this boundary, as for the pre-blur.
 *
 * sgm_resize_device: src (src_rows x src_cols u8, src_pitch bytes) -> dst at the
 * handle's full size (height x width, dst_pitch bytes; padding untouched).  One
 * launch on `stream` (NULL = the handle's stream), no host wait, no allocation:
 * capturable into a HIP graph.  Any handle serves, aux_only included; the source
 * may be any size from 1 x 1.  SGM_ERR_INVALID_ARG, with a message, for a NULL
 * pointer, a size below 1, src_pitch < src_cols or dst_pitch < width. */
int sgm_resize_device(sgm_handle *h, const uint8_t *d_src, int src_rows, int src_cols,
                      int src_pitch, uint8_t *d_dst, int dst_pitch, void *stream);
/* The same with HOST buffers (dst dense, height x width); synchronous. */
int sgm_stage_resize(sgm_handle *h, const uint8_t *src, int src_rows, int src_cols,
                     int src_pitch, uint8_t *dst);

/* The size of the images a frame takes: a property of the handle, like
 * sgm_set_min_disp (sgm_params and SGM_HIP_VERSION are unchanged).  (0, 0) = off
 * (default): frames run exactly as before.  With a size set, sgm_process and
 * sgm_process_device take src_rows x src_cols images (pitch >= src_cols); the
 * frame's first launch resizes both into handle-owned height x width images
 * (every frame handle's census reads both images, one-view and BM handles
 * included), and everything inside the frame reads those: the census, the
 * in-frame sky detector (params.sky_detect), the in-frame LKRefine, the BM
 * solver.  Sky masks passed in stay on the working grid.  The stand-alone
 * stage calls (sgm_lk_refine_device, sgm_sky_detect_device, sgm_stage_census,
 * ...) keep taking full-size images.
 * Allocates (or, at (0, 0), frees) the two resized images and the host API's
 * staging of the raw ones, counted in sgm_device_bytes.  Synchronises the
 * handle's last work first; call it outside stream capture, and re-capture
 * graphs afterwards.  SGM_ERR_INVALID_ARG, with a message, for a negative size,
 * exactly one of the two zero, and a non-zero size on an aux_only handle (it
 * runs no frames). */
int sgm_set_input_size(sgm_handle *h, int src_rows, int src_cols);
int sgm_get_input_size(const sgm_handle *h, int *src_rows, int *src_cols);
/* The last frame's resized image of `view` (SGM_VIEW_LEFT / SGM_VIEW_RIGHT):
 * handle-owned DEVICE memory, height x width u8, *pitch bytes per row; valid
 * until the next frame, sgm_set_input_size or sgm_destroy.  What the node hands
 * to the point cloud (node.cpp:138 reads the resized img_l).  Reads of it are
 * ordered after the frame on the frame's stream only.  SGM_ERR_INVALID_ARG with
 * no input size set, before any frame, for any other view, or a NULL pointer. */
int sgm_get_resized(sgm_handle *h, int view, const uint8_t **d_img, int *pitch);
/* The same image copied to a HOST buffer (height x width, dense); synchronous. */
int sgm_stage_resized(sgm_handle *h, int view, uint8_t *img);

/* ---- rectification: cv::convertMaps + cv::remap of raw camera images ----
 *
 * cv::remap of an 8-bit one-channel image with INTER_LINEAR and BORDER_CONSTANT
 * 0, over maps converted as cv::convertMaps does to OpenCV's fixed-point form
 * (5 fraction bits), pinned as DESIGN.md 5k states it and bit-exact against
 * tests/rectify_recipe.py: per coordinate q = rint(c * 32) clamped to
 * [-32768 * 32, 32767 * 32] (NaN: the lower clamp), x0 = q >> 5, a = q & 31, and
 *   dst = ((32-a)(32-b) S(y0,x0) + a(32-b) S(y0,x0+1) + (32-a)b S(y0+1,x0)
 *          + ab S(y0+1,x0+1) + 512) >> 10,   S = 0 outside the source, per tap.
 * Parity with a particular OpenCV build is not pinned at this boundary, as for
 * the pre-blur and the resize.
 *
 * sgm_set_rectify: a property of the handle, like sgm_set_input_size
 * (sgm_params and SGM_HIP_VERSION are unchanged).  Takes each view's HOST float
 * maps as cv::initUndistortRectifyMap(..., CV_32FC1, ...) returns them, at the
 * handle's full size (height x width, map_pitch floats per row): map_x[i, j],
 * map_y[i, j] is the position in the src_rows x src_cols source that
 * destination pixel (i, j) samples.  The source may be any size in [1, 32767]
 * per axis, so the remap also does the resize; non-finite and huge coordinates
 * give 0 pixels.  Converts the maps once on the host, uploads them packed (8
 * bytes per pixel and view, counted in sgm_device_bytes) and keeps the valid
 * masks.  (0, 0) with four NULL maps = off (default): everything is freed and
 * frames run exactly as before.  Calling it again replaces the maps.
 * With maps set, sgm_process and sgm_process_device take src_rows x src_cols
 * images (pitch >= src_cols; a side-by-side frame splits by pitch: left = frame,
 * right = frame + cols, pitch = 2 cols).  The frame's first launch remaps both
 * into handle-owned height x width images (one-view and BM handles need both
 * views' maps too: every frame handle's census reads both images), and
 * everything inside the frame reads those: the census, the in-frame sky
 * detector, the in-frame LKRefine, the BM solver.  Sky masks passed in stay on
 * the working grid; the stand-alone stage calls keep taking full-size images.
 * An aux_only handle may hold maps (for sgm_remap_device) but runs no frames.
 * Synchronises the handle's last work first; call it outside stream capture,
 * and re-capture graphs afterwards.  SGM_ERR_INVALID_ARG, with a message, for a
 * size outside [1, 32767] (other than the all-off form), exactly one of the two
 * zero, a NULL map with a non-zero size, map_pitch < width, and a non-zero size
 * while an input size is set (sgm_set_input_size refuses a non-zero size while
 * maps are set: one input stage at a time). */
int sgm_set_rectify(sgm_handle *h, int src_rows, int src_cols, const float *map_x_l,
                    const float *map_y_l, const float *map_x_r, const float *map_y_r,
                    int map_pitch);
int sgm_get_rectify(const sgm_handle *h, int *src_rows, int *src_cols);
/* Remaps `view`'s (SGM_VIEW_LEFT / SGM_VIEW_RIGHT) source image (src_rows x
 * src_cols u8 DEVICE memory, src_pitch bytes) into dst (height x width,
 * dst_pitch bytes; padding untouched).  One launch on `stream` (NULL = the
 * handle's stream), no host wait, no allocation: capturable into a HIP graph.
 * Any handle with maps set serves, aux_only included.  SGM_ERR_INVALID_ARG,
 * with a message, for a NULL pointer, no maps set, a view other than 0 or 1,
 * src_pitch < src_cols or dst_pitch < width. */
int sgm_remap_device(sgm_handle *h, int view, const uint8_t *d_src, int src_pitch,
                     uint8_t *d_dst, int dst_pitch, void *stream);
/* The same with HOST buffers (dst dense, height x width); synchronous. */
int sgm_stage_remap(sgm_handle *h, int view, const uint8_t *src, int src_pitch, uint8_t *dst);
/* The last frame's rectified image of `view`: handle-owned DEVICE memory,
 * height x width u8, *pitch bytes per row; valid until the next frame,
 * sgm_set_rectify or sgm_destroy.  What the point cloud reads.  Reads of it are
 * ordered after the frame on the frame's stream only.  SGM_ERR_INVALID_ARG with
 * no maps set, before any frame, for any other view, or a NULL pointer. */
int sgm_get_rectified(sgm_handle *h, int view, const uint8_t **d_img, int *pitch);
/* The same image copied to a HOST buffer (height x width, dense); synchronous. */
int sgm_stage_rectified(sgm_handle *h, int view, uint8_t *img);
/* `view`'s valid mask, to a HOST buffer (height x width, dense): 255 where all
 * four taps of the pixel lie inside the source, else 0 -- the per-pixel form of
 * stereoRectify's validPixROI.  Built on the host when the maps are set. */
int sgm_stage_rectify_valid(sgm_handle *h, int view, uint8_t *mask);

/* ---- colour input: the decoder's / cvtColor's grey conversion on the GPU ----
 *
 * The reference reads its images with imread(..., IMREAD_GRAYSCALE)
 * (node.cpp:69-70); a colour camera delivers bgr8, rgb8, bgra8 or rgba8.  For
 * 8-bit pixels, pinned as DESIGN.md 5l states it and bit-exact against
 * tests/gray_recipe.py:
 *   Y = (4899 R + 9617 G + 1868 B + 8192) >> 14
 * the fixed-point form of OpenCV 2.4.13's cvtColor(BGR2GRAY) and of its
 * decoder's grey conversion (0.299, 0.587, 0.114 at 14 bits, summing to 16384:
 * R = G = B = v gives v; pure red 76, green 150, blue 29; always in [0, 255]).
 * The alpha byte of a 4-channel format is ignored.  Later OpenCV releases use
 * 15-bit coefficients: parity with a particular OpenCV build is not pinned at
 * this boundary, as for the pre-blur, the resize and the remap.
 * Channels are interleaved, 1, 3 or 4 bytes per pixel; pitches stay in bytes. */
enum {
    SGM_PIX_GRAY8 = 0,
    SGM_PIX_BGR8 = 1,
    SGM_PIX_RGB8 = 2,
    SGM_PIX_BGRA8 = 3,
    SGM_PIX_RGBA8 = 4
};

/* The pixel format of the images a frame takes: a property of the handle, like
 * sgm_set_input_size and sgm_set_rectify (sgm_params and SGM_HIP_VERSION are
 * unchanged).  SGM_PIX_GRAY8 = off (default): frames run exactly as before.
 * With a colour format set, sgm_process and sgm_process_device take colour
 * images of the size the handle's frames take (the full size, the input size or
 * the maps' source size), pitch >= cols x bytes per pixel; a side-by-side frame
 * still splits by pitch (right = left + cols x bytes per pixel).  The format may
 * be set before or after sgm_set_input_size / sgm_set_rectify.  The frame's
 * first launch then writes handle-owned height x width grey images: with an
 * input size or maps set it is the same one resize or remap launch, which
 * converts each tap as it reads it (bit-equal to converting first); with
 * neither it is one conversion launch more.  Everything inside the frame reads
 * those images: the census, the in-frame sky detector, the in-frame LKRefine,
 * the BM solver.  Sky masks and the stand-alone stage calls (sgm_resize_device,
 * sgm_remap_device, sgm_stage_*, ...) stay one-channel.
 * Allocates and frees what the format needs -- the two grey images when no
 * input stage holds them already, the host API's staging of the raw images at
 * cols x bytes per pixel -- counted in sgm_device_bytes.  Synchronises the
 * handle's last work first; call it outside stream capture, and re-capture
 * graphs afterwards.  SGM_ERR_INVALID_ARG, with a message, for an unknown
 * format and for a colour format on an aux_only handle (it runs no frames); a
 * refused call changes nothing. */
int sgm_set_input_format(sgm_handle *h, int fmt);
int sgm_get_input_format(const sgm_handle *h, int *fmt);
/* Converts src (rows x cols pixels of the colour format fmt, DEVICE memory,
 * src_pitch bytes) into dst (rows x cols u8, dst_pitch bytes; padding
 * untouched).  Pointers and pitches may have any alignment.  One launch on
 * `stream` (NULL = the handle's stream), no host wait, no allocation:
 * capturable into a HIP graph.  Any handle serves, aux_only included; the size
 * is the call's own, from 1 x 1.  SGM_ERR_INVALID_ARG, with a message, for a
 * NULL pointer, a size below 1, SGM_PIX_GRAY8 or an unknown format, src_pitch <
 * cols x bytes per pixel or dst_pitch < cols. */
int sgm_gray_device(sgm_handle *h, int fmt, const uint8_t *d_src, int rows, int cols,
                    int src_pitch, uint8_t *d_dst, int dst_pitch, void *stream);
/* The same with HOST buffers (dst dense, rows x cols); synchronous. */
int sgm_stage_gray(sgm_handle *h, int fmt, const uint8_t *src, int rows, int cols, int src_pitch,
                   uint8_t *dst);
/* The last frame's grey image of `view` (SGM_VIEW_LEFT / SGM_VIEW_RIGHT) on a
 * handle with a colour format: handle-owned DEVICE memory, height x width u8,
 * *pitch bytes per row; valid until the next frame, a change of the format or
 * of an input stage, or sgm_destroy.  What the node hands to the point cloud
 * and to show_disp.  With an input stage set it is the buffer sgm_get_resized /
 * sgm_get_rectified return (they keep working).  Reads of it are ordered after
 * the frame on the frame's stream only.  SGM_ERR_INVALID_ARG for a grey handle,
 * before any frame, for any other view, or a NULL pointer. */
int sgm_get_input_gray(sgm_handle *h, int view, const uint8_t **d_img, int *pitch);
/* The same image copied to a HOST buffer (height x width, dense); synchronous. */
int sgm_stage_input_gray(sgm_handle *h, int view, uint8_t *img);

/* ---- reprojection: the disparity map through stereoRectify's Q, on the GPU ----
 *
 * What cv::reprojectImageTo3D, stereo_image_proc and depth consumers work on:
 * an organized float32 XYZ image on the pixel grid and a depth image, float32
 * or 16-bit (ROS REP 118's millimetres), from the frame's final map.  Pinned as
 * DESIGN.md 5m states it and bit-exact against tests/reproject_recipe.py.  Q is
 * 16 doubles, row-major; for working-grid pixel (i, j) of a handle with scale s,
 * x = (double)(j * s), y = (double)(i * s) (node.cpp:133-134), d =
 * (double)disp[i, j] (true disparity, as every map that leaves the library):
 *   X' = ((q0 x + q1 y) + q2 d) + q3      Y' = ((q4 x + q5 y) + q6 d) + q7
 *   Z' = ((q8 x + q9 y) + q10 d) + q11    W' = ((q12 x + q13 y) + q14 d) + q15
 *   iW = 1.0 / W',  X = (float)(X' iW),  Y = (float)(Y' iW),  Z = (float)(Z' iW)
 * each one IEEE double operation in the order written (no FMA, a correctly
 * rounded division, conversions to nearest): OpenCV's reprojectImageTo3D
 * arithmetic without its running sum along the row.  Parity with a particular
 * OpenCV build is not pinned at this boundary, as for the pre-blur, the resize,
 * the remap and the grey conversion.  A pixel is MISSING when disp[i, j] ==
 * (float)(D + min_disp + 1) (sgm_get_invalid_disp; node.cpp:129's exact
 * compare), or W' == 0.0, or max_range > 0 and not (0 < Z && Z <= max_range)
 * (fp32 compares on the rounded Z; max_range == 0: no range test).
 *   xyz     rows x cols x 3 f32, interleaved (CV_32FC3); missing: three times
 *           the bit pattern 0x7FC00000 (a quiet NaN)
 *   depth   rows x cols f32 = Z; missing: 0x7FC00000
 *   depth16 rows x cols u16: r = rintf(Z * depth_scale) (one fp32 multiply,
 *           ties to even) when 1 <= r <= 65535, else 0; missing: 0.
 *           depth_scale = 1000 gives millimetres when Q is in metres
 * A pixel whose W' is subnormal (iW overflows) is not pinned. */
enum { SGM_REPROJECT_XYZ = 1, SGM_REPROJECT_DEPTH = 2, SGM_REPROJECT_DEPTH16 = 4 };
typedef struct sgm_reproject {
    double q[16];        /* row-major Q */
    int outputs;         /* OR of the three bits: what a frame produces */
    float max_range;     /* 0 = no range test */
    float depth_scale;   /* depth16 = rint(Z * depth_scale) */
} sgm_reproject;

/* Reprojection is a property of the handle, like sgm_set_min_disp and
 * sgm_set_rectify (sgm_params and SGM_HIP_VERSION are unchanged).  NULL = off
 * (default): frames enqueue exactly the launches they did before.  With it set,
 * sgm_process and sgm_process_device end with one launch more, on the frame's
 * stream, after the frame's last map stage (the LR check, post_filter or
 * LKRefine; a BM handle's own last stage): it reads the frame's output map and
 * writes the products named in `outputs` into handle-owned buffers
 * (sgm_get_reprojected).  No host wait and no allocation: a frame with a fill
 * budget still captures into a HIP graph.  Allocates the products named in
 * `outputs` (12, 4 and 2 bytes per working-grid pixel), counted in
 * sgm_device_bytes; off frees them.  outputs == 0 is allowed on an aux_only
 * handle only: it runs no frames, holds Q for sgm_reproject_device and allocates
 * nothing (whatever `outputs` says).  Synchronises the handle's last work
 * first; call it outside stream capture, and re-capture graphs afterwards.
 * SGM_ERR_INVALID_ARG, with a message, for a non-finite q, unknown bits in
 * outputs, outputs == 0 on a handle that is not aux_only, a negative or
 * non-finite max_range, depth_scale not finite or <= 0 when DEPTH16 is asked
 * for, and a SGM_VIEW_RIGHT handle (Q belongs to the left camera); a refused
 * call changes nothing. */
int sgm_set_reproject(sgm_handle *h, const sgm_reproject *r);
/* r->outputs == 0 (and everything else 0) when off. */
int sgm_get_reproject(const sgm_handle *h, sgm_reproject *r);
/* The same launch on the caller's DEVICE buffers: d_disp a working-grid map
 * (rows x cols f32, pitch in floats); a NULL product pointer skips that
 * product; max_range and depth_scale come from the setter.  Pitches are in
 * elements of each product's type (xyz_pitch >= 3 * cols); padding is untouched;
 * pointers of any alignment their type allows are accepted.  One launch on
 * `stream` (NULL = the handle's stream), no host wait, no allocation:
 * capturable.  Any handle of the working size with Q set serves, aux_only
 * included.  SGM_ERR_INVALID_ARG, with a message, for no Q set, a NULL map, all
 * three products NULL, or a pitch too small. */
int sgm_reproject_device(sgm_handle *h, const float *d_disp, int pitch,
                         float *d_xyz, int xyz_pitch, float *d_depth, int depth_pitch,
                         uint16_t *d_depth16, int depth16_pitch, void *stream);
/* The same with HOST buffers (all dense; NULL products skipped); synchronous. */
int sgm_stage_reproject(sgm_handle *h, const float *disp, float *xyz, float *depth, uint16_t *depth16);
/* The last frame's product `which` (one SGM_REPROJECT_* bit): handle-owned
 * DEVICE memory, *pitch in elements of its type (3 * cols for XYZ, else cols);
 * valid until the next frame, sgm_set_reproject or sgm_destroy.  Reads of it
 * are ordered after the frame on the frame's stream only.
 * SGM_ERR_INVALID_ARG before any frame, for a product not in `outputs`, or a
 * NULL pointer. */
int sgm_get_reprojected(sgm_handle *h, int which, const void **d_img, int *pitch);
/* The same product copied to a HOST buffer (dense); synchronous. */
int sgm_stage_reprojected(sgm_handle *h, int which, void *img);
/* The pinhole Q of a camera, row-major:
 *   [1 0 0 -cx] [0 1 0 -cy] [0 0 0 f] [0 0 1/baseline 0],  f = ((double)fx + fy) / 2
 * so Z = f * baseline / d.  This is NOT the node's cloud (sgm_point_cloud_device,
 * node.cpp:119-143): one focal length for X and Y, and no 1e-6 added to the
 * disparity.  cam->max_range is not used (the range is sgm_reproject's).
 * SGM_ERR_INVALID_ARG for a NULL pointer, a zero baseline or a non-finite
 * field. */
int sgm_camera_q(const sgm_camera *cam, double q[16]);

/* ---- occlusion-aware hole filling ----
 * A dense map from the frame's final one: the last step of the SGM paper
 * (Hirschmueller 2008, 2.6).  Every invalid pixel (not <= max_disp + min_disp
 * - 1; a NaN counts as invalid) takes one of the up to 8 values its rays find,
 * the first valid pixel of the INPUT map in each of the 8 directions, sorted
 * ascending: an occlusion the second lowest (the background; the lowest of one),
 * a mismatch the upper median sorted[k / 2].  A pixel (i, j) is a mismatch iff
 * some integer d in [min_disp, min_disp + max_disp) has jr = j - d / scale >= 0,
 * the right view's map valid at (i, jr) and |R(i, jr) - d| <= lr_max_diff (the
 * handle's LR tolerance); else an occlusion.  SGM_FILL_BACKGROUND treats every
 * invalid pixel as an occlusion and reads no right map.  A pixel no ray serves
 * stays max_disp + min_disp + 1.  Beside the map a uint8 fill mask:
 *   0 measured, 1 filled as occlusion, 2 filled as mismatch, 3 still invalid.
 * Two launches, no host wait, capturable; the results equal
 * tests/fill_recipe.py bit for bit. */
enum { SGM_FILL_OFF = 0, SGM_FILL_BACKGROUND = 1, SGM_FILL_INTERPOLATE = 2 };
/* A property of the handle (like sgm_set_confidence; sgm_params and
 * SGM_HIP_VERSION are unchanged): with a mode set, every later frame
 * (sgm_process[_device] of any cost and schedule, BM frames, and
 * sgm_aggregate_device) fills its map as its last map stage, after post_filter
 * and LKRefine and before the reprojection, which then reads the dense map.
 * SGM_FILL_INTERPOLATE needs a two-view SGM handle (its right map is the
 * frame's own); one-view left and BM handles serve SGM_FILL_BACKGROUND; an
 * aux_only handle runs no frames and takes either mode for the scratch of
 * sgm_fill_device; a SGM_VIEW_RIGHT handle refuses any mode but off.  Setting a
 * mode allocates 25 bytes per pixel (six candidate planes and the mask),
 * SGM_FILL_OFF frees them; a handle with fill off enqueues exactly the launches
 * it did.  Waits for the handle's work; SGM_ERR_INVALID_ARG inside stream
 * capture, for an unknown mode and for the combinations above.  Re-capture
 * graphs afterwards. */
int sgm_set_fill(sgm_handle *h, int mode);
int sgm_get_fill(const sgm_handle *h, int *mode);
/* The fill in place on a DEVICE map of rows x cols true disparities (pitch in
 * floats), on any handle whose fill scratch exists (sgm_set_fill), with the
 * handle's min_disp and lr_max_diff.  mode: SGM_FILL_BACKGROUND or
 * SGM_FILL_INTERPOLATE, whatever the handle's own.  d_right: the right view's
 * row-major map (right_pitch floats per row; SGM_FILL_INTERPOLATE only, and not
 * d_disp); NULL means this handle's last frame's right view, which only a
 * two-view SGM handle keeps.  d_mask: the fill mask's destination (mask_pitch
 * bytes per row), or NULL for the handle's own (sgm_get_fill_mask).  Two
 * launches on `stream` (NULL: the handle's own; hipStreamLegacy is refused, as
 * by the volume calls), enqueue only. */
int sgm_fill_device(sgm_handle *h, float *d_disp, int pitch, const float *d_right, int right_pitch,
                    int mode, uint8_t *d_mask, int mask_pitch, void *stream);
/* The same with HOST arrays (dense; right and mask may be NULL); synchronous. */
int sgm_stage_fill(sgm_handle *h, float *disp, const float *right, int mode, uint8_t *mask);
/* The fill mask of the last filled frame (or sgm_fill_device call with d_mask
 * NULL): handle-owned DEVICE memory, *pitch in bytes; valid until the next
 * fill, sgm_set_fill or sgm_destroy.  SGM_ERR_INVALID_ARG before any fill. */
int sgm_get_fill_mask(sgm_handle *h, const uint8_t **d_mask, int *pitch);
/* The same mask copied to a HOST buffer (dense); synchronous. */
int sgm_stage_fill_mask(sgm_handle *h, uint8_t *mask);

/* Bytes of device memory the handle holds. */
size_t sgm_device_bytes(const sgm_handle *h);
/* The handle's own stream (a hipStream_t; what a NULL stream argument
 * means), valid until sgm_destroy; NULL for a NULL handle.  A caller that
 * runs its own work around the handle's calls can enqueue it on this stream
 * (e.g. as torch.cuda.ExternalStream) and pass NULL: calls on the handle's
 * stream record no events, while a call on a caller's stream records one as
 * it returns (see "Streams" above). */
void *sgm_get_stream(const sgm_handle *h);

/*
 * SGM::process(l, r, sky, sky_beta) (src/SGM.cpp:32-826, :829-834) up to and
 * including the LR check, on HOST buffers; synchronous.
 *   left/right : u8, height x width, row pitch in bytes
 *   sky_l/sky_r: u8 masks on the working grid (rows x cols), 255 = sky; may be
 *                NULL (Solver.cpp:146)
 *   out        : f32 rows x cols, LR-checked sub-pixel disparity
 *                (filtered_disp after SGM.cpp:818), invalid = D+1 (true
 *                disparity and D + min_disp + 1 with a minimum disparity set); with
 *                params.post_filter it is then post_filter()ed on the GPU
 *                (SGM.cpp:821, what get_disp() returns); with views == 1 it
 *                is the left sub-pixel map (SGM.cpp:443), or the right one
 *                (filtered_disp_beta, SGM.cpp:801) with params.view == SGM_VIEW_RIGHT
 *   raw_disp   : optional u16 rows x cols, left WTA disparity (SGM.cpp:411-415;
 *                disp_beta, SGM.cpp:755-795, with SGM_VIEW_RIGHT)
 */
int sgm_process(sgm_handle *h, const uint8_t *left, const uint8_t *right, int pitch,
                const uint8_t *sky_l, const uint8_t *sky_r, int sky_pitch,
                float *out, int out_pitch, uint16_t *raw_disp);

/* Same on DEVICE buffers, enqueued on `stream` (a hipStream_t; NULL = the
 * handle's own stream).  Returns after enqueueing; the caller synchronises.
 * With params.post_filter and no launch budget (sgm_set_post_filter_launches)
 * the call synchronises `stream` during the median fill's convergence test
 * (sgm_post_filter_device).
 * Volumes above the Infinity Cache may run the slanted-tile passes
 * (DESIGN.md 5e), whose tile-to-tile hand-offs poll with a bounded spin: a
 * frame in which a poll gave up (seconds without progress: a hung or
 * preempted neighbour; later polls of that launch then skip their wait) has
 * invalid maps.  sgm_check() reports it once the frame's work is done; the
 * NEXT sgm_process_device / sgm_process call on the handle also returns
 * SGM_ERR_HIP for it (sgm_process checks right after its own frame). */
int sgm_process_device(sgm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                       const uint8_t *d_sky_l, const uint8_t *d_sky_r, int sky_pitch,
                       float *d_out, int out_pitch, uint16_t *d_raw_disp, void *stream);

/* ---- a caller's cost volume: learned costs in, maps out ----
 *
 * For matching costs the library does not build itself (a network's, AD/SAD/MI,
 * a census of another window): sgm_volume describes the LEFT view's cost volume
 * on the working grid, in DEVICE memory.  Element (i, j, d), i < rows, j < cols,
 * d < D, is at d_cost[i * stride_row + j * stride_col + d * stride_disp]
 * (strides in ELEMENTS); index d stands for disparity min_disp + d.  Exactly
 * one of stride_disp == 1 ("HWD", the library's own layout) and stride_col == 1
 * ("DHW", torch's [D, H, W]) must hold; the other two strides may be anything
 * non-negative that keeps every element at its own address (padded rows and
 * planes, one item of a [B, D, H, W] batch): sorted by stride, each stride is at
 * least the previous stride times the previous extent.  d_cost is aligned to
 * its element type; 16-byte accesses are used wherever an address allows.
 * Costs are finite and in [0, 999999] (the reference's largest cost,
 * Solver.cpp:176; sgm_create's uniqueness bound rests on it).  Values outside
 * that range, NaN and Inf are not checked: the maps are then not pinned, but no
 * address depends on a cost, so memory safety is unaffected. */
enum { SGM_VOL_F32 = 0, SGM_VOL_F16 = 1 };
typedef struct sgm_volume {
    const void *d_cost;          /* DEVICE memory */
    int dtype;                   /* SGM_VOL_F32 | SGM_VOL_F16 (IEEE binary16) */
    long long stride_row, stride_col, stride_disp;   /* in ELEMENTS */
} sgm_volume;

/* Writes the dense fp32 rows x cols x D HWD volume of `view` into d_dst.
 * SGM_VIEW_LEFT: the re-layout, bit for bit (f16 to f32 is exact).
 * SGM_VIEW_RIGHT: the right view's volume derived from the left one,
 *   C_R[i, j, d] = C_L[i, min(j + (d + min_disp) / scale, cols - 1), d]
 * (integer division): build_dsi_from_table_beta's own column index
 * (Solver.cpp:239, with sgm_set_min_disp's shift).  Where that index is not
 * clamped this is an identity of the reference's raw DSIs (ham(ctL[j + k],
 * ctR[j]) is the left DSI at column j + k).  In the clamped columns (j + (d +
 * min_disp) / scale > cols - 1) it DIFFERS from the reference, which compares
 * ctL[cols - 1] with ctR[j] there: a caller's volume holds no such cost, and
 * the left volume's last column is the only choice it allows.
 * One launch on `stream` (NULL = the handle's stream), no host wait, no
 * allocation: capturable into a HIP graph.  Any handle of the working size
 * serves, aux_only included (its min_disp is the one used).  d_dst must not
 * overlap the source (not checked).  SGM_ERR_INVALID_ARG, with a message, for a
 * NULL pointer, a bad dtype or view, strides outside the rule above, or
 * hipStreamLegacy as the stream.
 * The legacy default stream is NOT accepted by this call and by
 * sgm_aggregate_device (unlike the entry points above): a call on a caller's
 * stream records its end there, and the next call on another stream waits on
 * that event; with the event recorded on hipStreamLegacy that wait crashed the
 * host process under PyTorch's HIP runtime (seen once, after a call on the
 * legacy stream followed by sgm_stage_confidence; the runtime-side reason is
 * not established).  Work on the legacy stream is ordered with these calls by
 * an event of the caller's: record it there, make a created stream (or the
 * handle's own, sgm_get_stream) wait for it, and pass that stream. */
int sgm_volume_import_device(sgm_handle *h, const sgm_volume *vol, int view, float *d_dst, void *stream);

/* The frame from the cost volume on: imports vol into the handle's own cost
 * buffer(s) (one launch writes both views' volumes on a views == 2 handle),
 * runs the aggregation sgm_stage_aggregate runs (the L3 checkpoints from the
 * final volume, then the whole-volume 8-path passes, or the 4-path passes on a
 * paths == 4 handle; with two views, view after view), then exactly what a
 * frame does after its aggregation: the LR check (views == 2) into d_out,
 * post_filter with params.post_filter (adaptive, or with a launch budget), the
 * reprojection launch with sgm_set_reproject, the confidence maps with
 * sgm_set_confidence.  Maps leave in true disparity (+ min_disp); d_raw is the
 * left raw WTA map or NULL.  The sky override and the census are the caller's
 * business: masks, sky_detect and blur play no part.  The reference's two cost
 * filters run on each view's volume after the import when the handle is set to
 * (sgm_set_volume_filter, below; off by default: the volume is then aggregated
 * as it comes).
 * Works on handles of every schedule (the aggregation itself always takes the
 * whole-volume passes, whose buffers every frame handle holds: no call
 * allocates).  It waits for nothing on the host given a fill budget or no post
 * filter, and can then be captured into and replayed from a HIP graph; call it
 * once eagerly before capturing, as for frames.  Stream ordering, the event
 * record and sgm_check behave as for sgm_process_device.  The import is timed
 * under the profile class "vol_import".
 * SGM_ERR_INVALID_ARG, with a message and nothing enqueued, for NULL pointers,
 * a bad dtype, strides outside the rule above, hipStreamLegacy as the stream
 * (see sgm_volume_import_device), out_pitch < cols, BM handles,
 * aux_only handles, SGM_VIEW_RIGHT handles, and handles with params.lk_refine
 * (LKRefine needs images: run sgm_lk_refine_device afterwards). */
int sgm_aggregate_device(sgm_handle *h, const sgm_volume *vol, float *d_out, int out_pitch,
                         uint16_t *d_raw, void *stream);

/* ---- the matching cost of a frame: census, or a SAD / SSD / CT window ----
 *
 * The reference's second way to build the disparity space image,
 * Solver::build_dsi (Solver.cpp:96-117) over the window costs SAD and SSD
 * (cost.cpp:4-59), on the GPU.  On the working grid (rows = h / scale, cols =
 * w / scale), with L and R the frame's grey images after its input slot,
 * decimated by scale as the census reads them and NOT blurred (build_dsi reads
 * img_l and img_r; params.blur plays no part), win_h = 7 / scale and win_w =
 * 9 / scale (integer division):
 *   AD(y, x, d)   = |L[y][x] - R[y][max(x - (d + min_disp) / scale, 0)]|   (SSD: its square)
 *   C_L[i][j][d]  = (sum over a = -win_h/2 .. win_h/2, b = -win_w/2 .. win_w/2 of
 *                    AD(clamp(i + a, 0, rows - 1), clamp(j + b, 0, cols - 1), d)) / win_h / win_w
 * The sum is an integer (at most 63 * 255^2); two correctly rounded fp32
 * divisions follow, in that order.  At scale 2 the loops run over 3 x 5 taps and
 * divide by 3 and 4, as the reference's do.  The largest cost is 65025.
 * WEIGHTED_COST (0 in the reference, inc/Solver.h:15) is the handle setting
 * sgm_set_weighted below; an ensemble with the census (no formula in the
 * reference) is not built.
 *
 * SGM_COST_CT is CT (cost.cpp:62-96), the function build_dsi
 * actually calls (Solver.cpp:110): a census per pixel and per disparity on the
 * same unblurred images and the same window.  With disp = d + min_disp and
 * k = disp / scale (integer division):
 *   cl = L[i][j],  cr = R[i][max(j - disp, 0)]        (disp, not k: cost.cpp:69 as written)
 *   C_L[i][j][d] = the number of taps (a, b) != (0, 0) -- on a weighted handle
 *                  only those of sgm_set_weighted's disc -- with
 *                  y = clamp(i + a, 0, rows - 1), x_l = clamp(j + b, 0, cols - 1),
 *                  x_r = x_l - k >= 0 (a tap with x_r < 0 is skipped, not clamped)
 *                  at which (L[y][x_l] > cl) != (R[y][x_r] > cr)
 * an integer in [0, 62], stored as a float.  It is not the Hamming distance of
 * two census tables: the right window follows the left one's clamped columns,
 * taps off the left edge are skipped and the right centre is clamped on its own.
 * At scale 2 the centre column uses disp while the taps use disp / 2; that is
 * the reference's text, reproduced as it stands: the volume is what its
 * compiled CT returns with `scale` passed (build_dsi itself passes none).
 * The value 3 is no kind and stays refused. */
enum { SGM_COST_CENSUS = 0, SGM_COST_SAD = 1, SGM_COST_SSD = 2, SGM_COST_CT = 4 };

/* The cost every later frame of the handle matches on.  SGM_COST_CENSUS is
 * every handle's default and runs exactly as before.  A property of the handle
 * (like sgm_set_min_disp; sgm_params and SGM_HIP_VERSION are unchanged); it
 * allocates nothing and waits for nothing; re-capture graphs afterwards.
 * A frame on a SAD, SSD or CT handle runs its input slot as before, then one launch
 * writes C_L into the handle's left cost buffer; with views == 2 the right
 * view's volume is derived from it by sgm_volume_import_device's rule,
 *   C_R[i, j, d] = C_L[i, min(j + (d + min_disp) / scale, cols - 1), d];
 * then comes what sgm_aggregate_device does after its import: the L3
 * checkpoints from the final volume, the whole-volume 8-path (or 4-path) passes
 * on every handle whatever its schedule, the LR check, post_filter, confidence
 * and reprojection; and LKRefine with params.lk_refine (the frame has images).
 * The 5 x 3 cost filters are not applied by default (the window sum is a box
 * aggregation already); with sgm_set_volume_filter (below) they run on each
 * view's volume after the right view's derivation, which makes the frame
 * SGM::process with build_dsi() in the place of the census DSI (SGM.cpp:66-72).
 * Sky masks have no meaning in build_dsi, so a frame call with a non-NULL mask
 * on such a handle returns SGM_ERR_INVALID_ARG.
 * SGM_ERR_INVALID_ARG, with a message, for a kind that is none of the four,
 * and for BM, aux_only, SGM_VIEW_RIGHT and sky_detect handles. */
int sgm_set_cost(sgm_handle *h, int kind);
int sgm_get_cost(const sgm_handle *h, int *kind);

/* The producer alone: the dense fp32 rows x cols x D (HWD) left volume C_L of
 * two grey images, into d_dst, DEVICE memory.  d_left and d_right are the
 * images sgm_process_device takes on a handle with no input stage set: height x
 * width bytes, `pitch` bytes per row, read decimated by scale; the handle's
 * min_disp is the one used.  kind is SGM_COST_SAD, SGM_COST_SSD or SGM_COST_CT,
 * whatever sgm_set_cost says.  One launch on `stream` (NULL = the handle's stream), no
 * host wait, no allocation: capturable into a HIP graph.  Any handle of the
 * working size serves, aux_only included.  The volume goes straight into
 * sgm_aggregate_device (SGM_VOL_F32, strides cols * D, D, 1).  Timed under the
 * profile class "window_cost" (CT: "window_cost_ct").  SGM_ERR_INVALID_ARG, with a message, for a bad
 * kind, a NULL or misaligned pointer, pitch < width, and hipStreamLegacy as the
 * stream (see sgm_volume_import_device). */
int sgm_window_cost_device(sgm_handle *h, int kind, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                           float *d_dst, void *stream);
/* Its HOST-memory twin (tests): images in, rows * cols * D floats out; synchronous. */
int sgm_stage_window_cost(sgm_handle *h, int kind, const uint8_t *left, const uint8_t *right, int pitch,
                          float *cost);
/* The columns one workgroup of the producer writes (tests and tools derive
 * their edge-case widths from it). */
int sgm_window_cost_tile_cols(void);

/* ---- the cost filters on a finished volume ----
 *
 * SGM::process runs cost_horizontal_filter(COST_WIN_W / scale) and
 * cost_vertical_filter(COST_WIN_H / scale) over the disparity space image it
 * built (SGM.cpp:66-72, Solver.cpp:296-368) before the path passes.  Census
 * frames have always done so, fused into their cost kernels; these entry points
 * run the same two filters, bit for bit, over a finished dense fp32 rows x cols
 * x D (HWD) volume: win_w = 5 / scale, win_h = 3 / scale (integer division: 5
 * and 3, or 2 and 1).  Horizontal, one serial chain per (row, d):
 *   sum = c[0] + .. + c[win - 1]                  (left to right, from 0)
 *   step t = 0 .. cols - 2 (win / 2) - 1:
 *     c[win - win / 2 - 1 + t] = sum / win        (correctly rounded)
 *     sum += c[win + t];  sum -= c[t]             (two roundings; not after the last step)
 * in place, so c[t] is an already FILTERED value once t >= win - win / 2 - 1: an
 * IIR, not a box filter.  The columns the steps do not write keep their raw
 * values (two on either side at win 5; the last two at win 2).  Vertical: the
 * same recursion down each (col, d) chain; win 1 is not the identity ((c0 + c1)
 * - c0 is rounded twice) and is reproduced.  Order: horizontal, then vertical.
 * Filtered values may leave [0, 999999]: after a steep drop the recursion
 * undershoots below zero (census frames beside sky pixels do the same).  The
 * maps stay pinned all the same: the path passes that follow are the ones
 * census frames run on such volumes.  Other windows are not offered. */
enum { SGM_FILTER_H = 1, SGM_FILTER_V = 2 };   /* sgm_stage_cost's `filters` bits */

/* The filters every later VOLUME frame of the handle runs: sgm_aggregate_device
 * and the frames of SAD / SSD handles (sgm_set_cost).  0 = off, every handle's
 * default: such a handle enqueues exactly the launches it always did.  A
 * property of the handle like sgm_set_cost (sgm_params and SGM_HIP_VERSION are
 * unchanged); it allocates nothing (every frame handle holds the Ch volume the
 * census frames filter through) and waits for nothing; call it outside stream
 * capture and re-capture graphs afterwards.  The filters run after the import or
 * producer launch; with views == 2 the right view's volume is first derived
 * from the RAW left volume, then each view is filtered on its own, as the
 * reference builds each view's DSI and then filters it.  The horizontal filter
 * is one launch over both views (profile class "vol_hfilter"); the vertical one
 * runs fused with the L3 forward pass, per view ("vfwd", in the place of
 * "pair_fwd_L3").  Census frames ignore the setting: they filter as ever.
 * SGM_ERR_INVALID_ARG, with a message and nothing changed, for bits other than
 * SGM_FILTER_H | SGM_FILTER_V and for BM, aux_only and SGM_VIEW_RIGHT handles. */
int sgm_set_volume_filter(sgm_handle *h, int filters);
int sgm_get_volume_filter(const sgm_handle *h, int *filters);

/* The filters `filters` names (whatever the setter says), in place on d_cost: a
 * dense fp32 HWD volume of the handle's working size and D in DEVICE memory,
 * 16-byte aligned.  Only enqueues on `stream` (NULL = the handle's stream): no
 * host wait, no allocation, capturable into a HIP graph.  The horizontal filter
 * alone runs inside d_cost; with the vertical one the call goes through the
 * left view's Ch volume and L3 checkpoints, scratch every frame rewrites, so
 * it is refused on aux_only handles, which hold none (every other handle
 * serves, BM and SGM_VIEW_RIGHT ones included).  The vertical filter alone
 * costs one device copy more (profile class "vol_copy").  A volume filtered
 * this way and handed to sgm_aggregate_device on a handle whose setting is 0
 * gives the maps the setting gives on a views == 1 handle; with views == 2 the
 * setting filters the derived right volume itself, which a caller-side filter
 * of the left volume cannot reproduce.  SGM_ERR_INVALID_ARG, with a message and
 * nothing enqueued, for a NULL or misaligned pointer, filters outside 1 .. 3,
 * hipStreamLegacy as the stream (see sgm_volume_import_device) and aux_only
 * handles. */
int sgm_filter_volume_device(sgm_handle *h, float *d_cost, int filters, void *stream);
/* Its HOST-memory twin (tests): rows * cols * D floats, filtered in place; synchronous. */
int sgm_stage_filter_volume(sgm_handle *h, float *cost, int filters);
/* The steps of one prefetched block of the horizontal filter's main loop (tests
 * and tools derive their edge-case widths from it). */
int sgm_volume_filter_block(void);
/* The columns of one strip of the slanted schedule's strip pass (tests derive
 * their edge-case widths from it). */
int sgm_vstrip_cols(void);

/* ---- the matching window: WIN_H, WIN_W of inc/Solver.h as a setting ----
 *
 * The reference writes WIN_H = 7, WIN_W = 9 as constants, but its cost functions
 * take the window at run time: Solver::build_cost_table and build_dsi pass
 * WIN_H / scale, WIN_W / scale (Solver.cpp:98-99, :127-128) to CT_pts, SAD and
 * SSD (cost.cpp).  sgm_set_window(h, win_h, win_w) sets those two constants for
 * one handle, BEFORE the division by scale; every handle starts at (7, 9).
 * With e_h = win_h / scale, e_w = win_w / scale (integer division), HH = e_h /
 * 2 and HW = e_w / 2, the loops run -HH .. HH and -HW .. HW (cost.cpp:8,14,107,
 * 111), so an even e_w = 4 still has 5 taps, as the default has at scale 2.
 *   census    CT_pts over (2 HH + 1) x (2 HW + 1) taps, the centre skipped, bits
 *             MSB first in row-major order, coordinates clamped to the
 *             working-grid edge, on the blurred image when params.blur = 1
 *   SAD, SSD  the integer sum over the same taps, then / e_h and / e_w: two
 *             correctly rounded fp32 divisions in that order (the divisors
 *             are e_h and e_w, not the tap counts)
 * Accepted: 1 <= e_h, e_w <= 9, not HH = HW = 0, and at most 64 census bits,
 * which excludes only HH = HW = 4 (80 bits: the reference's own word would
 * shift bits out).  Anything else returns SGM_ERR_INVALID_ARG with a message
 * and changes nothing.  The largest sum stays 63 taps * 255^2.
 * The window is read by every consumer of the census tables and of the window
 * costs on the handle: SGM frames of every schedule, one and two views,
 * SGM_SOLVER_BM, sgm_stage_census, frames after sgm_set_cost(SAD | SSD),
 * sgm_window_cost_device and sgm_stage_window_cost; any handle takes it,
 * aux_only included (it serves sgm_window_cost_device).  LKRefine's window, the
 * 5 x 3 cost filters, the median and the speckle constants are not part of it.
 * A property of the handle, like sgm_set_min_disp (sgm_params and
 * SGM_HIP_VERSION are unchanged): it synchronises the handle's last work,
 * allocates nothing, is to be called outside stream capture, and graphs are to
 * be re-captured afterwards.  (7, 9) launches exactly what an untouched handle
 * launches. */
int sgm_set_window(sgm_handle *h, int win_h, int win_w);
int sgm_get_window(const sgm_handle *h, int *win_h, int *win_w);

/* ---- weighted windows: WEIGHTED_COST of inc/Solver.h as a setting ----
 *
 * With WEIGHTED_COST on, Solver::Solver builds a Gaussian table over the window
 * (Solver.cpp:29-45), with e_h, e_w, HH, HW as above:
 *   w[a][b] = (float)exp(((a - HH)^2 + (b - HW)^2) / -25.0),  a < e_h, b < e_w
 * computed in double on the host whenever this setting or the window changes.
 *   SAD, SSD  cost = 0.0f; over the taps in row-major order (a outer, b inner):
 *             cost = cost + (float)AD * w[a][b], one fp32 multiply and one fp32
 *             add, never fused, AD the integer |L - R| or (L - R)^2 at the
 *             clamped coordinates of SGM_COST_*; then cost / e_h / e_w, two
 *             correctly rounded divisions (cost.cpp:19-22, :48-51)
 *   census    CT_pts skips every tap with w[a][b] < 0.5 (cost.cpp:115-116), that
 *             is every tap outside the disc (a - HH)^2 + (b - HW)^2 <= 17; the
 *             kept bits are appended in the same order, so the word narrows:
 *             7 x 9 keeps 50 of 62 bits, 7 x 7 44 of 48, 5 x 9 40 of 44; 5 x 5,
 *             3 x 3, 1 x 9 keep every bit.  Everything after the census sees
 *             only the words.
 * Odd effective windows only: with e_h or e_w even the reference indexes its
 * table one past a row's end (at the default window and scale 2, 3 x 4 with
 * 3 x 5 taps, past the table), which defines nothing.  sgm_set_weighted(h, 1)
 * returns SGM_ERR_INVALID_ARG with a message when e_h or e_w is even, and
 * sgm_set_window returns the same on a weighted handle for a window that would
 * make either even -- (7, 9) at scale 2 is such a window; set (14, 18), or
 * another odd pair, first.  Every other rule of sgm_set_window holds.
 * Every consumer of the handle's window follows the setting: the census of SGM
 * and BM frames of every schedule, sgm_stage_census, SAD / SSD frames,
 * sgm_window_cost_device and sgm_stage_window_cost; any handle takes it,
 * aux_only, BM and SGM_VIEW_RIGHT ones included.  A property of the handle like
 * sgm_set_window (sgm_params and SGM_HIP_VERSION are unchanged): it
 * synchronises the handle's last work, allocates nothing, is to be called
 * outside stream capture, and graphs are to be re-captured afterwards.  Off, the
 * default, launches exactly what an untouched handle launches; on, the census
 * launch (profile class "census_masked" where the disc drops a tap) and the
 * producer launch ("window_cost_weighted") are other kernels. */
int sgm_set_weighted(sgm_handle *h, int enable);
int sgm_get_weighted(const sgm_handle *h, int *enabled);
/* The e_h x e_w table in use, row-major, into w[0 .. max - 1]; *count = e_h * e_w
 * (w NULL: the count alone).  SGM_ERR_INVALID_ARG on a handle that is not
 * weighted, or with max below the count. */
int sgm_get_window_weights(sgm_handle *h, float *w, int max, int *count);

/* Post-sync validity check of the frames enqueued so far (the reference has
 * no asynchronous work to check: SGM::process is synchronous, SGM.cpp:32-826).
 * Waits for the handle's last call's work (its stream, or the event the call
 * recorded on the caller's stream), then returns SGM_ERR_HIP, with the
 * message in sgm_last_error, if any slanted-pass hand-off gave up, or any
 * fixed-budget median fill ended unproven (sgm_set_post_filter_launches),
 * since the last report -- the maps of the frames in between are then invalid
 * -- and clears the report; else SGM_OK.  Frames replayed from a captured HIP graph
 * are not calls on the handle: synchronise the graph's stream first, then
 * call sgm_check.  A caller that gathers or times maps should call it after
 * synchronising and before trusting them. */
int sgm_check(sgm_handle *h);

/* The LR check of SGM.cpp:803-818 on DEVICE working-grid maps: out(i, j) =
 * fl(i, j), or D+1 where j >= fl and |fl - fr(i, (int)(j - fl/s))| > lr_max_diff.
 * fl is the left view's sub-pixel map (filtered_disp), fr the right view's
 * (filtered_disp_beta), e.g. from two SGM_VIEW_LEFT / SGM_VIEW_RIGHT handles on
 * two GPUs with fr copied over; pitches in floats; d_out may alias d_fl but not
 * d_fr.  Any handle of the working size (aux_only included) serves.  Enqueued
 * on `stream` (NULL = the handle's stream); sgm_post_filter_device and
 * sgm_lk_refine_device then complete get_disp()'s map. */
int sgm_lr_check_device(sgm_handle *h, const float *d_fl, int fl_pitch, const float *d_fr,
                        int fr_pitch, float *d_out, int out_pitch, void *stream);

/* post_filter() (Solver.cpp:600-649: median fill :604-630, speckle_filter_new
 * :514-566) on the GPU, bit-exact against its single-thread semantics, in
 * place on a DEVICE map of the handle's working size (rows x cols f32, row
 * pitch in floats), enqueued on `stream` (NULL = the handle's stream).  The
 * median fill iterates to a proven fixed point; the call synchronises
 * `stream` once per two fill launches to read the convergence counter, and
 * returns with the speckle kernels enqueued (the caller synchronises).  With
 * a launch budget (sgm_set_post_filter_launches) it only enqueues. */
int sgm_post_filter_device(sgm_handle *h, float *d_disp, int pitch, void *stream);

/* The median fill's launch budget, a property of the handle (like
 * sgm_set_profiling; sgm_params is unchanged).
 * n == 0 (default): the adaptive fill (the host reads the convergence counter).
 * 1 <= n <= 4096: every post filter on this handle enqueues exactly n median-fill
 * launches, then the component kernels once, with no host readback, no event wait and
 * no stream synchronisation: the call returns after enqueueing and may be captured into
 * a HIP graph.  Launches after the one that proved the fixed point return at once.  If
 * launch n's change counter is not zero the fixed point is not proven: that frame's map
 * is invalid and is reported like a slanted hand-off timeout (sgm_check, or the next
 * sgm_process[_device] call; the synchronous sgm_process and sgm_stage_post_filter
 * check after their own work and return it themselves), once, then cleared; the
 * message reads "median fill not proven in <n> launches", n the budget of that filter.
 * ceil(cols / 64) * rows + 1 launches always prove it (DESIGN.md "Post filter"); stereo
 * maps need far fewer (sgm_post_filter_proved_at measures it; README).
 * Any other n, or a handle without post-filter buffers: SGM_ERR_INVALID_ARG. */
int sgm_set_post_filter_launches(sgm_handle *h, int n);

/* Waits as sgm_check does (without reading or clearing its report), then *launch =
 * 1-based index of the first fill launch of the handle's last post filter whose counter
 * was zero (the proof), or 0 if none was (or no post filter has run).  For sizing n.
 * Works after adaptive and fixed-budget filters, eager or replayed from a graph
 * (synchronise the graph's stream first). */
int sgm_post_filter_proved_at(sgm_handle *h, int *launch);

/* ---- match confidence: the uniqueness test's own quotient, per pixel ----
 *
 * ratio(i, j) = min_cost / sec_min_cost (SGM.cpp:392-409's locals) as one fp32
 * division: min_cost = min_d S[i, j, d], sec_min_cost the smallest S[i, j, d]
 * != min_cost, or FLT_MAX (SGM.cpp:399's initial value) when every cost of
 * the pixel is equal.  S is what the handle aggregates (8 paths, or
 * ((L1 + L2) + L3) + L4 with paths = 4).  Range [0, 1); lower = more
 * distinctive.  (Frames with sky masks only: beside a masked pixel's 999999
 * override a path cost C + min(...) - minL_prev can be negative, and the
 * quotient of such a pixel lies outside [0, 1); it is still the number the
 * uniqueness test compared.)  A pixel the uniqueness test invalidated has ratio >
 * params.uniqueness (and |min_d - sec_d| > 1).  The map is the WTA's: the LR
 * check, post_filter and LKRefine do not change it.  Bit-exact against the
 * oracle's aggregated volume (tests/confidence_recipe.py).
 *
 * A property of the handle (like sgm_set_post_filter_launches; sgm_params is
 * unchanged).  enable != 0: allocates one rows x cols f32 map per view the
 * handle computes (counted in sgm_device_bytes), and every later frame's final
 * pass (and sgm_stage_aggregate) stores the quotient beside the sub-pixel
 * map, in that map's layout (column-major in the two-view frames that keep a
 * column-major sub-pixel map; sgm_confidence_device transposes on the way
 * out, so no row-major twin is kept).  enable == 0: frees them; frames run
 * exactly as before.  Synchronises the handle's last work first; call it
 * outside stream capture, and re-capture graphs afterwards.  BM and aux_only
 * handles: SGM_ERR_INVALID_ARG. */
int sgm_set_confidence(sgm_handle *h, int enable);

/* Copies the last frame's ratio map of `view` (SGM_VIEW_LEFT / SGM_VIEW_RIGHT;
 * a views = 1 handle serves only its own view) to the caller's row-major
 * DEVICE buffer (rows x cols f32, pitch in floats >= cols; padding untouched).
 * One kernel enqueued on `stream` (NULL = the handle's stream), no host wait:
 * capturable into a HIP graph with the frame.  Ordered after the frame as
 * every call on the handle is ("Streams" above).  SGM_ERR_INVALID_ARG when
 * confidence is off or the handle does not compute that view. */
int sgm_confidence_device(sgm_handle *h, int view, float *d_ratio, int pitch, void *stream);

/* In place on a DEVICE working-grid map: disp = D+1 where ratio > max_ratio
 * (pitches in floats).  One elementwise kernel on `stream`; any handle of the
 * working size serves, aux_only included.  Applies a stricter uniqueness than
 * the frame's without re-running it.  It tests the quotient alone: the WTA's
 * second clause, |min_d - sec_d| > 1 (adjacent minima are kept whatever their
 * ratio), is NOT reproduced, so max_ratio = params.uniqueness invalidates a
 * superset of what the frame did. */
int sgm_confidence_filter_device(sgm_handle *h, float *d_disp, int pitch, const float *d_ratio,
                                 int ratio_pitch, float max_ratio, void *stream);

/* LKSubPixelImpl::LKRefine(img_l, img_r, disp_float) (LKRefine/LKSubPixelImpl.cpp:
 * 13-235) on the GPU: per-pixel Gauss-Newton refinement of the disparity over
 * a 7x7 window, interior pixels truncated first (:80), border pixels untouched.
 * d_left/d_right: DEVICE u8 images at the handle's full size (height x width,
 * row pitch in bytes), decimated by the scale as :29-44 does; d_disp: DEVICE
 * working-grid map (rows x cols f32, pitch in floats), refined in place.
 * Enqueued on `stream` (NULL = the handle's stream); the caller synchronises.
 * fp32 sums follow oracle/sgm_oracle.c:orc_lk_refine bit-for-bit (the
 * reference's Eigen reduction order is not pinned). */
int sgm_lk_refine_device(sgm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int pitch,
                         float *d_disp, int disp_pitch, void *stream);

/* SkyAreaDetector::detect(img, file, sky_label, scale) (sky_detector/
 * imageSkyDetector.cpp:166-208) on the GPU: d_img a DEVICE u8 image at the
 * handle's full size (height x width, pitch bytes); d_mask the DEVICE u8 mask
 * on the working grid (rows x cols, mask_pitch bytes), 255 = sky.  Four
 * launches on `stream` (NULL = the handle's stream), no host round trip.
 * Numerics pinned as oracle/sgm_oracle.c:orc_sky_detect (which reproduces
 * the reference's example/000017_14 mask exactly).  The debug image the
 * reference writes to `file` is not produced. */
int sgm_sky_detect_device(sgm_handle *h, const uint8_t *d_img, int pitch, uint8_t *d_mask,
                          int mask_pitch, void *stream);

/* Solver::colormap (src/Solver.cpp:652-707) of a DEVICE working-grid map
 * (rows x cols f32, pitch in floats) into DEVICE BGR (rows x cols x 3 u8,
 * bgr_pitch bytes): the image show_disp publishes (Solver.cpp:55-93).  With
 * a minimum disparity m set the colours are those of disp - (float)m over D. */
int sgm_colormap_device(sgm_handle *h, const float *d_disp, int pitch, uint8_t *d_bgr,
                        int bgr_pitch, void *stream);

/* The point cloud of node.cpp:119-143 from a DEVICE working-grid map: every
 * pixel with disp != D+1 and Z = (fx+fy)/2 * baseline / (disp + 1e-6) <=
 * max_range becomes (X, Y, Z) (doubles) and the gray value img(i, j) of the
 * DEVICE image d_img (img_pitch bytes; the node reads its full-size image
 * at working-grid indices, node.cpp:137), in row-major order.  d_xyz holds
 * up to rows*cols*3 doubles, d_pixel rows*cols bytes; *d_count (device int)
 * receives the number of points.  Enqueued on `stream`. */
int sgm_point_cloud_device(sgm_handle *h, const float *d_disp, int pitch, const uint8_t *d_img,
                           int img_pitch, const sgm_camera *cam, double *d_xyz,
                           uint8_t *d_pixel, int *d_count, void *stream);

/* ---- multi-GPU: pairs shard one per device, maps gathered to rank 0 ----
 *
 * stereo pairs are independent, so a batch runs one pair per
 * GPU (one sgm_handle per device) and the only collective is the gather of
 * the H x W disparity maps to rank 0: RCCL's ncclGather over xGMI (1.86 MB
 * per rank at K128).  The reference has no multi-GPU path; its per-pair call
 * is node.cpp:49,93 (SGM sgm(h, w, s, d); sgm.process(l, r)), which
 * include/sgm_amd/BatchSGM.h runs on every device of a batch, one host
 * thread per device.  RCCL is bound at run time on the first sgm_comm_*
 * call (an RCCL the process already holds, e.g. PyTorch's, is reused;
 * SGM_RCCL_LIB names another).  Errors before a communicator exists are
 * read with sgm_comm_last_error(NULL), per calling thread (as errno). */
typedef struct sgm_comm sgm_comm;

#define SGM_COMM_ID_BYTES 128  /* = sizeof(ncclUniqueId) */

/* Single process driving n devices, ranks 0..n-1 = devices[0..n-1]
 * (ncclCommInitAll).  Each device appears once. */
int sgm_comm_create(const int *devices, int n, sgm_comm **out);
/* One process per device (the torch.distributed.run layout): rank 0 makes an
 * id, every process receives it out of band and joins as `rank` of `nranks`
 * on `device` (ncclGetUniqueId / ncclCommInitRank; blocks until all joined). */
int sgm_comm_unique_id(char id[SGM_COMM_ID_BYTES]);
int sgm_comm_create_rank(const char id[SGM_COMM_ID_BYTES], int nranks, int rank, int device,
                         sgm_comm **out);
int sgm_comm_destroy(sgm_comm *c);
const char *sgm_comm_last_error(const sgm_comm *c);
/* ranks in the communicator, the first rank this object holds, and how many */
int sgm_comm_info(const sgm_comm *c, int *nranks, int *first_rank, int *nlocal);

/* Rank `rank`'s contribution to the gather (ncclGather, root 0): its DEVICE
 * map d_map (rows x cols f32, row pitch in floats >= cols; pitched maps are
 * packed first) lands at d_root_out + rank * rows * cols on rank 0's device
 * (nranks * rows * cols floats; ignored on other ranks).  Enqueued on
 * `stream`, a hipStream_t of the rank's device (NULL: the legacy default
 * stream), after the map's producer on that stream; returns after
 * enqueueing.  Every rank of the communicator must call it with the same
 * rows and cols: from its own host thread, or through sgm_batch_gather_all
 * when one thread drives all ranks.  Call sgm_check on the producing handle
 * first: a map from a frame sgm_check rejects is not valid.  A pitched map is
 * packed into one staging buffer per rank, so one rank's gathers go on one
 * stream (or are otherwise ordered). */
int sgm_batch_gather(sgm_comm *c, int rank, const float *d_map, int rows, int cols, int pitch,
                     float *d_root_out, void *stream);
/* The same for every rank this object holds, from one thread (one RCCL
 * group): d_maps[k] and streams[k] (NULL array: default streams) belong to
 * rank first_rank + k. */
int sgm_batch_gather_all(sgm_comm *c, const float *const *d_maps, int rows, int cols, int pitch,
                         float *d_root_out, void *const *streams);

/* ---- per-kernel timing (HIP events recorded around every launch) ---- */

typedef struct sgm_kernel_stat {
    char name[32];      /* kernel class, e.g. "sweep_L3_acc" */
    int launches;       /* completed launches since the last read */
    double total_ms;    /* sum of event-measured durations */
    double elems;       /* pixel-disparity elements touched per launch (mean over the launches) */
} sgm_kernel_stat;

/* enable != 0: every subsequent launch is bracketed by two HIP events on the
 * stream it runs on.  Off by default. */
int sgm_set_profiling(sgm_handle *h, int enable);
/* Synchronises the handle's device, folds all pending event pairs into the
 * per-class statistics, copies up to max entries to out, sets *count, and
 * resets the statistics. */
int sgm_get_profile(sgm_handle *h, sgm_kernel_stat *out, int max, int *count);

/* ---- stage entry points (host buffers, synchronous), for parity tests ---- */

/* Decimation + optional pre-blur + CT_pts on ONE image (cost.cpp:99-129).
 * img: height x width (full size, pitch bytes); ct: rows x cols u64. */
int sgm_stage_census(sgm_handle *h, const uint8_t *img, int pitch, uint64_t *ct);
/* build_dsi_from_table[_beta] + filters (Solver.cpp:143-248, 296-368).
 * view 0 = left, 1 = right; filters bit 1 = horizontal, bit 2 = vertical.
 * cost: rows x cols x D f32.  ctl/ctr are unshifted tables (sgm_stage_census):
 * with a minimum disparity m set the stage applies its view's shift, so
 * cost[.., d] is the cost of disparity m + d. */
int sgm_stage_cost(sgm_handle *h, const uint64_t *ctl, const uint64_t *ctr,
                   const uint8_t *sky, int view, int filters, float *cost);
/* One path DP over a cost volume (SGM.cpp:81-369): L (rows x cols x D) and
 * minL (rows x cols).  A 4-path handle (params.paths == 4) serves L1..L4 and
 * returns SGM_ERR_INVALID_ARG for L5..L8. */
int sgm_stage_path(sgm_handle *h, int dir, const float *cost, float *L, float *minL);
/* 8 paths (4 with params.paths == 4: ((L1+L2)+L3)+L4) + aggregation + WTA +
 * uniqueness + sub-pixel (SGM.cpp:81-443).  disp and sub leave in true
 * disparity (+ the handle's minimum disparity). */
int sgm_stage_aggregate(sgm_handle *h, const float *cost, uint16_t *disp, float *sub);
/* sgm_confidence_device with a HOST buffer: ratio rows x cols f32 (dense), the
 * map of `view` left by the last frame or sgm_stage_aggregate (view 0 of a
 * two-view handle, the handle's own view otherwise); synchronous. */
int sgm_stage_confidence(sgm_handle *h, int view, float *ratio);
/* sgm_confidence_filter_device with HOST buffers: disp and ratio rows x cols
 * f32 (dense), disp filtered in place; synchronous. */
int sgm_stage_confidence_filter(sgm_handle *h, float *disp, const float *ratio, float max_ratio);
/* LR check (SGM.cpp:803-818): out = checked copy of fl. */
int sgm_stage_lr(sgm_handle *h, const float *fl, const float *fr, float *out);
/* post_filter() (Solver.cpp:600-649) on a HOST rows x cols map, in place,
 * computed on the GPU (sgm_post_filter_device); synchronous.  With a launch
 * budget (sgm_set_post_filter_launches) a fill the budget did not prove is
 * this call's error: SGM_ERR_HIP, and the map written back is invalid. */
int sgm_stage_post_filter(sgm_handle *h, float *disp);
/* LKRefine (sgm_lk_refine_device) with HOST buffers: left/right full-size u8
 * images (pitch bytes), disp a rows x cols map refined in place; synchronous. */
int sgm_stage_lk_refine(sgm_handle *h, const uint8_t *left, const uint8_t *right, int pitch,
                        float *disp);
/* Sky detector (sgm_sky_detect_device) with HOST buffers: img full-size
 * (pitch bytes), mask rows x cols; synchronous. */
int sgm_stage_sky_detect(sgm_handle *h, const uint8_t *img, int pitch, uint8_t *mask);
/* colormap with HOST buffers: disp rows x cols, bgr rows x cols x 3. */
int sgm_stage_colormap(sgm_handle *h, const float *disp, uint8_t *bgr);
/* point cloud with HOST buffers: disp rows x cols, img the full-size image
 * (img_pitch bytes); xyz (3*rows*cols doubles) and pixel (rows*cols) receive
 * *count points. */
int sgm_stage_point_cloud(sgm_handle *h, const float *disp, const uint8_t *img, int img_pitch,
                          const sgm_camera *cam, double *xyz, uint8_t *pixel, int *count);

#ifdef __cplusplus
}
#endif
#endif
