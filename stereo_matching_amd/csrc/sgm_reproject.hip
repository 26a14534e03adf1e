// sgm_reproject.hip -- the disparity map through stereoRectify's Q: the organized
// XYZ image of cv::reprojectImageTo3D and the depth images (f32, and u16 as ROS
// REP 118 has it), pinned as DESIGN.md 5m states it and tests/reproject_recipe.py
// restates it; and its part of the C-ABI (include/sgm_hip.h): the setter, the
// _device launch, its host round trip and the last frame's products.
//
// One streaming kernel, one lane per pixel: 4 B in, 12, 4 and 2 B out.  The
// product set is a template mask, so a frame that asks for depth alone carries
// no XYZ code.  A wave takes 256 columns of one row as four 64-column chunks
// whose loads are issued before the first is computed; a workgroup four rows.
// The row's terms q1 y, q5 y, q9 y, q13 y are formed once per wave, and the sums
// keep 5m's association: ((q0 x + q1 y) + q2 d) + q3.  Every operation is one
// IEEE double operation (the library is built with -ffp-contract=off; HIP's
// double division is the correctly rounded one).  The library is also built
// with -fno-honor-nans: the missing value is stored as a bit pattern, validity
// comes from the disparity compare, W' == 0.0 and ordered compares of finite
// values, and the division never sees the zero (so no NaN is ever computed).
//
// The interleaved XYZ stores, two forms (profiles/reproject_ab.txt):
//   form 0: each lane stores its pixel's 12 bytes (a wave covers 768 contiguous
//           bytes with one 12-byte store per lane)
//   form 1: the wave's 192 dwords go through LDS and leave as 16-byte stores of
//           48 lanes (a row's last chunk: the dwords past the last whole 16
//           bytes one by one)
// Global memory takes either at any dword address, so the caller's pointers and
// pitches need no more than their type's alignment; nothing is written past
// 3 x cols floats (cols elements) of a row.
#include "sgm_device.h"
#include "sgm_handle.h"
#include "sgm_reproject_args.h"

#include <stdlib.h>

namespace sgm {
namespace {

constexpr uint32_t kMissingBits = 0x7FC00000u;  // the missing pixel's value, in xyz and depth
constexpr int kRpChunks = 4;                    // 64-column chunks per wave
constexpr int kRpCols = 64 * kRpChunks;         // columns per workgroup
constexpr int kRpRows = 4;                      // rows per workgroup (one per wave)

struct ReprojectArgs {
    double q[16];
    const float *disp;
    uint32_t *xyz, *depth;  // (f32 products, stored as bit patterns)
    uint16_t *d16;
    int pitch, xyz_pitch, depth_pitch, d16_pitch;  // in elements
    int rows, cols, scale;
    float invalid;  // (float)(D + min_disp + 1)
    float max_range, depth_scale;
};

template <int MASK, int FORM>
__global__ __launch_bounds__(256) void reproject_kernel(ReprojectArgs a) {
    const int lane = tid_x() & 63, wave = wave_id();
    const int i = bid_y() * kRpRows + wave;
    const int x0 = bid_x() * kRpCols;
    if (i >= a.rows) return;  // (wave-uniform)
    const float *__restrict__ row = a.disp + (size_t)i * a.pitch;
    float dv[kRpChunks];
#pragma unroll
    for (int c = 0; c < kRpChunks; ++c) {
        const int j = x0 + 64 * c + lane;
        dv[c] = j < a.cols ? row[j] : 0.0f;
    }
    const double y = (double)(i * a.scale);
    const double ry0 = a.q[1] * y, ry1 = a.q[5] * y, ry2 = a.q[9] * y, ry3 = a.q[13] * y;
#pragma unroll
    for (int c = 0; c < kRpChunks; ++c) {
        const int j0 = x0 + 64 * c, j = j0 + lane;
        if (j0 >= a.cols) break;  // (wave-uniform)
        const bool active = j < a.cols;
        const double x = (double)(j * a.scale), d = (double)dv[c];
        const double wp = ((a.q[12] * x + ry3) + a.q[14] * d) + a.q[15];
        const double zp = ((a.q[8] * x + ry2) + a.q[10] * d) + a.q[11];
        const bool w0 = wp == 0.0;
        const double iw = 1.0 / (w0 ? 1.0 : wp);
        const float Z = (float)(zp * iw);
        bool missing = dv[c] == a.invalid || w0;
        if (a.max_range > 0.0f) missing = missing || !(0.0f < Z && Z <= a.max_range);
        const uint32_t zb = missing ? kMissingBits : __float_as_uint(Z);
        if constexpr ((MASK & kReprojectDepth) != 0) {
            if (active) a.depth[(size_t)i * a.depth_pitch + j] = zb;
        }
        if constexpr ((MASK & kReprojectDepth16) != 0) {
            const float r = __builtin_rintf(Z * a.depth_scale);
            const bool fits = r >= 1.0f && r <= 65535.0f;
            const int v = (int)fminf(fmaxf(r, 0.0f), 65535.0f);
            if (active) a.d16[(size_t)i * a.d16_pitch + j] = (uint16_t)(fits && !missing ? v : 0);
        }
        if constexpr ((MASK & kReprojectXyz) != 0) {
            const double xp = ((a.q[0] * x + ry0) + a.q[2] * d) + a.q[3];
            const double yp = ((a.q[4] * x + ry1) + a.q[6] * d) + a.q[7];
            const float X = (float)(xp * iw), Y = (float)(yp * iw);
            uint32_t v[3] = {missing ? kMissingBits : __float_as_uint(X),
                             missing ? kMissingBits : __float_as_uint(Y), zb};
            uint32_t *dst = a.xyz + (size_t)i * a.xyz_pitch + 3 * (size_t)j0;  // the chunk's first dword
            if constexpr (FORM == 0) {
                if (active) __builtin_memcpy(dst + 3 * lane, v, 12);
            } else {
                __shared__ __attribute__((aligned(16))) uint32_t tile[kRpRows][192];
                uint32_t *w = tile[wave];
                // (LDS serves a wave's accesses in order: the reads below see these writes, and the
                // next chunk's writes land after them)
                w[3 * lane] = v[0];
                w[3 * lane + 1] = v[1];
                w[3 * lane + 2] = v[2];
                __builtin_amdgcn_wave_barrier();
                const int n = a.cols - j0 < 64 ? a.cols - j0 : 64;
                const int total = 3 * n, whole = total & ~3;
                if (4 * lane + 4 <= total) {
                    uint32_t t[4];
                    __builtin_memcpy(t, w + 4 * lane, 16);
                    __builtin_memcpy(dst + 4 * lane, t, 16);
                }
                if (lane < total - whole) dst[whole + lane] = w[whole + lane];
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

}  // namespace

// One launch: the products whose pointers are not null (at least one).  form:
// the XYZ store form (0 or 1; ignored without XYZ).
hipError_t launch_reproject(const double *q, const float *disp, int pitch, float *xyz, int xyz_pitch,
                            float *depth, int depth_pitch, uint16_t *depth16, int depth16_pitch,
                            float invalid, float max_range, float depth_scale, int form, Geom g,
                            hipStream_t st) {
    ReprojectArgs a{};
    for (int k = 0; k < 16; ++k) a.q[k] = q[k];
    a.disp = disp;
    a.xyz = reinterpret_cast<uint32_t *>(xyz);
    a.depth = reinterpret_cast<uint32_t *>(depth);
    a.d16 = depth16;
    a.pitch = pitch;
    a.xyz_pitch = xyz_pitch;
    a.depth_pitch = depth_pitch;
    a.d16_pitch = depth16_pitch;
    a.rows = g.H;
    a.cols = g.W;
    a.scale = g.scale;
    a.invalid = invalid;
    a.max_range = max_range;
    a.depth_scale = depth_scale;
    const int mask = (xyz ? kReprojectXyz : 0) | (depth ? kReprojectDepth : 0) | (depth16 ? kReprojectDepth16 : 0);
    const dim3 grid((unsigned)((g.W + kRpCols - 1) / kRpCols), (unsigned)((g.H + kRpRows - 1) / kRpRows));
#define SGM_RP_LAUNCH(M, F) hipLaunchKernelGGL((reproject_kernel<M, F>), grid, dim3(256), 0, st, a)
#define SGM_RP_XYZ(M)                \
    if (form == 0) SGM_RP_LAUNCH(M, 0); \
    else SGM_RP_LAUNCH(M, 1);        \
    break
    switch (mask) {
    case 1: SGM_RP_XYZ(1);
    case 2: SGM_RP_LAUNCH(2, 0); break;
    case 3: SGM_RP_XYZ(3);
    case 4: SGM_RP_LAUNCH(4, 0); break;
    case 5: SGM_RP_XYZ(5);
    case 6: SGM_RP_LAUNCH(6, 0); break;
    case 7: SGM_RP_XYZ(7);
    default: return hipErrorInvalidValue;  // (no product: there is nothing to launch)
    }
#undef SGM_RP_XYZ
#undef SGM_RP_LAUNCH
    return hipGetLastError();
}

}  // namespace sgm

using namespace sgm;

namespace {

// The XYZ store form every handle uses (profiles/reproject_ab.txt), unless
// SGM_REPROJECT_STORE = 0 / 1 names one (tools/reproject_time.py times both).
constexpr int kReprojectForm = 0;

int reproject_form() {
    const char *e = getenv("SGM_REPROJECT_STORE");
    return e && (*e == '0' || *e == '1') && !e[1] ? *e - '0' : kReprojectForm;
}

size_t product_elems(const sgm_handle *h, int which) {
    return (size_t)h->g.H * h->g.W * reproject_channels(which);
}

// The launch, on a handle whose Q is set, into whichever buffers are not null.
int enqueue(sgm_handle *h, const float *d_disp, int pitch, float *d_xyz, int xyz_pitch, float *d_depth,
            int depth_pitch, uint16_t *d_depth16, int depth16_pitch, hipStream_t st) {
    HIPCHK(h, timed(h, "reproject", (double)h->g.H * h->g.W, st, [&] {
               // (a true-disparity map: the invalid marker is D + min_disp + 1)
               return launch_reproject(h->rp.q, d_disp, pitch, d_xyz, xyz_pitch, d_depth, depth_pitch, d_depth16,
                                       depth16_pitch, (float)(h->gt.D + 1), h->rp.max_range, h->rp.depth_scale,
                                       h->rp_form, h->g, st);
           }));
    return SGM_OK;
}

// Frees the frame's products.
void free_products(sgm_handle *h) {
    dfree(h, &h->d_rp_xyz);
    dfree(h, &h->d_rp_depth);
    dfree(h, &h->d_rp_d16);
    h->rp_valid = false;
}

// The device buffer of product `which` (one bit) as sgm_get_reprojected hands it out.
int get_product(sgm_handle *h, const char *fn, int which, const void **d_img, int *pitch) {
    if (!reproject_one_bit(which))
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: `which` must be one SGM_REPROJECT_* bit, got %d", fn, which);
    if (!h->rp_on || !(h->rp.outputs & which) || h->p.aux_only)
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: product %d is not in the outputs the handle's frames write (sgm_set_reproject)",
                       fn, which);
    if (!h->rp_valid)
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: no frame has run since reprojection was set", fn);
    *d_img = which == kReprojectXyz ? (const void *)h->d_rp_xyz
                                    : which == kReprojectDepth ? (const void *)h->d_rp_depth : (const void *)h->d_rp_d16;
    *pitch = h->g.W * reproject_channels(which);
    return SGM_OK;
}

}  // namespace

int sgm::reproject_frame(sgm_handle *h, const float *d_map, int pitch, hipStream_t st) {
    const int W = h->g.W;
    if (int rc = enqueue(h, d_map, pitch, h->d_rp_xyz, 3 * W, h->d_rp_depth, W, h->d_rp_d16, W, st)) return rc;
    h->rp_valid = true;
    return SGM_OK;
}

extern "C" {

int sgm_set_reproject(sgm_handle *h, const sgm_reproject *r) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (r && !reproject_set_ok(r->q, r->outputs, r->max_range, r->depth_scale, h->p.aux_only != 0,
                               h->p.view == SGM_VIEW_RIGHT, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_reproject: %s", why);
    // (frames in flight still write the products)
    return change_setting(h, "sgm_set_reproject", !r && !h->rp_on, [&]() -> int {
        if (!r) {
            free_products(h);
            h->rp = sgm_reproject();
            h->rp_on = false;
            return SGM_OK;
        }
        // (an aux_only handle runs no frames: Q alone, for sgm_reproject_device)
        const int want = h->p.aux_only ? 0 : r->outputs;
        // what is missing first, as one group, so that a failed allocation leaves the handle as it was
        int rc = SGM_OK;
        Ledger::Group missing(h->mem);
        if ((want & kReprojectXyz) && !h->d_rp_xyz) rc = dalloc(h, &h->d_rp_xyz, product_elems(h, kReprojectXyz));
        if (!rc && (want & kReprojectDepth) && !h->d_rp_depth) rc = dalloc(h, &h->d_rp_depth, product_elems(h, kReprojectDepth));
        if (!rc && (want & kReprojectDepth16) && !h->d_rp_d16) rc = dalloc(h, &h->d_rp_d16, product_elems(h, kReprojectDepth16));
        if (rc) return rc;
        missing.commit();
        if (!(want & kReprojectXyz)) dfree(h, &h->d_rp_xyz);
        if (!(want & kReprojectDepth)) dfree(h, &h->d_rp_depth);
        if (!(want & kReprojectDepth16)) dfree(h, &h->d_rp_d16);
        h->rp = *r;
        h->rp_on = true;
        h->rp_valid = false;
        h->rp_form = reproject_form();
        return SGM_OK;
    });
}

int sgm_get_reproject(const sgm_handle *h, sgm_reproject *r) {
    if (!h || !r) return SGM_ERR_INVALID_ARG;
    *r = h->rp_on ? h->rp : sgm_reproject();
    return SGM_OK;
}

int sgm_reproject_device(sgm_handle *h, const float *d_disp, int pitch, float *d_xyz, int xyz_pitch,
                         float *d_depth, int depth_pitch, uint16_t *d_depth16, int depth16_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    if (!reproject_call_ok(h->rp_on, d_disp != nullptr, pitch, d_xyz != nullptr, xyz_pitch, d_depth != nullptr,
                           depth_pitch, d_depth16 != nullptr, depth16_pitch, h->g.W, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_reproject_device: %s", why);
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    return enqueue(h, d_disp, pitch, d_xyz, xyz_pitch, d_depth, depth_pitch, d_depth16, depth16_pitch, scope.st);
}

int sgm_stage_reproject(sgm_handle *h, const float *disp, float *xyz, float *depth, uint16_t *depth16) {
    if (!h) return SGM_ERR_INVALID_ARG;
    char why[160];
    const int W = h->g.W;
    if (!reproject_call_ok(h->rp_on, disp != nullptr, W, xyz != nullptr, 3 * W, depth != nullptr, W,
                           depth16 != nullptr, W, W, why, sizeof(why)))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_reproject: %s", why);
    const size_t npx = (size_t)h->g.H * W;
    Staging s(h);
    // staging: the map in d_out, the products in stream-ordered temporaries
    float *d_xyz = xyz ? s.temp<float>(3 * npx) : nullptr, *d_depth = depth ? s.temp<float>(npx) : nullptr;
    uint16_t *d_d16 = depth16 ? s.temp<uint16_t>(npx) : nullptr;
    s.up(h->d_out, disp, npx * sizeof(float));
    s.run([&] { return enqueue(h, h->d_out, W, d_xyz, 3 * W, d_depth, W, d_d16, W, h->st); });
    if (xyz) s.down(xyz, d_xyz, 3 * npx * sizeof(float));
    if (depth) s.down(depth, d_depth, npx * sizeof(float));
    if (depth16) s.down(depth16, d_d16, npx * sizeof(uint16_t));
    return s.finish();
}

int sgm_get_reprojected(sgm_handle *h, int which, const void **d_img, int *pitch) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_img || !pitch) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_get_reprojected: NULL pointer");
    return get_product(h, "sgm_get_reprojected", which, d_img, pitch);
}

int sgm_stage_reprojected(sgm_handle *h, int which, void *img) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!img) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_reprojected: NULL pointer");
    const void *d_img = nullptr;
    int pitch = 0;
    if (int rc = get_product(h, "sgm_stage_reprojected", which, &d_img, &pitch)) return rc;
    Staging s(h);
    s.down(img, d_img, product_elems(h, which) * reproject_elem_bytes(which));
    return s.finish();
}

int sgm_camera_q(const sgm_camera *cam, double q[16]) {
    if (!cam || !q) return SGM_ERR_INVALID_ARG;
    return camera_q(cam->fx, cam->fy, cam->cx, cam->cy, cam->baseline, q) ? SGM_OK : SGM_ERR_INVALID_ARG;
}

}  // extern "C"
