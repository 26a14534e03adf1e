// sgm_fill.hip -- occlusion-aware hole filling of the frame's final map
// (Hirschmueller 2008, 2.6), as tests/fill_recipe.py restates it;
// and its part of the C-ABI (include/sgm_hip.h): the setter, the _device call,
// its host round trip and the last filled frame's mask.
//
// Every invalid pixel takes one of the up to 8 values its rays find first, the
// first valid pixel of the INPUT map in each of the 8 directions: nothing reads a
// filled value, so two launches with no order between their threads do it all.
//
//   fill_march   one lane per image line, six families (workgroup y): columns,
//                diagonals j - i = c and anti-diagonals j + i = c, each walked
//                down and up one row per step.  A lane carries the last valid
//                value it saw and leaves it, at every invalid pixel it passes,
//                in its family's candidate plane.  At a row the lanes of a wave
//                stand in adjacent columns, in every family: each load and each
//                plane store is a row segment.  The loads do not depend on the
//                carry, so they run kFillRing rows ahead in registers and a step
//                is a compare and a select.  Lanes whose line is outside the
//                image at a row touch nothing.
//   fill_select  one wave per row, 64 columns per step.  The W and E candidates
//                come from the row itself: a ballot of the segment's valid
//                lanes, a shuffle from the nearest set bit below (above) the
//                lane, and a carry from segment to segment; the E pass runs
//                first, right to left, into LDS.  Then, left to right: the six
//                planes, the class test against the right view's row span
//                [j0 - (D + min_disp - 1) / scale, j0 + 63] staged in LDS, the
//                sort and the pick (sgm_fill_select.h), and full-line stores of
//                the map (valid pixels copied through) and the mask.
//
// No arithmetic but the class test's one subtraction; the validity test is on
// ordered compares and a bit test for NaN (the library is built with
// -fno-honor-nans).  The launch count is fixed and nothing is read back: the
// stage never waits on the host and can be captured into a HIP graph.
#include "sgm_device.h"
#include "sgm_fill_select.h"
#include "sgm_handle.h"

namespace sgm {
namespace {

constexpr int kFillRing = 16;     // rows a march's loads run ahead of its carry
constexpr int kFillPlanes = 6;    // N, NW, NE (marching down), S, SE, SW (marching up)

struct MarchArgs {
    const float *map;  // rows x cols, pitch floats per row
    float *planes;     // kFillPlanes dense rows x cols planes
    int pitch, H, W;
    float lim;         // valid <= lim
};

// family = kind + 3 * up; kind 0: the column t, 1: the diagonal j - i = t - (H - 1),
// 2: the anti-diagonal j + i = t.  Step s of a march is row s (down) or H - 1 - s (up).
__device__ __forceinline__ int march_col(int kind, int t, int H, int i) {
    return kind == 0 ? t : kind == 1 ? t - (H - 1) + i : t - i;
}

__global__ __launch_bounds__(64) void fill_march_kernel(MarchArgs a) {
    const int fam = bid_y(), kind = fam % 3;
    const bool up = fam >= 3;
    const int t = bid_x() * 64 + tid_x();
    const int H = a.H, W = a.W;
    if (t >= (kind == 0 ? W : H + W - 1)) return;
    float *plane = a.planes + (size_t)fam * H * W;
    float cur[kFillRing], nxt[kFillRing];
    auto load = [&](float (&v)[kFillRing], int s0) {
#pragma unroll
        for (int q = 0; q < kFillRing; ++q) {
            const int s = s0 + q, i = up ? H - 1 - s : s;
            const int j = march_col(kind, t, H, i);
            v[q] = s < H && j >= 0 && j < W ? a.map[(size_t)i * a.pitch + j] : fill_none();
        }
    };
    load(cur, 0);
    float carry = fill_none();
    for (int s0 = 0; s0 < H; s0 += kFillRing) {
        load(nxt, s0 + kFillRing);  // (past the last row: no access)
#pragma unroll
        for (int q = 0; q < kFillRing; ++q) {
            const int s = s0 + q, i = up ? H - 1 - s : s;
            const int j = march_col(kind, t, H, i);
            if (s < H && j >= 0 && j < W) {
                if (fill_valid(cur[q], a.lim)) carry = cur[q];
                else plane[(size_t)i * W + j] = carry;
            }
        }
#pragma unroll
        for (int q = 0; q < kFillRing; ++q) cur[q] = nxt[q];
    }
}

struct SelectArgs {
    float *map;            // in place
    const float *planes;
    const float *right;    // the right view's map (interpolate), element (i, j) at right[i * rs + j * cs]
    uint8_t *mask;
    long long rs, cs;
    int pitch, mask_pitch, H, W;
    int mode, min_disp, D, scale;  // D: the handle's disparity count (not D + min_disp)
    float lim, inv, lr_max_diff;
};

// LDS floats of a select workgroup: the row's E candidates, then the right view's span
__host__ __device__ inline int select_span(int min_disp, int D, int scale) { return (D + min_disp - 1) / scale; }

__global__ __launch_bounds__(64) void fill_select_kernel(SelectArgs a) {
    extern __shared__ float fill_lds[];
    float *e_row = fill_lds, *r_span = fill_lds + a.W;
    const int i = bid_x(), lane = tid_x(), W = a.W;
    float *row = a.map + (size_t)i * a.pitch;
    const int nseg = (W + 63) / 64;
    const bool interp = a.mode == kFillInterpolate;
    const int span = select_span(a.min_disp, a.D, a.scale);
    // E candidates, right to left (lane j alone writes and later reads e_row[j])
    float carry = fill_none();
    for (int s = nseg - 1; s >= 0; --s) {
        const int j = s * 64 + lane;
        const float v = j < W ? row[j] : fill_none();
        const unsigned long long m = __ballot(j < W && fill_valid(v, a.lim));
        const unsigned long long above = lane == 63 ? 0ull : m & (~0ull << (lane + 1));
        const float got = __shfl(v, above ? __builtin_ctzll(above) : lane);
        if (j < W) e_row[j] = above ? got : carry;
        if (m) carry = __shfl(v, __builtin_ctzll(m));
    }
    carry = fill_none();
    for (int s = 0; s < nseg; ++s) {
        const int j0 = s * 64, j = j0 + lane;
        const float v = j < W ? row[j] : fill_none();
        const bool ok = j < W && fill_valid(v, a.lim);
        const unsigned long long m = __ballot(ok);
        const int lo = j0 - span > 0 ? j0 - span : 0, hi = j0 + 63 < W - 1 ? j0 + 63 : W - 1;
        if (interp) {
            __syncthreads();  // (the span of the segment before is read no more)
            const float *r = a.right + (long long)i * a.rs;
            for (int c = lo + lane; c <= hi; c += 64) r_span[c - lo] = r[(long long)c * a.cs];
            __syncthreads();
        }
        const unsigned long long below = m & ((1ull << lane) - 1);
        const float got = __shfl(v, below ? 63 - __builtin_clzll(below) : lane);
        const float w = below ? got : carry;
        if (m) carry = __shfl(v, 63 - __builtin_clzll(m));
        if (j < W) {
            float out = v;
            uint8_t code = kFillMeasured;
            if (!ok) {
                const size_t px = (size_t)i * W + j, np = (size_t)a.H * W;
                float c[8] = {w, e_row[j]};
#pragma unroll
                for (int p = 0; p < kFillPlanes; ++p) c[2 + p] = a.planes[p * np + px];
                const bool mis = interp && fill_mismatch([&](int jr) { return r_span[jr - lo]; }, j, a.min_disp,
                                                         a.D, a.scale, a.lim, a.lr_max_diff);
                out = fill_pick(c, a.lim, mis, a.inv, &code);
            }
            row[j] = out;
            a.mask[(size_t)i * a.mask_pitch + j] = code;
        }
    }
}

constexpr size_t kSelectLdsMax = 64 * 1024;

size_t select_lds_bytes(int W, int min_disp, int D, int scale) {
    return ((size_t)W + 64 + select_span(min_disp, D, scale)) * sizeof(float);
}

}  // namespace
}  // namespace sgm

using namespace sgm;

namespace {

void free_fill(sgm_handle *h) {
    dfree(h, &h->d_fill_planes);
    dfree(h, &h->d_fill_mask);
    h->fill_mask_valid = false;
}

const char *mode_refusal(int mode) {
    return mode == kFillBackground || mode == kFillInterpolate
               ? nullptr
               : "mode must be SGM_FILL_BACKGROUND or SGM_FILL_INTERPOLATE";
}

}  // namespace

// The two launches, in place on d_map (a true-disparity map).  d_right, rs, cs: the right view's
// map by row and column strides (interpolate; else not read); d_mask: where the mask goes.
int sgm::fill_map(sgm_handle *h, float *d_map, int pitch, const float *d_right, long long rs, long long cs,
                  int mode, uint8_t *d_mask, int mask_pitch, hipStream_t st) {
    const Geom g = h->gt;  // (valid <= D + min_disp - 1, invalid D + min_disp + 1)
    const double npx = (double)g.H * g.W;
    const float lim = (float)(g.D - 1);
    MarchArgs ma{d_map, h->d_fill_planes, pitch, g.H, g.W, lim};
    HIPCHK(h, timed(h, "fill_march", kFillPlanes * npx, st, [&] {
               hipLaunchKernelGGL(fill_march_kernel, dim3((unsigned)((g.H + g.W - 1 + 63) / 64), kFillPlanes), dim3(64),
                                  0, st, ma);
               return hipGetLastError();
           }));
    SelectArgs sa{};
    sa.map = d_map;
    sa.planes = h->d_fill_planes;
    sa.right = d_right;
    sa.mask = d_mask;
    sa.rs = rs;
    sa.cs = cs;
    sa.pitch = pitch;
    sa.mask_pitch = mask_pitch;
    sa.H = g.H;
    sa.W = g.W;
    sa.mode = mode;
    sa.min_disp = h->min_disp;
    sa.D = h->g.D;
    sa.scale = g.scale;
    sa.lim = lim;
    sa.inv = (float)(g.D + 1);
    sa.lr_max_diff = h->p.lr_max_diff;
    const size_t lds = select_lds_bytes(g.W, h->min_disp, h->g.D, g.scale);
    HIPCHK(h, timed(h, "fill_select", npx, st, [&] {
               hipLaunchKernelGGL(fill_select_kernel, dim3((unsigned)g.H), dim3(64), lds, st, sa);
               return hipGetLastError();
           }));
    return SGM_OK;
}

int sgm::fill_frame(sgm_handle *h, float *d_map, int pitch, hipStream_t st) {
    const bool interp = h->fill_mode == kFillInterpolate;
    const bool cm = h->plan.sub_cm != 0;  // (the handle's layout of d_sub[1])
    if (int rc = fill_map(h, d_map, pitch, interp ? h->d_sub[1] : nullptr, cm ? 1 : h->g.W, cm ? h->g.H : 1,
                          h->fill_mode, h->d_fill_mask, h->g.W, st))
        return rc;
    h->fill_mask_valid = true;
    return SGM_OK;
}

extern "C" {

int sgm_set_fill(sgm_handle *h, int mode) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (mode != kFillOff && mode_refusal(mode))
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_fill: mode must be SGM_FILL_OFF, SGM_FILL_BACKGROUND or SGM_FILL_INTERPOLATE, got %d", mode);
    if (mode != kFillOff && h->p.view == SGM_VIEW_RIGHT)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_fill: a SGM_VIEW_RIGHT handle (the fill works on the left view's map)");
    // (an aux_only handle runs no frames: either mode gives it the scratch of sgm_fill_device)
    if (mode == kFillInterpolate && !h->p.aux_only && (h->p.solver != SGM_SOLVER_SGM || h->nviews != 2))
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_set_fill: SGM_FILL_INTERPOLATE needs the right view's map of a two-view SGM handle; "
                       "one-view and BM handles serve SGM_FILL_BACKGROUND");
    if (mode != kFillOff && select_lds_bytes(h->g.W, h->min_disp, h->g.D, h->g.scale) > kSelectLdsMax)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_set_fill: the select kernel stages a row in LDS; %d columns are too many",
                       h->g.W);
    // (frames in flight still write the planes and the mask)
    return change_setting(h, "sgm_set_fill", mode == h->fill_mode, [&]() -> int {
        if (mode == kFillOff) {
            free_fill(h);
        } else if (!h->d_fill_planes) {
            const size_t npx = (size_t)h->g.H * h->g.W;
            Ledger::Group scratch(h->mem);
            if (int rc = dalloc(h, &h->d_fill_planes, kFillPlanes * npx)) return rc;
            if (int rc = dalloc(h, &h->d_fill_mask, npx)) return rc;
            scratch.commit();
        }
        h->fill_mode = mode;
        return SGM_OK;
    });
}

int sgm_get_fill(const sgm_handle *h, int *mode) {
    if (!h || !mode) return SGM_ERR_INVALID_ARG;
    *mode = h->fill_mode;
    return SGM_OK;
}

int sgm_fill_device(sgm_handle *h, float *d_disp, int pitch, const float *d_right, int right_pitch, int mode,
                    uint8_t *d_mask, int mask_pitch, void *stream) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (const char *why = mode_refusal(mode)) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_fill_device: %s, got %d", why, mode);
    if (!h->d_fill_planes)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_fill_device: the handle has no fill scratch (sgm_set_fill)");
    if (!d_disp || pitch < h->g.W || (d_mask && mask_pitch < h->g.W) || (d_right && right_pitch < h->g.W))
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_fill_device: bad pointer or pitch");
    if (stream == (void *)hipStreamLegacy)
        return set_err(h, SGM_ERR_INVALID_ARG,
                       "sgm_fill_device: hipStreamLegacy is not accepted; pass a created stream, or NULL for the handle's own");
    if (select_lds_bytes(h->g.W, h->min_disp, h->g.D, h->g.scale) > kSelectLdsMax)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_fill_device: min_disp grew the right view's span past the LDS");
    long long rs = right_pitch, cs = 1;
    if (mode == kFillInterpolate) {
        if (d_right == d_disp)
            return set_err(h, SGM_ERR_INVALID_ARG, "sgm_fill_device: d_right must not alias d_disp (the fill is in place)");
        if (!d_right) {  // this handle's last frame's right view, in the handle's layout
            if (h->p.aux_only || h->p.solver != SGM_SOLVER_SGM || h->nviews != 2)
                return set_err(h, SGM_ERR_INVALID_ARG,
                               "sgm_fill_device: d_right = NULL means the right view of a two-view SGM handle's last "
                               "frame; this handle keeps none");
            d_right = h->d_sub[1];
            rs = h->plan.sub_cm ? 1 : h->g.W;
            cs = h->plan.sub_cm ? h->g.H : 1;
        }
    }
    DeviceGuard guard(h->device);
    StreamScope scope(h, stream);
    if (int rc = sgm::fill_map(h, d_disp, pitch, d_right, rs, cs, mode, d_mask ? d_mask : h->d_fill_mask,
                               d_mask ? mask_pitch : h->g.W, scope.st))
        return rc;
    if (!d_mask) h->fill_mask_valid = true;
    return SGM_OK;
}

int sgm_stage_fill(sgm_handle *h, float *disp, const float *right, int mode, uint8_t *mask) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!disp) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_fill: NULL map");
    if (!h->d_fill_planes)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_fill: the handle has no fill scratch (sgm_set_fill)");
    const size_t npx = (size_t)h->g.H * h->g.W;
    Staging s(h);
    // staging: the map in d_out, the right view's in the post filter's working map (dead between calls)
    s.up(h->d_out, disp, npx * sizeof(float));
    if (right) s.up(h->d_pf_work, right, npx * sizeof(float));
    const float *d_right = right ? h->d_pf_work : nullptr;
    s.run([&] { return sgm_fill_device(h, h->d_out, h->g.W, d_right, h->g.W, mode, nullptr, 0, nullptr); });
    s.down(disp, h->d_out, npx * sizeof(float));
    if (mask) s.down(mask, h->d_fill_mask, npx);
    return s.finish();
}

int sgm_get_fill_mask(sgm_handle *h, const uint8_t **d_mask, int *pitch) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!d_mask || !pitch) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_get_fill_mask: NULL pointer");
    if (!h->d_fill_mask || !h->fill_mask_valid)
        return set_err(h, SGM_ERR_INVALID_ARG, "sgm_get_fill_mask: no map has been filled since fill was set (sgm_set_fill)");
    *d_mask = h->d_fill_mask;
    *pitch = h->g.W;
    return SGM_OK;
}

int sgm_stage_fill_mask(sgm_handle *h, uint8_t *mask) {
    if (!h) return SGM_ERR_INVALID_ARG;
    if (!mask) return set_err(h, SGM_ERR_INVALID_ARG, "sgm_stage_fill_mask: NULL pointer");
    const uint8_t *d_mask = nullptr;
    int pitch = 0;
    if (int rc = sgm_get_fill_mask(h, &d_mask, &pitch)) return rc;
    Staging s(h);
    s.down(mask, d_mask, (size_t)h->g.H * h->g.W);
    return s.finish();
}

}  // extern "C"
