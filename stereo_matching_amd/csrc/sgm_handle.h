// sgm_handle.h -- the handle behind include/sgm_hip.h and the host helpers
// every function that works on it uses: shared by the C-ABI (sgm_create.hip,
// sgm_capi.hip, sgm_stages.hip, and sgm_input.hip for the input stage) and the frame schedules (sgm_frame.hip).
// The handle holds the plan sgm_create made for it (sgm_plan.h: the schedule
// of its frames) once, as `plan`.
// Host-only; not part of the public interface.
#pragma once

#include "../../include/sgm_hip.h"
#include "sgm_input_stage.h"
#include "sgm_internal.h"
#include "sgm_ledger.h"
#include "sgm_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>

using sgm::Geom;
using sgm::SweepArgs;
using sgm::vol_elems;

struct __attribute__((visibility("hidden"))) sgm_handle {  // (its inline members stay out of the exported symbols)
    sgm_params p;
    sgm::HandlePlan plan; // the schedule of the handle's frames (plan_handle, sgm_plan.h)
    Geom g;               // plan.g
    Geom gt;              // g with D + min_disp for D: the geometry of every stage that works on
                          // true-disparity maps (LR check, post filter, LKRefine, confidence
                          // filter, point cloud: valid <= D+m-1, invalid D+m+1)
    int device;
    int nviews;           // plan.nviews
    sgm::Ledger mem{[](void **p, size_t n) { return (int)hipMalloc(p, n); }, [](void *p) { (void)hipFree(p); }};
                          // every live dalloc and its size (sgm_device_bytes: their sum), in device memory
    hipStream_t st;      // the handle's own stream (host API, stages)
    hipEvent_t ev_pf;     // the post filter's convergence readback
    hipEvent_t ev_last;   // the end of the last call's work on last_st (StreamScope)
    hipStream_t last_st;  // the stream of the last entry point's work (null: none yet)
    bool last_recorded;   // ev_last was recorded at the end of that call (a caller's stream)
    uint8_t *d_in[2];     // full-size input staging (host API)
    sgm::InputStage in;   // the input size, the maps' source size and the pixel format frames take
                          //   (sgm_input_stage.h; all off: frames read the caller's images)
    uint8_t *d_rs[2];     //   the full-size grey images the frame's first launch writes (left, right)
    uint8_t *d_raw[2];    //   staging of the raw images (host API): cols x bytes per pixel per row
    bool rs_valid;        //   a frame has filled d_rs since a setter last changed the stage
    uint32_t *d_map[2];   //   each view's packed map, two words per full-size pixel (sgm_rectify_maps.h;
                          //   aux_only handles: the maps alone, for sgm_remap_device)
    std::vector<uint8_t> valid[2];  //   each view's valid mask (host, full size, dense)
    size_t raw_bytes;     // bytes of each d_raw (0: none): what fit_input_buffers compares, sgm_input.hip
    uint8_t *d_sky[2];    // working-grid sky masks (host API / stages)
    uint64_t *d_ct[2];    // census words
    int min_disp;         // sgm_set_min_disp: index d of the volumes stands for disparity min_disp + d
    sgm::Window win;      // sgm_set_window over the scale: the census's and the window costs' window
    int win_h, win_w;     //   as set (the reference's WIN_H, WIN_W: 7, 9)
    float weights[sgm::kWinMax * sgm::kWinMax];  // sgm_set_weighted (win.weighted): window_weights' table of
                          //   win, rebuilt by the setters; read by the weighted producer's launches
    int cost_kind;        // sgm_set_cost: SGM_COST_CENSUS (frames as ever), or the SAD / SSD / CT window cost
                          //   (frames: window_cost_stage + volume_frame, sgm_frame.hip)
    int vol_filter;       // sgm_set_volume_filter: the cost filters (SGM_FILTER_H | SGM_FILTER_V) every
                          //   volume frame runs on each view's volume (aggregate_volume, SAD / SSD
                          //   frames: volume_frame, sgm_frame.hip); 0: none
    uint64_t *d_cts[2];   // the tables shifted by min_disp / scale columns (launch_ct_shift):
                          // [0] the left image's (the right view's DSI reads it), [1] the right
                          // image's (the left view's); min_disp = 0: d_ct[0], d_ct[1] themselves
    float *d_ch[2];       // horizontally filtered cost; reused as the T chain
    float *d_ch_base[2];  // its allocation: d_ch is preceded by t_guard_rows rows (final pass)
    float *d_c[2];        // final cost volume (+ kVolGuard: row-walking prefetch rings)
    float *d_s[2];        // S chain
    uint16_t *d_disp[2];  // WTA disparity
    float *d_sub[2];      // sub-pixel disparity
    float *d_ratio[2];    // match confidence min / second-min (sgm_set_confidence; null: off)
    bool ratio_cm[2];     //   the last final pass stored it column-major (as its sub-pixel map)
    float *d_out;         // LR-checked output (host API)
    float *d_min;         // minL (stage_path)
    float *d_zero;        // 256 zero floats (PairArgs::zero)
    float *d_ck[2][3];    // checkpoints per view and pair family (H, V, D2)
    float *d_carry[2][3]; // banded backward passes: chain state at band edges (L7, L8, L4)
    float *d_l3[2];       // slant (plan.slant): the full L3 volume per view
    unsigned long long *d_gran;  // slant: hand-off granules (both views)
    sgm::SlantCtl *d_slant_ctl;  // slant: launch bookkeeping of the passes
    float *d_slant_dummy;        // slant: the target of inactive lanes' stores
    int mf_rows;          // median fill tile rows (4 or 8 by frame size; SGM_MF_ROWS)
    // post_filter scratch (sgm_post.hip)
    float *d_pf_orig;     // the map as it entered the median fill
    float *d_pf_work;     // contiguous working map (pitched callers)
    int *d_pf_label;      // union-find parents
    int *d_pf_count;      // pixels under each tile-local root
    int *d_pf_area;       // component sizes
    float *d_pf_snap;     // per median tile: the working-map cells it last read
    int *d_pf_changes;    // per median launch: tiles that changed a pixel
    int *h_pf_changes;    // pinned readback of one counter
    unsigned *h_pf_err;   // host-mapped word: the budget of a fixed-budget fill that was not proven (0: none)
    unsigned *d_pf_err;   //   its device-side address (pf_verdict_kernel)
    int pf_launches;      // sgm_set_post_filter_launches: 0 = adaptive, else the fixed budget
    unsigned *h_slant_err;  // slant: host-mapped hang-guard word (SlantArgs::err_host)
    hipStream_t st_h;       // slant: the H pair's stream, beside the top-down pass
    hipEvent_t ev_fork, ev_join;  //   its fork from / join into the frame's stream
    unsigned *d_slant_err;  //   its device-side address
    int pf_iters;         // median launches of the last post filter
    float *d_lk_in;       // LKRefine input copy (the kernel refines the map in place)
    uint8_t *d_sky_scratch;  // sky detector scratch (sgm_sky.hip)
    int *d_cloud_counts;  // point cloud: per-row counts -> offsets, then the total
    sgm_reproject rp;     // sgm_set_reproject: Q, the products a frame writes, the range and the scale
    bool rp_on;           //   rp is set (off: frames end as before, sgm_reproject_device refuses)
    bool rp_valid;        //   a frame has filled the products since the setter last changed them
    int rp_form;          //   the XYZ store form (sgm_reproject.hip; SGM_REPROJECT_STORE picks the other)
    float *d_rp_xyz;      //   the frame's products (null: not asked for): rows x cols x 3 f32,
    float *d_rp_depth;    //   rows x cols f32,
    uint16_t *d_rp_d16;   //   rows x cols u16
    int fill_mode;        // sgm_set_fill: SGM_FILL_OFF, or the hole filling every frame ends its maps with
                          //   (sgm_fill.hip)
    float *d_fill_planes; //   its scratch (null: off): six rows x cols planes of directional candidates,
    uint8_t *d_fill_mask; //   and the rows x cols fill mask of the last filled map
    bool fill_mask_valid; //   a fill has written the mask since the scratch was allocated
    uint8_t *h_pin;       // pinned host staging for sgm_process (allocated on first use)
    size_t h_pin_bytes;
    char err[512];
    // profiling (sgm_set_profiling)
    int profiling;
    std::vector<hipEvent_t> ev_pool;
    struct Pending { int cls; double elems; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<sgm_kernel_stat> stats;
    std::vector<double> stat_elems;  // elements of the class's launches since the last readout
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Every entry point's work shares the handle's scratch (cost volumes,
// checkpoints, post-filter and LKRefine buffers), whichever stream the caller
// passes.
// Orders calls on different streams (they share the handle's scratch).  A
// call on a CALLER's stream records ev_last on that stream as it returns,
// while the stream certainly exists (a rocprof trace shows the record as a
// ~5 us gap before the next kernel; frame loops can run on the handle's own
// stream, sgm_get_stream, instead); a call on the handle's own stream
// records nothing (the same-stream path stays free of event records) and a later
// call on another stream records ev_last on the handle's stream, which the
// handle owns.  So no stream handle of the caller is kept past the call that
// used it.  Entry points construct the scope after their argument checks, so
// a call rejected before enqueueing anything leaves the state untouched.
struct StreamScope {
    sgm_handle *h;
    hipStream_t st;
    StreamScope(sgm_handle *handle, void *stream)
        : h(handle), st(stream ? (hipStream_t)stream : handle->st) {
        if (h->last_st && h->last_st != st) {
            if (h->last_recorded)
                (void)hipStreamWaitEvent(st, h->ev_last, 0);
            else if (hipEventRecord(h->ev_last, h->last_st) == hipSuccess)
                (void)hipStreamWaitEvent(st, h->ev_last, 0);
        }
    }
    ~StreamScope() {
        h->last_st = st;
        h->last_recorded = st != h->st && hipEventRecord(h->ev_last, st) == hipSuccess;
    }
};

inline int set_err(sgm_handle *h, int code, const char *fmt, ...) {
    if (h) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(h->err, sizeof(h->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(h, expr)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err((h), e_ == hipErrorOutOfMemory ? SGM_ERR_OUT_OF_MEMORY : SGM_ERR_HIP, \
                           "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,   \
                           __LINE__);                                                        \
    } while (0)

// sgm_capi.hip, shared by the C-ABI's files and kept out of the library's exported symbols: the
// wait for the last call's work; a frame's give-up (hang guard, unproven fill) reported and cleared.
__attribute__((visibility("hidden"))) int wait_last(sgm_handle *h);
__attribute__((visibility("hidden"))) int check_frame_err(sgm_handle *h);

// What every setter that reallocates buffers does after its argument checks:
// refuse inside a stream capture (`fn`: the setter's name, for the message),
// return at once when nothing changes, else wait for the frames in flight
// (they still read what `apply` frees or replaces) and apply.
template <typename F>
int change_setting(sgm_handle *h, const char *fn, bool unchanged, F &&apply) {
    DeviceGuard guard(h->device);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(h, hipStreamIsCapturing(h->st, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return set_err(h, SGM_ERR_INVALID_ARG, "%s: call it outside stream capture", fn);
    if (unchanged) return SGM_OK;
    if (int rc = wait_last(h)) return rc;
    return apply();
}

// STAGE_HIP(s, call): a HIP call as a step of the Staging `s`, its failure reported as HIPCHK's.
#define STAGE_HIP(s, expr) (s).run([&]() -> int { HIPCHK((s).h, expr); return SGM_OK; })

// The host round trip of a sgm_stage_* function: the device guard, the scope on the handle's own
// stream (a _device call made inside opens its own on the same stream: intended, it orders nothing
// anew), uploads, stream-ordered temporaries (freed on every return path), the stage's work,
// downloads, the final synchronise.  The first error sticks: later steps are skipped, finish() returns it.
struct __attribute__((visibility("hidden"))) Staging {
    sgm_handle *h;
    DeviceGuard guard;
    StreamScope scope;
    int rc = SGM_OK;
    std::vector<void *> temps;  // hipMallocAsync'ed
    explicit Staging(sgm_handle *handle) : h(handle), guard(handle->device), scope(handle, nullptr) {}
    ~Staging() { for (void *p : temps) (void)hipFreeAsync(p, h->st); }
    // the stage's work: a _device call or another step that returns an rc, with h->err its own
    template <typename F>
    void run(F &&work) { if (!rc) rc = work(); }
    // `count` elements that live until the round trip ends (null after an error)
    template <typename T>
    T *temp(size_t count) {
        void *p = nullptr;
        STAGE_HIP(*this, hipMallocAsync(&p, count * sizeof(T), h->st));
        if (p) temps.push_back(p);
        return (T *)p;
    }
    void up(void *d_dst, const void *src, size_t bytes) {
        STAGE_HIP(*this, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->st));
    }
    // rows of row_bytes, `pitch` apart on the host, dense on the device
    void up_rows(void *d_dst, const void *src, size_t row_bytes, size_t rows, size_t pitch) {
        STAGE_HIP(*this, hipMemcpy2DAsync(d_dst, row_bytes, src, pitch, row_bytes, rows, hipMemcpyHostToDevice, h->st));
    }
    void down(void *dst, const void *d_src, size_t bytes) {
        STAGE_HIP(*this, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->st));
    }
    void sync() { STAGE_HIP(*this, hipStreamSynchronize(h->st)); }
    int finish() {
        if (rc) (void)hipStreamSynchronize(h->st);  // (what was enqueued before the error still reads host memory)
        sync();
        return rc;
    }
};

// count elements of device memory on the handle's ledger (0: null, nothing allocated)
template <typename T>
int dalloc(sgm_handle *h, T **p, size_t count) {
    const int e = h->mem.alloc((void **)p, count * sizeof(T));  // (hipMalloc's code; the text is HIPCHK's of it)
    if (e == hipSuccess) return SGM_OK;
    return set_err(h, e == hipErrorOutOfMemory ? SGM_ERR_OUT_OF_MEMORY : SGM_ERR_HIP, "hipMalloc((void **)p, count * sizeof(T)) "
                   "failed: %s (%s:%d)", hipGetErrorString((hipError_t)e), __FILE__, __LINE__);
}

// Frees a dalloc and nulls the pointer (null: nothing).
template <typename T>
void dfree(sgm_handle *h, T **p) {
    h->mem.free((void **)p);
}

// The profile names of the two launches sgm_set_weighted changes: the masked
// census where the disc drops a tap of the window (else the launch is the unmasked kernel's),
// and the weighted producer.
inline const char *census_name(const sgm_handle *h) {
    const sgm::Window w = h->win;
    return w.weighted && sgm::weighted_bits(w.hh(), w.hw()) < w.bits() ? "census_masked" : "census";
}
inline const char *window_cost_name(const sgm_handle *h, int kind) {
    // (CT's weighting is a mask in the launch's arguments: one kernel, one class)
    if (kind == sgm::kCostCt) return "window_cost_ct";
    return h->win.weighted ? "window_cost_weighted" : "window_cost";
}

inline hipEvent_t pool_event(sgm_handle *h) {
    if (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

inline int stat_class(sgm_handle *h, const char *name, double elems) {
    for (size_t k = 0; k < h->stats.size(); ++k)
        if (!strncmp(h->stats[k].name, name, sizeof(h->stats[k].name))) return (int)k;
    sgm_kernel_stat st{};
    snprintf(st.name, sizeof(st.name), "%s", name);
    st.elems = elems;
    h->stats.push_back(st);
    h->stat_elems.push_back(0.0);
    return (int)h->stats.size() - 1;
}

// Launch `fn` on `st`; with profiling on, bracket it with pooled events.
template <typename F>
hipError_t timed(sgm_handle *h, const char *name, double elems, hipStream_t st, F &&fn) {
    if (!h->profiling) return fn();
    hipEvent_t a = pool_event(h), b = pool_event(h);
    if (!a || !b) return hipErrorOutOfMemory;
    hipError_t e = hipEventRecord(a, st);
    if (e == hipSuccess) e = fn();
    if (e == hipSuccess) e = hipEventRecord(b, st);
    h->pending.push_back({stat_class(h, name, elems), elems, a, b});
    return e;
}

// Upper bound on median-fill launches of one post filter: the fill reaches its
// fixed point in 2-3 launches on stereo output; the bound only stops a runaway.
constexpr int kMedianMaxLaunches = 4096;

inline SweepArgs sweep_args(const sgm_handle *h) {
    SweepArgs a{};
    a.p1 = (float)h->p.p1;
    a.p2 = (float)h->p.p2;
    return a;
}

inline sgm::PairArgs pair_args(const sgm_handle *h) {
    sgm::PairArgs a{};
    a.zero = h->d_zero;
    a.p1 = (float)h->p.p1;
    a.p2 = (float)h->p.p2;
    a.uniq = h->p.uniqueness;
    a.min_disp = h->min_disp;
    return a;
}

// vfwd's arguments for a view: the L3 checkpoints it writes
inline sgm::PairArgs vfwd_args(const sgm_handle *h, int view) {
    sgm::PairArgs a = pair_args(h);
    a.ckpt = h->d_ck[view][sgm::PAIR_V];
    return a;
}

// the view's final cost volume C and its T chain (T reuses the horizontally
// filtered volume, dead once vfwd has read it; an in-place vfwd with T in the
// second volume measured no faster, profiles/r03_experiments/inplace_c.txt)
inline float *cost_buf(sgm_handle *h, int v) { return h->d_c[v]; }
inline float *t_buf(sgm_handle *h, int v) { return h->d_ch[v]; }

// One frame's device buffers, as sgm_process_device takes them.
struct FrameIO {
    const uint8_t *left, *right;  // full-size images (camera-size images with an input size or maps set)
    int pitch;
    const uint8_t *sky_l, *sky_r;  // working-grid sky masks (null: none)
    int sky_pitch;
    float *out;                   // the frame's map
    int out_pitch;
    uint16_t *raw;                // the left view's raw WTA map (null: not wanted)
};

// sgm_frame.hip: what the C-ABI calls into it
namespace sgm {
int run_frame(sgm_handle *h, FrameIO f, hipStream_t st);
int post_filter(sgm_handle *h, float *d_map, int pitch, hipStream_t st, bool to_lk = false);
int lk_refine(sgm_handle *h, const uint8_t *d_left, const uint8_t *d_right, int pitch,
              float *d_map, int map_pitch, hipStream_t st, bool staged = false);
// the cost stage's view slots (sgm_internal.h) and the shifted tables they read
sgm::CostSlot cost_slot(sgm_handle *h, int slot, int dsi, const uint8_t *sky);
int shift_tables(sgm_handle *h, const sgm::CostSlot *s, int nviews, hipStream_t st);
// one view's vfwd launch (profile class "vfwd" over `elems`): in -> out, the L3 checkpoints into
// the view's; band: forward_bands' rows (default: the whole volume)
int vfwd_view(sgm_handle *h, int view, const float *in, float *out, double elems, hipStream_t st,
              sgm::Band band = {});
// sgm_stage_aggregate: view 0's aggregation from the final cost volume in
// d_c[0], whole-volume passes on every handle, into d_disp[0] and d_sub[0]
int stage_aggregate(sgm_handle *h, hipStream_t st);
// sgm_aggregate_device: the frame from the cost volume on: the caller's volume
// imported into every view's C, stage_aggregate's whole-volume passes view after view (both at
// once on a 4-path handle), then the LR check, post_filter and the output slot as run_frame's
// (the tail a SAD / SSD frame shares: volume_frame, sgm_frame.hip)
int aggregate_volume(sgm_handle *h, const sgm_volume &vol, float *d_out, int out_pitch, uint16_t *d_raw,
                     hipStream_t st);
// sgm_filter_volume_device: the cost filters `filters` in place on a caller's dense fp32 HWD volume
// (the horizontal filter alone runs in it; with the vertical one, view 0's Ch is the scratch)
int filter_volume(sgm_handle *h, float *d_cost, int filters, hipStream_t st);
// the device's CU count (the plan's and the slanted passes' grids)
int slant_cus();
// sgm_reproject.hip: the frame's last launch on a handle with reprojection set
// (the products of the frame's map into the handle's buffers)
int reproject_frame(sgm_handle *h, const float *d_map, int pitch, hipStream_t st);
// sgm_fill.hip: the hole filling, two launches in place on a true-disparity map:
// fill_frame as the frame's last map stage on a handle with fill set (the right view's map is the
// handle's d_sub[1], the mask the handle's); fill_map with the right view's map by row and column
// strides in elements (SGM_FILL_INTERPOLATE; else not read) and the mask's destination
int fill_frame(sgm_handle *h, float *d_map, int pitch, hipStream_t st);
int fill_map(sgm_handle *h, float *d_map, int pitch, const float *d_right, long long rs, long long cs, int mode,
             uint8_t *d_mask, int mask_pitch, hipStream_t st);
}  // namespace sgm
