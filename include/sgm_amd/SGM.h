/*
 * sgm_amd/SGM.h -- the reference's Solver / SGM class surface over the C-ABI.
 *
 * Same class names, signatures, ownership and error behaviour as the
 * reference (inc/Solver.h:23-70, inc/SGM.h:10-26), so the ROS node
 * (node.cpp:49,93,104,107) compiles against this header unchanged; the work
 * runs in libsgm_hip.so (include/sgm_hip.h) on one MI355X.  Header-only,
 * C++11.
 *
 *   SGM(h, w, s, d)              Solver.cpp:4-16   (asserts: h,w,s,d > 0,
 *                                s in {1,2}, d in {32,64,128} -- widened to 256)
 *   SGM(h, w, s, d, paths)       inc/SGM.h:7        (paths = 4: USE_8_PATH = false; 8: as above)
 *   SGM(h, w, s, d, paths, m)    (not in the reference) min_disp = m: disparities [m, m + d)
 *                                are searched, get_disp() is in true disparity and
 *                                invalid = d + m + 1 (get_invalid_disp()); a sky pixel
 *                                reports m; BM takes no min_disp (sgm_set_min_disp)
 *   process(l, r)                SGM.cpp:32-826     (LR-checked, post-filtered)
 *   process(l, r, sky, sky_b)    SGM.cpp:829-834    (masks kept as members)
 *   BM(h, w, s, d)               BM.cpp:4-97        (filtered-cost WTA, post-filtered)
 *   get_disp()                   Solver.h:36        (CV_32FC1, invalid = d+1)
 *   set_post_filter_launches(n)  (not in the reference) post_filter without host waits
 *   resize(src, dst)             node.cpp:75-76     cv::resize(src, dst, Size(w, h)) on the GPU
 *   set_input_size(rows, cols)   (not in the reference) process() takes rows x cols images
 *                                and resizes them on the GPU first
 *   set_rectify(rows, cols, xl, yl, xr, yr)  (not in the reference) process() takes raw
 *                                rows x cols camera images and rectifies them on the GPU
 *                                first: cv::remap through initUndistortRectifyMap's maps
 *   remap(src, dst, view)        cv::remap(src, dst, map_x, map_y, INTER_LINEAR) on the GPU
 *   set_input_format(fmt)        (not in the reference) process() takes CV_8UC3 / CV_8UC4 colour
 *                                images (SGM_PIX_BGR8, ...) and converts them on the GPU first
 *   gray(src, dst, fmt)          node.cpp:69-70     the decoder's / cvtColor's grey conversion
 *                                on the GPU, Y = (4899 R + 9617 G + 1868 B + 8192) >> 14
 *   input_gray(view)             the grey image the last process() matched
 *   set_fill(mode)               (not in the reference) every process() fills its map's holes
 *   set_reproject(q, outputs)    (not in the reference) every process() also reprojects its map
 *                                through stereoRectify's Q on the GPU: xyz() (CV_32FC3, what
 *                                cv::reprojectImageTo3D gives), depth() (CV_32FC1), depth16()
 *                                (CV_16UC1, REP 118's millimetres); reproject(disp, ...) on any map
 *   aggregate_device(vol, ...)   (not in the reference) a caller's DEVICE cost volume through the
 *                                path aggregation, the LR check and post_filter (sgm_aggregate_device);
 *                                import_volume_device(vol, view, dst) is its first launch alone
 *   set_cost(kind), cost()       Solver.cpp:96-117 over cost.cpp:4-96: frames match on the SAD or
 *                                SSD window cost, or on CT (SGM_COST_CT, build_dsi's own
 *                                per-disparity census), instead of the census (sgm_set_cost);
 *                                window_cost_device(kind, l, r, pitch, dst) is that volume alone
 *   set_volume_filter(bits)      Solver.cpp:296-368 on each view's volume of every volume frame
 *                                (sgm_set_volume_filter); filter_volume_device(d_cost, bits) is
 *                                the two filters alone, in place
 *   set_window(win_h, win_w)     inc/Solver.h:10-11  WIN_H, WIN_W as a setting of SGM and BM: the
 *                                census's and the window costs' window (sgm_set_window)
 *   set_weighted(on), weighted() inc/Solver.h:15     WEIGHTED_COST as a setting: Gaussian SAD / SSD
 *                                taps, the census masked to a disc (sgm_set_weighted);
 *                                window_weights() is Solver.cpp:29-45's table
 *   show_disp(view)              Solver.cpp:55-93   (2h x w BGR, colormap :652-707)
 *
 * Mat is cv::Mat when OpenCV's core header is included first (or
 * SGM_AMD_USE_OPENCV is defined); otherwise a minimal row-major stand-in with
 * the members the class surface uses.  Errors abort with a message, like the
 * reference's asserts (define SGM_AMD_THROW to get std::runtime_error).
 */
#ifndef SGM_AMD_SGM_H
#define SGM_AMD_SGM_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sgm_hip.h"

#if defined(SGM_AMD_USE_OPENCV) || defined(OPENCV_CORE_HPP) || defined(__OPENCV_CORE_HPP__)
#include <opencv2/core/core.hpp>
namespace sgm_amd {
using cv::Mat;
typedef cv::Vec3b Vec3b;
}  // namespace sgm_amd
#define SGM_AMD_HAVE_OPENCV 1
#else
#ifndef CV_8UC1
#define CV_8UC1 0
#endif
#ifndef CV_32FC1
#define CV_32FC1 5
#endif
#ifndef CV_8UC3
#define CV_8UC3 16
#endif
#ifndef CV_16UC1
#define CV_16UC1 2
#endif
#ifndef CV_32FC3
#define CV_32FC3 21
#endif
#ifndef CV_8UC4
#define CV_8UC4 24
#endif
namespace sgm_amd {
struct Vec3b {
    unsigned char v[3];
    unsigned char &operator[](int i) { return v[i]; }
    const unsigned char &operator[](int i) const { return v[i]; }
};
// Minimal cv::Mat stand-in: shallow copies share the buffer (as cv::Mat).
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step = 0;  // bytes per row
    unsigned char *data = nullptr;

    Mat() = default;
    Mat(int r, int c, int t) { create(r, c, t); }
    void create(int r, int c, int t) {
        if (r == rows && c == cols && t == type_ && data) return;
        rows = r;
        cols = c;
        type_ = t;
        step = (size_t)c * elem_size(t);
        buf_.reset(new unsigned char[(size_t)r * step](), std::default_delete<unsigned char[]>());
        data = buf_.get();
    }
    void release() {
        buf_.reset();
        data = nullptr;
        rows = cols = 0;
        step = 0;
    }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    int type() const { return type_; }
    int channels() const { return type_ == CV_8UC3 || type_ == CV_32FC3 ? 3 : (type_ == CV_8UC4 ? 4 : 1); }
    Mat clone() const {  // packed copy (step = cols * elem), row by row as cv::Mat::clone
        Mat m(rows, cols, type_);
        for (int i = 0; i < rows && !empty(); ++i)
            std::memcpy(m.data + (size_t)i * m.step, data + (size_t)i * step, m.step);
        return m;
    }
    template <typename T> T *ptr(int i) { return reinterpret_cast<T *>(data + (size_t)i * step); }
    template <typename T> const T *ptr(int i) const {
        return reinterpret_cast<const T *>(data + (size_t)i * step);
    }
    template <typename T> T &at(int i, int j) { return ptr<T>(i)[j]; }
    template <typename T> const T &at(int i, int j) const { return ptr<T>(i)[j]; }

private:
    static size_t elem_size(int t) {
        return t == CV_32FC3 ? 12 : t == CV_32FC1 || t == CV_8UC4 ? 4 : t == CV_8UC3 ? 3 : t == CV_16UC1 ? 2 : 1;
    }
    int type_ = -1;
    std::shared_ptr<unsigned char> buf_;
};
}  // namespace sgm_amd
#endif

namespace sgm_amd {

inline void fail(const char *what, const char *detail) {
#ifdef SGM_AMD_THROW
    throw std::runtime_error(std::string(what) + ": " + (detail ? detail : ""));
#else
    std::fprintf(stderr, "sgm_amd: %s: %s\n", what, detail ? detail : "");
    std::abort();
#endif
}

// Solver (inc/Solver.h:23-70): geometry, result maps and the device handle.
class Solver {
public:
    // m: the minimum disparity, sgm_set_min_disp (0: the reference's range [0, d))
    explicit Solver(int h, int w, int s, int d, int m = 0) {
        if (!(h > 0 && w > 0 && s > 0 && d > 0) || !(s == 1 || s == 2) ||
            !(d == 32 || d == 64 || d == 128 || d == 256))
            fail("Solver", "h,w,s,d > 0, s in {1,2}, d in {32,64,128,256} (Solver.cpp:6-10)");
        if (m < 0 || m % s != 0 || d + m + 1 > 65535)
            fail("Solver", "min_disp must be >= 0, a multiple of s and d + min_disp + 1 <= 65535");
        img_h = h / s;
        img_w = w / s;
        scale = s;
        max_disp = d;
        min_disp = m;
        invalid_disp = d + m + 1;
        in_h_ = h;
        in_w_ = w;
        filtered_disp.create(img_h, img_w, CV_32FC1);
        colored_disp.create(img_h, img_w, CV_8UC3);
    }
    virtual ~Solver() = default;

    Solver(const Solver &) = delete;
    Solver &operator=(Solver &) = delete;

    virtual void process(Mat &img_l, Mat &img_r) = 0;
    virtual void process(Mat &img_l, Mat &img_r, Mat &sky_mask, Mat &sky_mask_beta) = 0;

    // Solver.cpp:55-93: left image (BGR) above the colour-mapped disparity;
    // the lower tile starts at row img_h - 1 as in the reference.
    virtual void show_disp(Mat &debug_view) {
        colormap();
        debug_view.create(img_h * 2, img_w, CV_8UC3);
        std::memset(debug_view.data, 0, (size_t)debug_view.rows * debug_view.step);
        for (int i = 0; i < img_h && !img_l.empty(); ++i) {
            const unsigned char *src = img_l.template ptr<unsigned char>(i);
            Vec3b *dst = debug_view.template ptr<Vec3b>(i);
            for (int j = 0; j < img_w; ++j) dst[j][0] = dst[j][1] = dst[j][2] = src[j];
        }
        for (int i = 0; i < img_h; ++i)
            std::memcpy(debug_view.template ptr<Vec3b>(img_h - 1 + i),
                        colored_disp.template ptr<Vec3b>(i), (size_t)img_w * 3);
    }
    virtual const Mat &get_disp() const { return filtered_disp; }
    // the value of an invalid pixel of get_disp(): d + min_disp + 1 (Solver.cpp:21 with min_disp = 0)
    int get_invalid_disp() const { return invalid_disp; }
    int get_min_disp() const { return min_disp; }

protected:
    int img_h, img_w;
    int scale;
    int max_disp, invalid_disp;
    int min_disp;
    int in_h_, in_w_;

    Mat img_l, img_r;
    Mat filtered_disp;
    Mat colored_disp;
    Mat sky_mask, sky_mask_beta;

    // Solver.cpp:652-707 (on v - min_disp: the colours span the search range)
    void colormap() {
        for (int i = 0; i < img_h; ++i)
            for (int j = 0; j < img_w; ++j) {
                float v = filtered_disp.template at<float>(i, j) - (float)min_disp;
                Vec3b &c = colored_disp.template at<Vec3b>(i, j);
                if (v > max_disp - 1) {
                    c[0] = c[1] = c[2] = 0;
                    continue;
                }
                v *= (256 / (max_disp));
                if (v <= 51) {
                    c[0] = 255; c[1] = (unsigned char)(v * 5); c[2] = 0;
                } else if (v <= 102) {
                    v -= 51;
                    c[0] = (unsigned char)(255 - v * 5); c[1] = 255; c[2] = 0;
                } else if (v <= 153) {
                    v -= 102;
                    c[0] = 0; c[1] = 255; c[2] = (unsigned char)(v * 5);
                } else if (v <= 204) {
                    v -= 153;
                    c[0] = 0; c[1] = (unsigned char)(255 - (unsigned char)(128.0 * v / 51.0 + 0.5)); c[2] = 255;
                } else {
                    v -= 204;
                    c[0] = 0; c[1] = (unsigned char)(127 - (unsigned char)(127.0 * v / 51.0 + 0.5)); c[2] = 255;
                }
            }
    }
};

typedef std::shared_ptr<Solver> SolverPtr;

// Common body of the two solvers: one libsgm_hip.so handle per object, the
// whole frame (and post_filter) on the GPU.
class HipSolver : public Solver {
public:
    virtual ~HipSolver() {
        if (handle_) sgm_destroy(handle_);
    }
    HipSolver(const HipSolver &) = delete;
    HipSolver &operator=(const HipSolver &) = delete;

    // SGM.cpp:829-834 / BM.cpp:91-96
    virtual void process(Mat &img_l, Mat &img_r, Mat &sky_mask, Mat &sky_mask_beta) {
        this->sky_mask = sky_mask;
        this->sky_mask_beta = sky_mask_beta;
        process(img_l, img_r);
    }
    virtual void process(Mat &img_l, Mat &img_r) {
        if (img_l.rows != img_r.rows || img_l.cols != img_r.cols || img_l.type() != img_r.type() ||
            img_l.type() != pix_type(format_) || img_l.rows != in_h_ || img_l.cols != in_w_)
            fail("process", format_ == SGM_PIX_GRAY8
                                ? "inputs must be CV_8UC1 of the constructed size (SGM.cpp:34-38)"
                                : "inputs must be CV_8UC3 / CV_8UC4, as the input format says, of the "
                                  "constructed size");
        this->img_l = img_l;  // shallow, as SGM.cpp:59-60 (decimated on the device)
        this->img_r = img_r;
        if (staging()) {  // checked before any work: the grey images' host copies
            resized_[0] = Mat(full_h_, full_w_, CV_8UC1);
            resized_[1] = Mat(full_h_, full_w_, CV_8UC1);
        }
        // Each mask applies on its own, as in the reference: sky_mask to the
        // left DSI (Solver.cpp:146-178), sky_mask_beta to the right one
        // (Solver.cpp:200-232); BM reads sky_mask only (BM.cpp:33-34).
        const bool sky_l = !sky_mask.empty();
        const bool sky_r = !bm_ && !sky_mask_beta.empty();
        if (sky_l) check_mask(sky_mask, "sky_mask");
        if (sky_r) check_mask(sky_mask_beta, "sky_mask_beta");
        // The C-ABI takes one pitch for both masks: copy to a common (packed)
        // pitch when the two masks' steps differ.
        Mat ml = sky_mask, mr = sky_mask_beta;
        if (sky_l && sky_r && ml.step != mr.step) {
            ml = sky_mask.clone();
            mr = sky_mask_beta.clone();
        }
        const int sky_pitch = sky_l ? (int)ml.step : sky_r ? (int)mr.step : 0;
        const int rc = sgm_process(handle_, img_l.data, img_r.data, (int)img_l.step,
                                   sky_l ? ml.data : nullptr, sky_r ? mr.data : nullptr, sky_pitch,
                                   filtered_disp.template ptr<float>(0),
                                   (int)(filtered_disp.step / sizeof(float)), nullptr);
        if (rc != SGM_OK) fail("process", sgm_last_error(handle_));
        if (confidence_on_ &&
            sgm_stage_confidence(handle_, SGM_VIEW_LEFT, confidence_.template ptr<float>(0)) != SGM_OK)
            fail("process", sgm_last_error(handle_));
        if (!fill_mask_.empty() && sgm_stage_fill_mask(handle_, fill_mask_.data) != SGM_OK)
            fail("process", sgm_last_error(handle_));
        if (staging()) {
            // what the frame matched: the node's resized img_l / img_r (node.cpp:75-76), the
            // rectified or the converted pair, for show_disp and the point cloud (node.cpp:107,138)
            const auto stage = resizing_     ? sgm_stage_resized
                               : rectifying_ ? sgm_stage_rectified
                                             : sgm_stage_input_gray;
            for (int v = 0; v < 2; ++v)
                if (stage(handle_, v, resized_[v].data) != SGM_OK) fail("process", sgm_last_error(handle_));
            this->img_l = resized_[0];
            this->img_r = resized_[1];
        }
        if (scale > 1) decimate_left();
        // the products of this frame's map (sgm_set_reproject), as host copies
        if ((rp_outputs_ & SGM_REPROJECT_XYZ) && sgm_stage_reprojected(handle_, SGM_REPROJECT_XYZ, xyz_.data) != SGM_OK)
            fail("process", sgm_last_error(handle_));
        if ((rp_outputs_ & SGM_REPROJECT_DEPTH) &&
            sgm_stage_reprojected(handle_, SGM_REPROJECT_DEPTH, depth_.data) != SGM_OK)
            fail("process", sgm_last_error(handle_));
        if ((rp_outputs_ & SGM_REPROJECT_DEPTH16) &&
            sgm_stage_reprojected(handle_, SGM_REPROJECT_DEPTH16, depth16_.data) != SGM_OK)
            fail("process", sgm_last_error(handle_));
    }

    // Reprojection through stereoRectify's Q (sgm_set_reproject; 16 doubles,
    // row-major): every process() then also writes the products named in
    // `outputs` (SGM_REPROJECT_XYZ | SGM_REPROJECT_DEPTH | SGM_REPROJECT_DEPTH16)
    // from its final map, on the GPU, for xyz(), depth() and depth16().
    // max_range > 0: pixels with Z outside (0, max_range] are missing;
    // depth16 = rint(Z * depth_scale).  Missing pixels hold NaN (0 in depth16).
    void set_reproject(const double q[16], int outputs, float max_range = 0, float depth_scale = 1000) {
        sgm_reproject r;
        std::memcpy(r.q, q, sizeof(r.q));
        r.outputs = outputs;
        r.max_range = max_range;
        r.depth_scale = depth_scale;
        if (sgm_set_reproject(handle_, &r) != SGM_OK) fail("set_reproject", sgm_last_error(handle_));
        rp_outputs_ = outputs;
        xyz_ = (outputs & SGM_REPROJECT_XYZ) ? Mat(img_h, img_w, CV_32FC3) : Mat();
        depth_ = (outputs & SGM_REPROJECT_DEPTH) ? Mat(img_h, img_w, CV_32FC1) : Mat();
        depth16_ = (outputs & SGM_REPROJECT_DEPTH16) ? Mat(img_h, img_w, CV_16UC1) : Mat();
    }
    void clear_reproject() {
        if (sgm_set_reproject(handle_, nullptr) != SGM_OK) fail("clear_reproject", sgm_last_error(handle_));
        rp_outputs_ = 0;
        xyz_ = depth_ = depth16_ = Mat();
    }
    // A working-grid CV_32FC1 map reprojected on the GPU through the Q set
    // (sgm_stage_reproject): each product whose pointer is not null is created
    // and filled (CV_32FC3, CV_32FC1, CV_16UC1).
    void reproject(const Mat &disp, Mat *xyz, Mat *depth, Mat *depth16) {
        if (disp.type() != CV_32FC1 || disp.rows != img_h || disp.cols != img_w)
            fail("reproject", "disp must be CV_32FC1 on the working grid");
        const Mat d = disp.step == (size_t)img_w * sizeof(float) ? disp : disp.clone();
        Mat x, z, u;
        if (xyz) x = Mat(img_h, img_w, CV_32FC3);
        if (depth) z = Mat(img_h, img_w, CV_32FC1);
        if (depth16) u = Mat(img_h, img_w, CV_16UC1);
        if (sgm_stage_reproject(handle_, d.template ptr<float>(0), xyz ? x.template ptr<float>(0) : nullptr,
                                depth ? z.template ptr<float>(0) : nullptr,
                                depth16 ? u.template ptr<unsigned short>(0) : nullptr) != SGM_OK)
            fail("reproject", sgm_last_error(handle_));
        if (xyz) *xyz = x;
        if (depth) *depth = z;
        if (depth16) *depth16 = u;
    }
    // The last process()'s products on the working grid; a product that
    // set_reproject was not asked for fails
    const Mat &xyz() const { return product(SGM_REPROJECT_XYZ, xyz_, "xyz"); }
    const Mat &depth() const { return product(SGM_REPROJECT_DEPTH, depth_, "depth"); }
    const Mat &depth16() const { return product(SGM_REPROJECT_DEPTH16, depth16_, "depth16"); }

    // A caller's DEVICE cost volume (sgm_volume: learned costs, AD/SAD/MI, ...)
    // through the frame from the cost volume on (sgm_aggregate_device): the
    // path aggregation, the LR check, post_filter and the reprojection as the
    // handle is set up; d_out a DEVICE rows x cols f32 map (out_pitch floats),
    // d_raw the left raw map or null.  Enqueue only: the caller synchronises.
    void aggregate_device(const sgm_volume &vol, float *d_out, int out_pitch, uint16_t *d_raw = nullptr,
                          void *stream = nullptr) {
        if (sgm_aggregate_device(handle_, &vol, d_out, out_pitch, d_raw, stream) != SGM_OK)
            fail("aggregate_device", sgm_last_error(handle_));
    }
    // Its first launch alone (sgm_volume_import_device): the dense fp32 rows x
    // cols x D volume of `view` (the right view's derived from the left one)
    void import_volume_device(const sgm_volume &vol, int view, float *d_dst, void *stream = nullptr) {
        if (sgm_volume_import_device(handle_, &vol, view, d_dst, stream) != SGM_OK)
            fail("import_volume_device", sgm_last_error(handle_));
    }

    // The reference's two cost filters (Solver.cpp:296-368) on a finished volume.
    // set_volume_filter(bits): SGM_FILTER_H | SGM_FILTER_V on each view's volume in every later
    // volume frame (aggregate_device, frames after set_cost(SAD | SSD)); 0, the default: none.
    void set_volume_filter(int filters) {
        if (sgm_set_volume_filter(handle_, filters) != SGM_OK) fail("set_volume_filter", sgm_last_error(handle_));
    }
    int volume_filter() const {
        int filters = 0;
        if (sgm_get_volume_filter(handle_, &filters) != SGM_OK) fail("volume_filter", sgm_last_error(handle_));
        return filters;
    }
    // The filters `filters` names, in place on a dense fp32 rows x cols x D DEVICE volume
    // (sgm_filter_volume_device).  Enqueue only.
    void filter_volume_device(float *d_cost, int filters = SGM_FILTER_H | SGM_FILTER_V, void *stream = nullptr) {
        if (sgm_filter_volume_device(handle_, d_cost, filters, stream) != SGM_OK)
            fail("filter_volume_device", sgm_last_error(handle_));
    }

    // The matching cost of every later frame (sgm_set_cost): SGM_COST_CENSUS
    // (the default), or the reference's SAD / SSD window cost or its CT, SGM_COST_CT
    // (Solver::build_dsi over cost.cpp:4-96: no blur, no cost filters; sky masks are
    // then refused).
    void set_cost(int kind) {
        if (sgm_set_cost(handle_, kind) != SGM_OK) fail("set_cost", sgm_last_error(handle_));
    }
    int cost() const {
        int kind = SGM_COST_CENSUS;
        if (sgm_get_cost(handle_, &kind) != SGM_OK) fail("cost", sgm_last_error(handle_));
        return kind;
    }
    // The matching window of the census and of the SAD / SSD costs (sgm_set_window): the
    // reference's WIN_H, WIN_W (inc/Solver.h:10-11: 7, 9) before the division by s.  Every later
    // frame of an SGM or a BM, and window_cost_device, use it.  Accepted: 1 <= win_h / s,
    // win_w / s <= 9, not 1 x 1 taps, not 9 x 9 (80 census bits); anything else fails and
    // changes nothing.
    void set_window(int win_h, int win_w) {
        if (sgm_set_window(handle_, win_h, win_w) != SGM_OK) fail("set_window", sgm_last_error(handle_));
    }
    void get_window(int *win_h, int *win_w) const {
        if (sgm_get_window(handle_, win_h, win_w) != SGM_OK) fail("get_window", sgm_last_error(handle_));
    }
    // The reference's WEIGHTED_COST (inc/Solver.h:15) as a setting (sgm_set_weighted): Gaussian
    // taps in SAD and SSD, and the census's window masked to the disc of weights >= 0.5.  Every
    // consumer of the window follows it.  Only with win_h / s and win_w / s odd: enabling it on
    // another window, or setting such a window on a weighted solver, fails and changes nothing.
    void set_weighted(bool enable) {
        if (sgm_set_weighted(handle_, enable ? 1 : 0) != SGM_OK) fail("set_weighted", sgm_last_error(handle_));
    }
    bool weighted() const {
        int on = 0;
        if (sgm_get_weighted(handle_, &on) != SGM_OK) fail("weighted", sgm_last_error(handle_));
        return on != 0;
    }
    // The (win_h / s) x (win_w / s) weight table in use, row-major (sgm_get_window_weights).
    std::vector<float> window_weights() const {
        int n = 0;
        if (sgm_get_window_weights(handle_, nullptr, 0, &n) != SGM_OK) fail("window_weights", sgm_last_error(handle_));
        std::vector<float> w((size_t)n);
        if (sgm_get_window_weights(handle_, w.data(), n, &n) != SGM_OK) fail("window_weights", sgm_last_error(handle_));
        return w;
    }
    // The SAD / SSD / CT volume alone (sgm_window_cost_device): DEVICE grey images of
    // the constructed size, `pitch` bytes per row, into the dense fp32 rows x
    // cols x D volume d_dst, which aggregate_device takes.  Enqueue only.
    void window_cost_device(int kind, const uint8_t *d_left, const uint8_t *d_right, int pitch, float *d_dst,
                            void *stream = nullptr) {
        if (sgm_window_cost_device(handle_, kind, d_left, d_right, pitch, d_dst, stream) != SGM_OK)
            fail("window_cost_device", sgm_last_error(handle_));
    }

    // The pixel format of the images process() takes (sgm_set_input_format):
    // SGM_PIX_BGR8 / SGM_PIX_RGB8 take CV_8UC3 Mats, SGM_PIX_BGRA8 /
    // SGM_PIX_RGBA8 CV_8UC4 ones, and every frame converts them to grey on the
    // GPU first -- inside the resize or the remap when one is set.
    // SGM_PIX_GRAY8: off, CV_8UC1 again.
    void set_input_format(int fmt) {
        const int rc = sgm_set_input_format(handle_, fmt);
        sync_input_stage();  // (before failing: a failed allocation leaves the handle's stages off)
        if (rc != SGM_OK) fail("set_input_format", sgm_last_error(handle_));
    }
    // The decoder's grey conversion (node.cpp:69-70 IMREAD_GRAYSCALE; cvtColor)
    // of a colour image of any size on the GPU (sgm_stage_gray); dst may be src.
    void gray(const Mat &src, Mat &dst, int fmt) {
        if (src.empty() || fmt == SGM_PIX_GRAY8 || src.type() != pix_type(fmt))
            fail("gray", "src must be a CV_8UC3 / CV_8UC4 image, as the colour format says");
        Mat out(src.rows, src.cols, CV_8UC1);
        if (sgm_stage_gray(handle_, fmt, src.data, src.rows, src.cols, (int)src.step, out.data) != SGM_OK)
            fail("gray", sgm_last_error(handle_));
        dst = out;
    }
    // CV_8UC1 at the constructed size: the grey image of `view` (0 left, 1
    // right) the last process() matched -- converted, and resized or rectified
    // when those stages are set; empty while the input format is grey
    const Mat &input_gray(int view) const {
        return format_ != SGM_PIX_GRAY8 ? resized_[view == 1 ? 1 : 0] : none_;
    }

    // cv::resize(src, dst, Size(w, h)) (node.cpp:75-76: 8-bit, one channel,
    // INTER_LINEAR in its pinned fixed-point form, sgm_stage_resize) on the
    // GPU, to the constructed size; dst may be src, as in the node.
    void resize(const Mat &src, Mat &dst) {
        if (src.empty() || src.type() != CV_8UC1) fail("resize", "src must be a CV_8UC1 image");
        Mat out(full_h_, full_w_, CV_8UC1);
        if (sgm_stage_resize(handle_, src.data, src.rows, src.cols, (int)src.step, out.data) != SGM_OK)
            fail("resize", sgm_last_error(handle_));
        dst = out;
    }

    // The size of the images process() takes (sgm_set_input_size): every
    // frame then starts by resizing both to the constructed size on the GPU,
    // and images of any other size fail as a wrong-size image does.  (0, 0):
    // off, the constructed size again.
    void set_input_size(int rows, int cols) {
        const int rc = sgm_set_input_size(handle_, rows, cols);
        sync_input_stage();  // (before failing: a failed allocation leaves the handle's stage off)
        if (rc != SGM_OK) fail("set_input_size", sgm_last_error(handle_));
    }
    // CV_8UC1 at the constructed size: the last process()'s resized image of
    // `view` (0 left, 1 right); empty while no input size is set
    const Mat &get_resized(int view) const { return resizing_ ? resized_[view == 1 ? 1 : 0] : none_; }

    // Rectification (sgm_set_rectify): process() then takes raw rows x cols
    // camera images, and every frame starts by remapping both through these
    // maps on the GPU -- cv::initUndistortRectifyMap(..., CV_32FC1, ...)'s
    // outputs at the constructed size, one pair per view; cv::convertMaps +
    // cv::remap INTER_LINEAR, BORDER_CONSTANT 0 in their pinned fixed-point
    // form.  The maps may read a source of any size, so this also resizes: not
    // together with set_input_size.  (0, 0) with four empty Mats: off.
    void set_rectify(int rows, int cols, const Mat &map_x_l, const Mat &map_y_l, const Mat &map_x_r,
                     const Mat &map_y_r) {
        const Mat *in[4] = {&map_x_l, &map_y_l, &map_x_r, &map_y_r};
        Mat m[4];
        bool same_step = true;
        for (int k = 0; k < 4; ++k) {
            if (!in[k]->empty() &&
                (in[k]->type() != CV_32FC1 || in[k]->rows != full_h_ || in[k]->cols != full_w_))
                fail("set_rectify", "maps must be CV_32FC1 of the constructed size");
            m[k] = *in[k];
            same_step = same_step && (m[k].empty() || m[0].empty() || m[k].step == m[0].step);
        }
        // the C-ABI takes one pitch for the four maps: dense copies when their steps differ
        for (int k = 0; k < 4 && !same_step; ++k)
            if (!m[k].empty()) m[k] = m[k].clone();
        int pitch = full_w_;
        for (int k = 0; k < 4; ++k)
            if (!m[k].empty()) pitch = (int)(m[k].step / sizeof(float));
        const float *p[4];
        for (int k = 0; k < 4; ++k) p[k] = m[k].empty() ? nullptr : m[k].template ptr<float>(0);
        const int rc = sgm_set_rectify(handle_, rows, cols, p[0], p[1], p[2], p[3], pitch);
        sync_input_stage();  // (before failing: a failed replacement of maps leaves them off)
        if (rc != SGM_OK) fail("set_rectify", sgm_last_error(handle_));
    }
    // cv::remap(src, dst, map_x, map_y, INTER_LINEAR) of `view`'s (0 left, 1
    // right) raw image through the maps set, on the GPU (sgm_stage_remap);
    // dst may be src.
    void remap(const Mat &src, Mat &dst, int view) {
        int rows = 0, cols = 0;
        sgm_get_rectify(handle_, &rows, &cols);
        if (rows && (src.type() != CV_8UC1 || src.rows != rows || src.cols != cols))
            fail("remap", "src must be a CV_8UC1 image of the size the maps were set for");
        Mat out(full_h_, full_w_, CV_8UC1);
        if (sgm_stage_remap(handle_, view, src.data, (int)src.step, out.data) != SGM_OK)
            fail("remap", sgm_last_error(handle_));
        dst = out;
    }
    // CV_8UC1 at the constructed size: the last process()'s rectified image of
    // `view` (0 left, 1 right); empty while no maps are set
    const Mat &rectified(int view) const { return rectifying_ ? resized_[view == 1 ? 1 : 0] : none_; }
    // CV_8UC1 at the constructed size: 255 where all four taps of the pixel
    // lie inside the raw image, else 0 (stereoRectify's validPixROI per pixel)
    Mat rectify_valid(int view) {
        Mat out(full_h_, full_w_, CV_8UC1);
        if (sgm_stage_rectify_valid(handle_, view, out.data) != SGM_OK)
            fail("rectify_valid", sgm_last_error(handle_));
        return out;
    }

    sgm_handle *handle() const { return handle_; }

    // The median fill's launch budget (sgm_set_post_filter_launches): n = 0,
    // the adaptive fill, whose convergence test blocks the host inside
    // process(); 1..4096, exactly n fill launches and no host wait before the
    // frame's end, where process() reports a fill that launch n did not prove.
    void set_post_filter_launches(int n) {
        if (sgm_set_post_filter_launches(handle_, n) != SGM_OK)
            fail("set_post_filter_launches", sgm_last_error(handle_));
    }

    // The per-pixel match confidence (sgm_set_confidence): with it on, every
    // process() also keeps the left view's uniqueness ratio, min_cost /
    // sec_min_cost of the aggregated WTA (SGM.cpp:392-409; lower = more
    // distinctive), for get_confidence().  BM has none: it fails.
    void set_confidence(bool enable) {
        if (sgm_set_confidence(handle_, enable ? 1 : 0) != SGM_OK)
            fail("set_confidence", sgm_last_error(handle_));
        confidence_on_ = enable;
        if (enable) {
            confidence_.create(img_h, img_w, CV_32FC1);
            std::memset(confidence_.data, 0, (size_t)confidence_.rows * confidence_.step);
        } else {
            confidence_ = Mat();
        }
    }
    // CV_32FC1 on the working grid, the left view of the last process();
    // empty while confidence is off
    const Mat &get_confidence() const { return confidence_; }

    // The occlusion-aware hole filling (sgm_set_fill; SGM_FILL_OFF,
    // SGM_FILL_BACKGROUND, SGM_FILL_INTERPOLATE): with a mode set, every
    // process() fills the invalid pixels of its post-filtered map on the GPU
    // (Hirschmueller 2008, 2.6) before the reprojection, and get_disp() is the
    // dense map.  SGM serves both modes, BM and GPU_SGM (one view) the
    // background mode; anything else fails.
    void set_fill(int mode) {
        if (sgm_set_fill(handle_, mode) != SGM_OK) fail("set_fill", sgm_last_error(handle_));
        fill_mask_ = mode != SGM_FILL_OFF ? Mat(img_h, img_w, CV_8UC1) : Mat();
        if (!fill_mask_.empty()) std::memset(fill_mask_.data, 0, (size_t)fill_mask_.rows * fill_mask_.step);
    }
    // CV_8UC1 on the working grid, of the last process(): 0 measured, 1 filled
    // as occlusion, 2 filled as mismatch, 3 still invalid; empty while fill is off
    const Mat &get_fill_mask() const { return fill_mask_; }

protected:
    // views = 1: the left view alone (BM; GPU_SGM, gpu_sgm/src/SGM.cu:105-232)
    // paths = 4: the reference built with USE_8_PATH = false (inc/SGM.h:7)
    // min_disp: the search range starts there (sgm_set_min_disp; BM: 0 only)
    HipSolver(int h, int w, int s, int d, int solver, int views = 2, int paths = 8, int min_disp = 0)
        : Solver(h, w, s, d, min_disp), bm_(solver == SGM_SOLVER_BM), full_h_(h), full_w_(w) {
        if (paths != 4 && paths != 8) fail("Solver", "paths must be 4 or 8 (USE_8_PATH, inc/SGM.h:7)");
        if (bm_ && min_disp != 0) fail("Solver", "BM takes no min_disp");
        sgm_params p;
        if (sgm_default_params(&p, h, w, s, d) != SGM_OK) fail("Solver", "sgm_default_params");
        p.solver = solver;
        p.paths = paths;
        p.post_filter = 1;  // process() ends with post_filter(): SGM.cpp:821, BM.cpp:88 (on the GPU)
        p.views = bm_ ? 1 : views;
        const int rc = sgm_create(&p, device(), &handle_);
        if (rc != SGM_OK) fail("sgm_create", handle_ ? sgm_last_error(handle_) : "no device");
        if (min_disp != 0 && sgm_set_min_disp(handle_, min_disp) != SGM_OK)
            fail("sgm_set_min_disp", sgm_last_error(handle_));
        if (sgm_get_invalid_disp(handle_, &invalid_disp) != SGM_OK) fail("Solver", "sgm_get_invalid_disp");
    }

private:
    sgm_handle *handle_ = nullptr;
    bool bm_;
    bool confidence_on_ = false;
    Mat confidence_;
    Mat fill_mask_;          // set_fill: the last process()'s fill mask
    int full_h_, full_w_;    // the constructed size (in_h_, in_w_: what process() takes)
    bool resizing_ = false;  // set_input_size
    bool rectifying_ = false;  // set_rectify
    int format_ = SGM_PIX_GRAY8;  // set_input_format
    Mat resized_[2];         // the resized, rectified or converted pair of the last process()
    Mat none_;
    int rp_outputs_ = 0;     // set_reproject: the products process() downloads
    Mat xyz_, depth_, depth16_;

    const Mat &product(int which, const Mat &m, const char *what) const {
        if (!(rp_outputs_ & which)) fail(what, "set_reproject was not asked for this product");
        return m;
    }

    // resizing_, rectifying_ and the size process() takes, read back from the
    // handle (sgm_last_error is untouched): at most one of the two stages is
    // set, and switching the other off changes nothing
    void sync_input_stage() {
        int rs_rows = 0, rs_cols = 0, rc_rows = 0, rc_cols = 0;
        sgm_get_input_size(handle_, &rs_rows, &rs_cols);
        sgm_get_rectify(handle_, &rc_rows, &rc_cols);
        resizing_ = rs_rows != 0;
        rectifying_ = rc_rows != 0;
        in_h_ = resizing_ ? rs_rows : rectifying_ ? rc_rows : full_h_;
        in_w_ = resizing_ ? rs_cols : rectifying_ ? rc_cols : full_w_;
        sgm_get_input_format(handle_, &format_);
        if (!staging()) resized_[0] = resized_[1] = Mat();
    }

    // an input stage is set: process() keeps host copies of the grey pair the frame matched
    bool staging() const { return resizing_ || rectifying_ || format_ != SGM_PIX_GRAY8; }

    // the Mat type of a pixel format's images
    static int pix_type(int fmt) {
        return fmt == SGM_PIX_GRAY8 ? CV_8UC1 : (fmt == SGM_PIX_BGR8 || fmt == SGM_PIX_RGB8 ? CV_8UC3 : CV_8UC4);
    }

    void check_mask(const Mat &m, const char *what) const {
        if (m.type() != CV_8UC1 || m.rows != img_h || m.cols != img_w)
            fail(what, "sky masks must be CV_8UC1 on the working grid (Solver.cpp:146,200)");
    }

    static int device() {
        const char *e = std::getenv("SGM_AMD_DEVICE");
        return e ? std::atoi(e) : 0;
    }
    // keep img_l on the working grid for show_disp: SGM.cpp:40-56 takes rows
    // i*scale, BM.cpp:20-31 rows i (both every scale-th column)
    void decimate_left() {
        Mat small(img_h, img_w, CV_8UC1);
        for (int i = 0; i < img_h; ++i) {
            const unsigned char *src = img_l.template ptr<unsigned char>(bm_ ? i : i * scale);
            unsigned char *dst = small.template ptr<unsigned char>(i);
            for (int j = 0; j < img_w; ++j) dst[j] = src[j * scale];
        }
        img_l = small;
    }
};

// SGM (inc/SGM.h:10-26): 8-path semi-global matching, both views, LR check,
// post_filter (SGM.cpp:32-826).
class SGM : public HipSolver {
public:
    explicit SGM(int h, int w, int s, int d) : HipSolver(h, w, s, d, SGM_SOLVER_SGM) {}
    // paths = 4: the reference's USE_8_PATH = false (inc/SGM.h:7), S = ((L1+L2)+L3)+L4
    SGM(int h, int w, int s, int d, int paths) : HipSolver(h, w, s, d, SGM_SOLVER_SGM, 2, paths) {}
    // min_disp = m: disparities [m, m + d), true-disparity maps, invalid = d + m + 1
    SGM(int h, int w, int s, int d, int paths, int min_disp)
        : HipSolver(h, w, s, d, SGM_SOLVER_SGM, 2, paths, min_disp) {}
    SGM(const SGM &) = delete;
    SGM &operator=(const SGM &) = delete;
};

// BM (inc/BM.h:6-19): census cost, the two cost filters and a WTA on the
// filtered cost (BM.cpp:9-97).  get_disp() is the post-filtered integer
// disparity (the reference's BM::process never writes filtered_disp).
class BM : public HipSolver {
public:
    explicit BM(int h, int w, int s, int d) : HipSolver(h, w, s, d, SGM_SOLVER_BM) {}
    BM(const BM &) = delete;
    BM &operator=(const BM &) = delete;
};

typedef std::shared_ptr<BM> BMSolverPtr;
typedef std::shared_ptr<SGM> SGMSolverPtr;

}  // namespace sgm_amd

#endif
