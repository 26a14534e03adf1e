/*
 * Stand-in for <opencv2/core/core.hpp>, written from OpenCV's public API.
 *
 * TEST INFRASTRUCTURE ONLY.  It exists so that the reference's
 * src/{Solver,SGM,cost,BM}.cpp compile unmodified where OpenCV is absent
 * (oracle/Makefile, target ref).  It holds exactly what those four files use:
 * a reference-counted cv::Mat over one contiguous buffer, Point/Size/Rect,
 * Vec3b, the CV_* constants and the MIN/MAX macros, plus declarations of
 * cv::GaussianBlur and cv::cvtColor (defined by oracle/ref/ref_driver.cpp).
 * Unlike cv::Mat::create, create() here zero-fills, so that a map the
 * reference never writes (BM's filtered_disp) reads the same on every run.
 */
#ifndef SGM_REF_STANDIN_CORE_HPP
#define SGM_REF_STANDIN_CORE_HPP

#include <algorithm>
#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

typedef unsigned char uchar;

#ifndef MIN
#define MIN(a, b) ((a) > (b) ? (b) : (a))
#endif
#ifndef MAX
#define MAX(a, b) ((a) < (b) ? (b) : (a))
#endif

/* type = depth + ((channels - 1) << 3), as in OpenCV's CV_MAKETYPE */
#define CV_8U 0
#define CV_32F 5
#define CV_8UC1 (CV_8U + (0 << 3))
#define CV_8UC3 (CV_8U + (2 << 3))
#define CV_32FC1 (CV_32F + (0 << 3))
#define CV_GRAY2BGR 8

namespace cv {

struct Point {
    int x, y;
    Point() : x(0), y(0) {}
    Point(int x_, int y_) : x(x_), y(y_) {}
};

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

struct Vec3b {
    uchar val[3];
    uchar &operator[](int i) { return val[i]; }
    const uchar &operator[](int i) const { return val[i]; }
};

class Mat {
public:
    int rows, cols;
    uchar *data;
    size_t step;   /* bytes per row */

    Mat() : rows(0), cols(0), data(NULL), step(0), type_(0) {}
    Mat(int r, int c, int type) : rows(0), cols(0), data(NULL), step(0), type_(0) { create(r, c, type); }
    /* header over caller-owned memory */
    Mat(int r, int c, int type, void *p) : rows(r), cols(c), data((uchar *)p), type_(type)
    {
        step = (size_t)c * elemSize();
    }

    void create(int r, int c, int type)
    {
        if (data && r == rows && c == cols && type == type_)
            return;
        rows = r;
        cols = c;
        type_ = type;
        step = (size_t)c * elemSize();
        const size_t n = step * (size_t)r;
        buf_.reset(new uchar[n ? n : 1], std::default_delete<uchar[]>());
        std::memset(buf_.get(), 0, n);
        data = buf_.get();
    }

    void release()
    {
        buf_.reset();
        data = NULL;
        rows = cols = 0;
        step = 0;
    }

    bool empty() const { return data == NULL || rows == 0 || cols == 0; }
    int type() const { return type_; }
    int depth() const { return type_ & 7; }
    int channels() const { return (type_ >> 3) + 1; }
    size_t elemSize() const { return (size_t)channels() * (depth() == CV_32F ? 4 : 1); }

    template <typename T> T *ptr(int i = 0) { return (T *)(data + (size_t)i * step); }
    template <typename T> const T *ptr(int i = 0) const { return (const T *)(data + (size_t)i * step); }
    template <typename T> T &at(int i, int j) { return ptr<T>(i)[j]; }
    template <typename T> const T &at(int i, int j) const { return ptr<T>(i)[j]; }

    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }

    /* a view that shares the parent's buffer */
    Mat operator()(const Rect &r) const
    {
        Mat m;
        m.rows = r.height;
        m.cols = r.width;
        m.type_ = type_;
        m.step = step;
        m.buf_ = buf_;
        m.data = data + (size_t)r.y * step + (size_t)r.x * elemSize();
        return m;
    }

    void copyTo(Mat &dst) const
    {
        dst.create(rows, cols, type_);
        for (int i = 0; i < rows; ++i)
            std::memcpy(dst.data + (size_t)i * dst.step, data + (size_t)i * step, (size_t)cols * elemSize());
    }

private:
    int type_;
    std::shared_ptr<uchar> buf_;
};

void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sigmaX, double sigmaY = 0);
void cvtColor(const Mat &src, Mat &dst, int code);

} /* namespace cv */

#endif
