// sgm_resize_args.h -- the host side of the input resize (sgm_resize.hip): the
// checks of its sizes and the scale factors the kernel takes.  Plain C++ with
// no HIP in it, so that tests/cpp/resize_args_main.cpp can run it on the CPU
// under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdio.h>

namespace sgm {

// What resize_kernel takes beside the sizes.
struct ResizeScale {
    double x, y;  // 1.0 / ((double)dst / (double)src), in that order (cv::resize's inv_scale)
    int half;     // exactly half size in both axes: the 2x2 mean
};

inline ResizeScale resize_scale(int src_rows, int src_cols, int dst_rows, int dst_cols) {
    ResizeScale s;
    s.x = 1.0 / ((double)dst_cols / (double)src_cols);
    s.y = 1.0 / ((double)dst_rows / (double)src_rows);
    s.half = src_cols == 2 * (long long)dst_cols && src_rows == 2 * (long long)dst_rows;
    return s;
}

// sgm_set_input_size's sizes: (0, 0) switches the resize off, otherwise both
// positive and the image addressable.  Returns false with the reason in why.
inline bool input_size_ok(int src_rows, int src_cols, char *why, size_t n) {
    if (src_rows < 0 || src_cols < 0) {
        snprintf(why, n, "sizes must be >= 0, got %d x %d", src_rows, src_cols);
        return false;
    }
    if ((src_rows == 0) != (src_cols == 0)) {
        snprintf(why, n, "both sizes are zero (off) or neither, got %d x %d", src_rows, src_cols);
        return false;
    }
    if ((unsigned long long)src_rows * (unsigned long long)src_cols > 0x7fffffffULL) {
        snprintf(why, n, "image too large: %d x %d", src_rows, src_cols);
        return false;
    }
    return true;
}

// One resize call's source: at least 1 x 1, rows no narrower than the image.
inline bool resize_src_ok(int src_rows, int src_cols, int src_pitch, char *why, size_t n) {
    if (src_rows <= 0 || src_cols <= 0) {
        snprintf(why, n, "source size must be >= 1 x 1, got %d x %d", src_rows, src_cols);
        return false;
    }
    if (src_pitch < src_cols) {
        snprintf(why, n, "src_pitch %d below src_cols %d", src_pitch, src_cols);
        return false;
    }
    return true;
}

}  // namespace sgm
