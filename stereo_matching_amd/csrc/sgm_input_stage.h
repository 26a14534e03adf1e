// sgm_input_stage.h -- what stands in front of a frame (DESIGN.md "The input
// slot"): the input size, the rectification maps' source size and the pixel
// format a handle was given, and every question the host side asks of them.
// Plain C++ with no HIP in it, so that tests/cpp/input_stage_main.cpp can run it
// on the CPU under a sanitizer.
#pragma once

#include "sgm_gray_args.h"

namespace sgm {

// The launch a frame begins with.  The resize and the remap exclude each other
// (the setters see to it); a colour format rides inside either and is a launch
// of its own only when neither is set.
enum InputKind { INPUT_NONE, INPUT_RESIZE, INPUT_RECTIFY, INPUT_GRAY };

struct InputStage {
    int in_rows = 0, in_cols = 0;  // sgm_set_input_size: frames take in_rows x in_cols images (0, 0: off)
    int rc_rows = 0, rc_cols = 0;  // sgm_set_rectify: the maps read rc_rows x rc_cols images (0, 0: off)
    int fmt = 0;                   // sgm_set_input_format: the images' pixel format (SGM_PIX_GRAY8 = 0: off)

    InputKind kind() const { return in_rows ? INPUT_RESIZE : rc_rows ? INPUT_RECTIFY : fmt ? INPUT_GRAY : INPUT_NONE; }
    // rows x cols of the images a frame of a height x width handle takes, their bytes per pixel and per row
    int rows(int height) const { return in_rows ? in_rows : rc_rows ? rc_rows : height; }
    int cols(int width) const { return in_rows ? in_cols : rc_rows ? rc_cols : width; }
    int bpp() const { return pix_bpp(fmt); }
    int row_bytes(int width) const { return cols(width) * bpp(); }
    // Whether the handle owns the two full-size grey images the first launch writes and the host
    // API's staging of the two raw images (an aux_only handle runs no frames: it keeps maps for
    // sgm_remap_device alone), and the bytes of each staging image (0: none).
    bool stages(bool aux_only) const { return in_rows || (rc_rows && !aux_only) || fmt; }
    size_t raw_bytes(int height, int width, bool aux_only) const {
        return stages(aux_only) ? (size_t)rows(height) * row_bytes(width) : 0;
    }
};

// The frames' images at format fmt must stay addressable with an int: rows x
// cols of them, or height x width with no size given (rows == 0).
inline bool input_bytes_ok(int fmt, int rows, int cols, int height, int width) {
    size_t bytes;
    return pix_image_bytes(fmt, rows ? rows : height, rows ? cols : width, &bytes);
}

}  // namespace sgm
