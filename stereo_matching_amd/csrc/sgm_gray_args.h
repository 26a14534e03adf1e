// sgm_gray_args.h -- the host side of the colour input (sgm_gray.hip, DESIGN.md
// 5l): the table from pixel format to bytes per pixel and the checks of a
// conversion call's sizes and pitches.  Plain C++ with no HIP in it, so that
// tests/cpp/gray_args_main.cpp can run it on the CPU under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdio.h>

namespace sgm {

// The formats of include/sgm_hip.h (SGM_PIX_*), by value: 0 grey, 1 BGR8,
// 2 RGB8, 3 BGRA8, 4 RGBA8.
constexpr int kPixFormats = 5;

// Bytes per pixel of a format; 0 for a value that is no format.
inline int pix_bpp(int fmt) {
    static const int bpp[kPixFormats] = {1, 3, 3, 4, 4};
    return fmt >= 0 && fmt < kPixFormats ? bpp[fmt] : 0;
}

// The byte of a pixel that holds red (blue is at 2 minus that, green at 1, a
// fourth byte is alpha and ignored); grey has none.
inline int pix_red_at(int fmt) { return fmt == 1 || fmt == 3 ? 2 : 0; }

// sgm_set_input_format's format: any of the five.
inline bool input_format_ok(int fmt, char *why, size_t n) {
    if (!pix_bpp(fmt)) {
        snprintf(why, n, "unknown pixel format %d", fmt);
        return false;
    }
    return true;
}

// Bytes of one staged image of rows x cols pixels; false when a row or the
// image is not addressable with an int.
inline bool pix_image_bytes(int fmt, int rows, int cols, size_t *bytes) {
    const unsigned long long row = (unsigned long long)cols * (unsigned)pix_bpp(fmt);
    const unsigned long long all = row * (unsigned long long)rows;
    if (rows < 0 || cols < 0 || row > 0x7fffffffULL || all > 0x7fffffffULL) return false;
    *bytes = (size_t)all;
    return true;
}

// One conversion call: a colour format, at least 1 x 1, rows no narrower than
// the image on either side.  Returns false with the reason in why.
inline bool gray_call_ok(int fmt, int rows, int cols, int src_pitch, int dst_pitch, char *why, size_t n) {
    const int bpp = pix_bpp(fmt);
    if (!bpp) {
        snprintf(why, n, "unknown pixel format %d", fmt);
        return false;
    }
    if (bpp == 1) {
        snprintf(why, n, "format %d is grey already: nothing to convert", fmt);
        return false;
    }
    if (rows <= 0 || cols <= 0) {
        snprintf(why, n, "size must be >= 1 x 1, got %d x %d", rows, cols);
        return false;
    }
    size_t bytes;
    if (!pix_image_bytes(fmt, rows, cols, &bytes)) {
        snprintf(why, n, "image too large: %d x %d at %d bytes per pixel", rows, cols, bpp);
        return false;
    }
    if ((long long)src_pitch < (long long)cols * bpp) {
        snprintf(why, n, "src_pitch %d below cols x bytes per pixel %lld", src_pitch, (long long)cols * bpp);
        return false;
    }
    if (dst_pitch < cols) {
        snprintf(why, n, "dst_pitch %d below cols %d", dst_pitch, cols);
        return false;
    }
    return true;
}

}  // namespace sgm
