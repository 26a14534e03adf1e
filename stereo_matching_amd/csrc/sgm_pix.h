// sgm_pix.h -- one input pixel as the grey value the frame works on (DESIGN.md
// 5l), shared by the stand-alone conversion (sgm_gray.hip) and the fused input
// stages (sgm_resize.hip, sgm_rectify.hip).  Device code.
//
//   Y = (4899 R + 9617 G + 1868 B + 8192) >> 14
//
// (0.299, 0.587, 0.114 at 14 bits, summing to 16384: R = G = B = v gives v, the
// result is in [0, 255]; OpenCV 2.4.13's cvtColor(BGR2GRAY).)  F is a
// SGM_PIX_* value: 0 grey, 1 BGR8, 2 RGB8, 3 BGRA8, 4 RGBA8; the alpha byte is
// never used.
#pragma once

#include <stdint.h>

namespace sgm {

template <int F>
struct Pix {
    static constexpr int bpp = F == 0 ? 1 : (F <= 2 ? 3 : 4);
    static constexpr int red = (F == 1 || F == 3) ? 2 : 0;  // byte of R; B at 2 - red
};

__device__ __forceinline__ int gray_y(int r, int g, int b) {
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14;
}

// The grey value of the pixel whose first byte is p[0].  F = 0 is the plain
// byte load the one-channel kernels always did.
template <int F>
__device__ __forceinline__ int gray_px(const uint8_t *p) {
    if (F == 0) return (int)p[0];
    if (Pix<F>::bpp == 4) {  // one dword, whatever its alignment
        uint32_t w;
        __builtin_memcpy(&w, p, 4);
        return gray_y((int)((w >> (8 * Pix<F>::red)) & 255u), (int)((w >> 8) & 255u),
                      (int)((w >> (8 * (2 - Pix<F>::red))) & 255u));
    }
    return gray_y((int)p[Pix<F>::red], (int)p[1], (int)p[2 - Pix<F>::red]);
}

}  // namespace sgm

// Runs CALL(F) with the run-time format as the compile-time F; a value that is
// no format makes the enclosing launch function fail (a missing kernel is an
// error).
#define SGM_PIX_DISPATCH(fmt, CALL)        \
    switch (fmt) {                         \
    case 0: CALL(0); break;                \
    case 1: CALL(1); break;                \
    case 2: CALL(2); break;                \
    case 3: CALL(3); break;                \
    case 4: CALL(4); break;                \
    default: return hipErrorInvalidValue;  \
    }
