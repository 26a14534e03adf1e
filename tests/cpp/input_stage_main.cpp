// The handle's input stage (stereo_matching_amd/csrc/sgm_input_stage.h: which
// launch a frame begins with, the shape of the images it takes, whether the
// handle stages them) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all input_stage_main.cpp
// Exits 0 when every check holds.  The expected values are written out, for a
// handle constructed 48 x 96.
#include "../../stereo_matching_amd/csrc/sgm_input_stage.h"

static int failures = 0;
#define EXPECT(c)                                                             \
    do {                                                                      \
        if (!(c)) {                                                           \
            ++failures;                                                       \
            fprintf(stderr, "line %d (stage %d, format %d): %s\n", __LINE__, s, f, #c); \
        }                                                                     \
    } while (0)

struct Want {
    sgm::InputKind kind;
    int rows, cols, row_bytes;
    bool stages;
    size_t raw_bytes;
};

int main() {
    using namespace sgm;
    // stage: 0 none, 1 an input size of 37 x 53, 2 maps reading 37 x 53, 3 those maps on an aux_only
    // handle (which runs no frames; its setters refuse a colour format, the struct does not care);
    // format: grey, BGR8, RGB8, BGRA8, RGBA8
    static const Want want[4][kPixFormats] = {
        {{INPUT_NONE, 48, 96, 96, false, 0},
         {INPUT_GRAY, 48, 96, 288, true, 13824},
         {INPUT_GRAY, 48, 96, 288, true, 13824},
         {INPUT_GRAY, 48, 96, 384, true, 18432},
         {INPUT_GRAY, 48, 96, 384, true, 18432}},
        {{INPUT_RESIZE, 37, 53, 53, true, 1961},
         {INPUT_RESIZE, 37, 53, 159, true, 5883},
         {INPUT_RESIZE, 37, 53, 159, true, 5883},
         {INPUT_RESIZE, 37, 53, 212, true, 7844},
         {INPUT_RESIZE, 37, 53, 212, true, 7844}},
        {{INPUT_RECTIFY, 37, 53, 53, true, 1961},
         {INPUT_RECTIFY, 37, 53, 159, true, 5883},
         {INPUT_RECTIFY, 37, 53, 159, true, 5883},
         {INPUT_RECTIFY, 37, 53, 212, true, 7844},
         {INPUT_RECTIFY, 37, 53, 212, true, 7844}},
        {{INPUT_RECTIFY, 37, 53, 53, false, 0},
         {INPUT_RECTIFY, 37, 53, 159, true, 5883},
         {INPUT_RECTIFY, 37, 53, 159, true, 5883},
         {INPUT_RECTIFY, 37, 53, 212, true, 7844},
         {INPUT_RECTIFY, 37, 53, 212, true, 7844}},
    };
    static const int bpp[kPixFormats] = {1, 3, 3, 4, 4};
    int s = -1, f = -1;
    EXPECT(InputStage().kind() == INPUT_NONE && !InputStage().stages(false));  // as sgm_create leaves it
    for (s = 0; s < 4; ++s)
        for (f = 0; f < kPixFormats; ++f) {
            InputStage in;
            if (s == 1) in.in_rows = 37, in.in_cols = 53;
            if (s >= 2) in.rc_rows = 37, in.rc_cols = 53;
            in.fmt = f;
            const bool aux_only = s == 3;
            const Want &w = want[s][f];
            EXPECT(in.kind() == w.kind);
            EXPECT(in.rows(48) == w.rows && in.cols(96) == w.cols);
            EXPECT(in.bpp() == bpp[f] && in.row_bytes(96) == w.row_bytes);
            EXPECT(in.stages(aux_only) == w.stages);
            EXPECT(in.raw_bytes(48, 96, aux_only) == w.raw_bytes);
        }
    s = f = -1;
    // the images stay addressable with an int (format 3: BGRA8, 4 bytes per pixel; 46341^2 =
    // 2147488281 is past 2^31 - 1 already at one byte, 46340^2 is not)
    EXPECT(!input_bytes_ok(3, 46341, 46341, 48, 96));
    EXPECT(input_bytes_ok(3, 1, 1, 48, 96));
    EXPECT(input_bytes_ok(0, 46340, 46340, 48, 96) && !input_bytes_ok(1, 46340, 46340, 48, 96));
    // no size given: the constructed one
    EXPECT(input_bytes_ok(3, 0, 0, 48, 96) && !input_bytes_ok(3, 0, 0, 46341, 46341));
    if (failures) return 1;
    printf("input stage ok\n");
    return 0;
}
