// The host side of the input resize (stereo_matching_amd/csrc/sgm_resize_args.h:
// the size checks and the scale factors) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all resize_args_main.cpp
// Exits 0 when every check holds.
#include "../../stereo_matching_amd/csrc/sgm_resize_args.h"

#include <limits.h>
#include <string.h>

static int failures = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
        }                                                          \
    } while (0)

int main() {
    char why[24];  // shorter than every message: snprintf must truncate, not overrun
    EXPECT(sgm::input_size_ok(0, 0, why, sizeof(why)));
    EXPECT(sgm::input_size_ok(375, 1242, why, sizeof(why)));
    EXPECT(sgm::input_size_ok(1, 1, why, sizeof(why)));
    EXPECT(!sgm::input_size_ok(-1, 10, why, sizeof(why)) && strlen(why) == sizeof(why) - 1);
    EXPECT(!sgm::input_size_ok(10, -1, why, sizeof(why)));
    EXPECT(!sgm::input_size_ok(INT_MIN, INT_MIN, why, sizeof(why)));
    EXPECT(!sgm::input_size_ok(0, 10, why, sizeof(why)));
    EXPECT(!sgm::input_size_ok(10, 0, why, sizeof(why)));
    EXPECT(!sgm::input_size_ok(INT_MAX, INT_MAX, why, sizeof(why)));   // no overflow in the product
    EXPECT(sgm::input_size_ok(1, INT_MAX, why, sizeof(why)));
    EXPECT(!sgm::input_size_ok(2, INT_MAX, why, sizeof(why)));

    EXPECT(sgm::resize_src_ok(1, 1, 1, why, sizeof(why)));
    EXPECT(sgm::resize_src_ok(37, 53, 64, why, sizeof(why)));
    EXPECT(!sgm::resize_src_ok(37, 53, 52, why, sizeof(why)));
    EXPECT(!sgm::resize_src_ok(0, 53, 64, why, sizeof(why)));
    EXPECT(!sgm::resize_src_ok(37, 0, 64, why, sizeof(why)));
    EXPECT(!sgm::resize_src_ok(INT_MIN, 53, 64, why, sizeof(why)));
    EXPECT(!sgm::resize_src_ok(37, INT_MAX, INT_MAX - 1, why, sizeof(why)));

    sgm::ResizeScale s = sgm::resize_scale(2, 2, 1, 4);      // the worked case's columns
    EXPECT(s.x == 0.5 && s.y == 2.0 && !s.half);
    s = sgm::resize_scale(48, 160, 24, 80);
    EXPECT(s.half && s.x == 2.0 && s.y == 2.0);
    s = sgm::resize_scale(48, 161, 24, 80);
    EXPECT(!s.half);
    s = sgm::resize_scale(49, 160, 24, 80);
    EXPECT(!s.half);
    s = sgm::resize_scale(375, 1242, 360, 1240);
    EXPECT(s.x == 1.0 / (1240.0 / 1242.0) && s.y == 1.0 / (360.0 / 375.0) && !s.half);
    s = sgm::resize_scale(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
    EXPECT(s.x == 1.0 && s.y == 1.0 && !s.half);
    s = sgm::resize_scale(INT_MAX - 1, 2, (INT_MAX - 1) / 2, 1);   // 2 * dst computed without overflow
    EXPECT(s.half);
    s = sgm::resize_scale(2, 2, INT_MAX, INT_MAX);
    EXPECT(!s.half && s.x > 0.0);
    if (failures) return 1;
    printf("resize args ok\n");
    return 0;
}
