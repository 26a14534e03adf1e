// The host side of the reprojection (stereo_matching_amd/csrc/
// sgm_reproject_args.h: the setter's and the device call's checks, the pinhole Q)
// on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all reproject_args_main.cpp
// Exits 0 when every check holds.
#include "../../stereo_matching_amd/csrc/sgm_reproject_args.h"

#include "../../include/sgm_hip.h"

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

static bool set_ok(const double *q, int outputs, float max_range, float depth_scale, bool aux, bool right,
                   char *why, size_t n) {
    return sgm::reproject_set_ok(q, outputs, max_range, depth_scale, aux, right, why, n);
}

// (Q set, map, pitch, xyz, xyz pitch, depth, depth pitch, depth16, depth16 pitch) on 53 columns
static bool call_ok(bool q, bool d, int p, bool x, int xp, bool z, int zp, bool u, int up, char *why, size_t n) {
    return sgm::reproject_call_ok(q, d, p, x, xp, z, zp, u, up, 53, why, n);
}

int main() {
    char why[24];  // shorter than every message: snprintf must truncate, not overrun
    const size_t n = sizeof(why);
    // the bits, against the public enum
    EXPECT(sgm::kReprojectXyz == SGM_REPROJECT_XYZ && sgm::kReprojectDepth == SGM_REPROJECT_DEPTH &&
           sgm::kReprojectDepth16 == SGM_REPROJECT_DEPTH16 && sgm::kReprojectAll == 7);
    double q[16];
    for (int k = 0; k < 16; ++k) q[k] = 0.25 * (k + 1);
    const float inf = __builtin_inff(), nan = __builtin_nanf("");

    // the setter: every acceptance
    for (int outputs = 1; outputs <= 7; ++outputs) {
        EXPECT(set_ok(q, outputs, 0.0f, 1000.0f, false, false, why, n));
        EXPECT(set_ok(q, outputs, 100.0f, 0.5f, true, false, why, n));
    }
    EXPECT(set_ok(q, 0, 0.0f, 1000.0f, true, false, why, n));   // Q alone: an aux_only handle
    EXPECT(set_ok(q, 3, 0.0f, 0.0f, false, false, why, n));     // depth_scale is depth16's alone
    EXPECT(set_ok(q, 3, 0.0f, nan, false, false, why, n));
    EXPECT(set_ok(q, 0, 0.0f, -1.0f, true, false, why, n));
    EXPECT(set_ok(q, 7, 3.0e38f, 1.0e-30f, false, false, why, n));
    // ... and every refusal
    EXPECT(!set_ok(q, 7, 0.0f, 1000.0f, false, true, why, n) && strstr(why, "SGM_VIEW_RIGHT") &&
           strlen(why) == n - 1);
    EXPECT(!set_ok(q, 0, 0.0f, 1000.0f, true, true, why, n));
    for (int k = 0; k < 16; ++k) {
        const double bad[3] = {(double)nan, (double)inf, -(double)inf};
        for (int b = 0; b < 3; ++b) {
            double qq[16];
            memcpy(qq, q, sizeof(qq));
            qq[k] = bad[b];
            EXPECT(!set_ok(qq, 7, 0.0f, 1000.0f, false, false, why, n) && strstr(why, "not finite"));
            EXPECT(!set_ok(qq, 0, 0.0f, 1000.0f, true, false, why, n));
        }
    }
    EXPECT(!set_ok(q, 8, 0.0f, 1000.0f, false, false, why, n) && strstr(why, "unknown bits"));
    EXPECT(!set_ok(q, 15, 0.0f, 1000.0f, true, false, why, n));
    EXPECT(!set_ok(q, -1, 0.0f, 1000.0f, false, false, why, n));
    EXPECT(!set_ok(q, INT_MIN, 0.0f, 1000.0f, false, false, why, n));
    EXPECT(!set_ok(q, INT_MAX, 0.0f, 1000.0f, false, false, why, n));
    EXPECT(!set_ok(q, 0, 0.0f, 1000.0f, false, false, why, n) && strstr(why, "outputs is 0"));
    EXPECT(!set_ok(q, 7, -1.0f, 1000.0f, false, false, why, n) && strstr(why, "max_range"));
    EXPECT(!set_ok(q, 7, -1.0e-45f, 1000.0f, false, false, why, n));   // the smallest negative
    EXPECT(!set_ok(q, 7, nan, 1000.0f, false, false, why, n));
    EXPECT(!set_ok(q, 7, inf, 1000.0f, false, false, why, n));
    EXPECT(!set_ok(q, 0, -inf, 1000.0f, true, false, why, n));
    const float scales[] = {0.0f, -0.0f, -1000.0f, nan, inf, -inf};
    for (float sc : scales) {
        EXPECT(!set_ok(q, 4, 0.0f, sc, false, false, why, n) && strstr(why, "depth_scale"));
        EXPECT(!set_ok(q, 7, 0.0f, sc, true, false, why, n));
        EXPECT(set_ok(q, 3, 0.0f, sc, false, false, why, n));
    }

    // the device call: every acceptance
    EXPECT(call_ok(true, true, 53, true, 159, true, 53, true, 53, why, n));
    EXPECT(call_ok(true, true, 60, true, 170, true, 61, true, 59, why, n));
    EXPECT(call_ok(true, true, 53, true, 159, false, 0, false, 0, why, n));        // a skipped product's pitch is not read
    EXPECT(call_ok(true, true, 53, false, -5, true, 53, false, INT_MIN, why, n));
    EXPECT(call_ok(true, true, 53, false, 0, false, 0, true, 53, why, n));
    EXPECT(call_ok(true, true, INT_MAX, true, INT_MAX, true, INT_MAX, true, INT_MAX, why, n));
    // ... and every refusal
    EXPECT(!call_ok(false, true, 53, true, 159, true, 53, true, 53, why, n) && strstr(why, "no Q is set"));
    EXPECT(!call_ok(true, false, 53, true, 159, true, 53, true, 53, why, n) && strstr(why, "NULL disparity"));
    EXPECT(!call_ok(true, true, 53, false, 159, false, 53, false, 53, why, n) && strstr(why, "all three"));
    EXPECT(!call_ok(true, true, 52, true, 159, true, 53, true, 53, why, n) && strstr(why, "pitch 52"));
    EXPECT(!call_ok(true, true, -1, true, 159, true, 53, true, 53, why, n));
    EXPECT(!call_ok(true, true, 53, true, 158, true, 53, true, 53, why, n) && strstr(why, "xyz_pitch"));
    EXPECT(!call_ok(true, true, 53, true, 53, false, 0, false, 0, why, n));
    EXPECT(!call_ok(true, true, 53, true, 159, true, 52, true, 53, why, n) && strstr(why, "depth_pitch"));
    EXPECT(!call_ok(true, true, 53, true, 159, true, 53, true, 52, why, n) && strstr(why, "depth16_pitch"));
    EXPECT(!call_ok(true, true, 53, false, 0, false, 0, true, INT_MIN, why, n));
    // 3 x cols past an int: compared in 64 bits
    EXPECT(!sgm::reproject_call_ok(true, true, INT_MAX, true, INT_MAX, false, 0, false, 0, INT_MAX, why, n));
    EXPECT(sgm::reproject_call_ok(true, true, INT_MAX, false, 0, true, INT_MAX, false, 0, INT_MAX, why, n));

    // one product at a time
    EXPECT(sgm::reproject_one_bit(1) && sgm::reproject_one_bit(2) && sgm::reproject_one_bit(4));
    EXPECT(!sgm::reproject_one_bit(0) && !sgm::reproject_one_bit(3) && !sgm::reproject_one_bit(7) &&
           !sgm::reproject_one_bit(8) && !sgm::reproject_one_bit(-1) && !sgm::reproject_one_bit(INT_MIN));
    EXPECT(sgm::reproject_channels(1) == 3 && sgm::reproject_channels(2) == 1 && sgm::reproject_channels(4) == 1);
    EXPECT(sgm::reproject_elem_bytes(1) == 4 && sgm::reproject_elem_bytes(2) == 4 &&
           sgm::reproject_elem_bytes(4) == 2);

    // the pinhole Q
    double c[16];
    EXPECT(sgm::camera_q(700.0f, 702.0f, 320.5f, 240.25f, 0.125, c));
    const double want[16] = {1, 0, 0, -320.5, 0, 1, 0, -240.25, 0, 0, 0, 701.0, 0, 0, 8.0, 0};
    EXPECT(memcmp(c, want, sizeof(c)) == 0);
    EXPECT(set_ok(c, 7, 0.0f, 1000.0f, false, false, why, n));
    EXPECT(!sgm::camera_q(700.0f, 700.0f, 320.0f, 240.0f, 0.0, c));
    EXPECT(!sgm::camera_q(700.0f, 700.0f, 320.0f, 240.0f, (double)nan, c));
    EXPECT(!sgm::camera_q(700.0f, 700.0f, 320.0f, 240.0f, 4.9e-324, c));   // 1 / baseline overflows
    EXPECT(!sgm::camera_q(inf, 700.0f, 320.0f, 240.0f, 0.5, c));
    EXPECT(!sgm::camera_q(700.0f, nan, 320.0f, 240.0f, 0.5, c));
    EXPECT(!sgm::camera_q(700.0f, 700.0f, inf, 240.0f, 0.5, c));
    EXPECT(!sgm::camera_q(700.0f, 700.0f, 320.0f, nan, 0.5, c));
    EXPECT(sgm::camera_q(3.0e38f, 3.0e38f, 0.0f, 0.0f, -0.5, c) && c[11] == 3.0e38f && c[14] == -2.0);
    if (failures) return 1;
    printf("reproject args ok\n");
    return 0;
}
