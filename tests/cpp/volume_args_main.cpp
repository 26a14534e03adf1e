// The host side of the caller's cost volume (stereo_matching_amd/csrc/
// sgm_volume_args.h: the stride rule, the layout, the source's extent) on the
// CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all volume_args_main.cpp
// Exits 0 when every check holds.
#include "../../stereo_matching_amd/csrc/sgm_volume_args.h"

#include "../../include/sgm_hip.h"

#include <string.h>

static int failures = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
        }                                                          \
    } while (0)

static char why[40];  // shorter than most messages: snprintf must truncate, not overrun

// the layout of strides (row, col, disp) on a 7 x 33 x 64 grid
static sgm::VolLayout lay(long long sr, long long sc, long long sd, int dtype = SGM_VOL_F32) {
    return sgm::volume_layout(dtype, sr, sc, sd, 7, 33, 64, why, sizeof(why));
}

int main() {
    const int H = 7, W = 33, D = 64;
    EXPECT(sgm::kVolF32 == SGM_VOL_F32 && sgm::kVolF16 == SGM_VOL_F16);
    EXPECT(sgm::volume_elem_bytes(SGM_VOL_F32) == 4 && sgm::volume_elem_bytes(SGM_VOL_F16) == 2 &&
           sgm::volume_elem_bytes(2) == 0 && sgm::volume_elem_bytes(-1) == 0);

    // accepted: dense HWD, dense DHW, padded, a batch slice
    EXPECT(lay(W * D, D, 1) == sgm::VOL_LAYOUT_HWD);
    EXPECT(lay(W, 1, H * W) == sgm::VOL_LAYOUT_DHW);
    EXPECT(lay(W * D, D, 1, SGM_VOL_F16) == sgm::VOL_LAYOUT_HWD);
    EXPECT(lay(W, 1, H * W, SGM_VOL_F16) == sgm::VOL_LAYOUT_DHW);
    EXPECT(lay((D + 3) * W + 5, D + 3, 1) == sgm::VOL_LAYOUT_HWD);       // padded columns and rows
    EXPECT(lay(W + 3, 1, (W + 3) * H + 5) == sgm::VOL_LAYOUT_DHW);       // padded rows and planes
    EXPECT(lay(W, 1, 3LL * H * W) == sgm::VOL_LAYOUT_DHW);               // planes of another tensor between
    EXPECT(lay(D * W * 1000, D, 1) == sgm::VOL_LAYOUT_HWD);
    EXPECT(lay(D, D * H, 1) == sgm::VOL_LAYOUT_HWD);                     // a transposed (W, H, D) tensor
    EXPECT(lay(1LL << 40, 1, 1LL << 50) == sgm::VOL_LAYOUT_DHW);
    // refused: both 1, neither 1, overlapping, negative, a bad dtype
    EXPECT(lay(W * D, 1, 1) == sgm::VOL_LAYOUT_BAD && strstr(why, "both 1"));
    EXPECT(lay(W * D * 2, 2 * D, 2) == sgm::VOL_LAYOUT_BAD && strstr(why, "neither"));
    EXPECT(lay(W * D, D, 0) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(W * D, D - 1, 1) == sgm::VOL_LAYOUT_BAD && strstr(why, "overlapping") && strlen(why) == sizeof(why) - 1);
    EXPECT(lay(W * D - 1, D, 1) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(0, D, 1) == sgm::VOL_LAYOUT_BAD);                         // every row on the first
    EXPECT(lay(W - 1, 1, H * W) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(W, 1, H * W - 1) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(W, 1, 0) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(D, D, 1) == sgm::VOL_LAYOUT_BAD);                         // equal strides
    EXPECT(lay(-W * D, D, 1) == sgm::VOL_LAYOUT_BAD && strstr(why, "negative"));
    EXPECT(lay(W * D, -D, 1) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(W, 1, -H * W) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(LLONG_MIN, D, 1) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(W * D, D, 1, 2) == sgm::VOL_LAYOUT_BAD && strstr(why, "dtype"));
    EXPECT(lay(W * D, D, 1, -1) == sgm::VOL_LAYOUT_BAD);
    // strides past a 64-bit byte offset: refused, not overflowed
    EXPECT(lay(LLONG_MAX, D, 1) == sgm::VOL_LAYOUT_BAD && strstr(why, "64-bit"));
    EXPECT(lay(LLONG_MAX / 8, D, 1) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(W, 1, LLONG_MAX / 64) == sgm::VOL_LAYOUT_BAD);
    EXPECT(lay(LLONG_MAX / 16 / H, D, 1) == sgm::VOL_LAYOUT_HWD);
    // an empty grid
    EXPECT(sgm::volume_layout(SGM_VOL_F32, 1, 1, 1, 0, 5, 32, why, sizeof(why)) == sgm::VOL_LAYOUT_BAD);
    // the degenerate extents, which handles cannot have: both strides 1 is then no overlap
    EXPECT(sgm::volume_layout(SGM_VOL_F32, 5, 1, 1, 3, 5, 1, why, sizeof(why)) == sgm::VOL_LAYOUT_DHW);
    EXPECT(sgm::volume_layout(SGM_VOL_F32, 32, 1, 1, 3, 1, 32, why, sizeof(why)) == sgm::VOL_LAYOUT_HWD);

    // the extent: one past the last element, by brute force over the corners
    const long long cases[][3] = {{W * D, D, 1}, {W, 1, H * W}, {(D + 3) * W + 5, D + 3, 1}, {W + 3, 1, (W + 3) * H + 5}};
    for (const auto &c : cases) {
        long long last = 0;
        for (int i = 0; i < H; i += H - 1)
            for (int j = 0; j < W; j += W - 1)
                for (int d = 0; d < D; d += D - 1) {
                    const long long at = i * c[0] + j * c[1] + d * c[2];
                    if (at > last) last = at;
                }
        EXPECT(sgm::volume_extent_elems(c[0], c[1], c[2], H, W, D) == last + 1);
        EXPECT(sgm::volume_extent_bytes(SGM_VOL_F16, c[0], c[1], c[2], H, W, D) == 2 * (last + 1));
        EXPECT(sgm::volume_extent_bytes(SGM_VOL_F32, c[0], c[1], c[2], H, W, D) == 4 * (last + 1));
    }
    EXPECT(sgm::volume_extent_elems(W * D, D, 1, H, W, D) == (long long)H * W * D);
    // the accepted strides never put two elements on one address (a small grid, every element)
    {
        const int h = 3, w = 5, d = 4;
        const long long ok[][3] = {{20, 4, 1}, {5, 1, 15}, {23, 4, 1}, {7, 1, 30}, {4, 12, 1}};
        for (const auto &c : ok) {
            EXPECT(sgm::volume_layout(SGM_VOL_F32, c[0], c[1], c[2], h, w, d, why, sizeof(why)) != sgm::VOL_LAYOUT_BAD);
            bool seen[128] = {};
            bool clash = false;
            for (int i = 0; i < h; ++i)
                for (int j = 0; j < w; ++j)
                    for (int k = 0; k < d; ++k) {
                        const long long at = i * c[0] + j * c[1] + k * c[2];
                        if (at >= 128 || seen[at]) clash = true;
                        else seen[at] = true;
                    }
            EXPECT(!clash);
        }
    }
    if (failures) return 1;
    printf("volume args ok\n");
    return 0;
}
