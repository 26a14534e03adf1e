// Driver of tests/golden/make_ref_window_cost_golden.py: calls the reference's
// own SAD and SSD (src/cost.cpp, compiled unmodified beside this file) per pixel
// and per disparity, as Solver::build_dsi (Solver.cpp:96-117) would.
//   driver <request> <result>
// request: 7 int32 (rows, cols, D, scale, min_disp, kind 1 = SAD / 2 = SSD, 0),
//          then the working-grid images L and R, rows * cols bytes each
// result:  rows * cols * D float32, HWD
// TEST INFRASTRUCTURE ONLY; this file holds none of the reference's text.
#include "inc/cost.h"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 64;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int head[7];
    if (std::fread(head, sizeof(int), 7, in) != 7) return 2;
    const int rows = head[0], cols = head[1], D = head[2], scale = head[3], min_disp = head[4], kind = head[5];
    Mat L(rows, cols, CV_8UC1), R(rows, cols, CV_8UC1);
    for (int i = 0; i < rows; ++i)
        if (std::fread(L.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    for (int i = 0; i < rows; ++i)
        if (std::fread(R.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    std::fclose(in);
    const int win_h = 7 / scale, win_w = 9 / scale;  // WIN_H / scale, WIN_W / scale (Solver.cpp:98-99)
    std::vector<float> cost((size_t)rows * cols * D);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j)
            for (int d = 0; d < D; ++d)
                cost[((size_t)i * cols + j) * D + d] =
                    kind == 2 ? SSD(L, R, Point(j, i), d + min_disp, win_h, win_w, nullptr, scale)
                              : SAD(L, R, Point(j, i), d + min_disp, win_h, win_w, nullptr, scale);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out || std::fwrite(cost.data(), sizeof(float), cost.size(), out) != cost.size()) return 3;
    std::fclose(out);
    return 0;
}
