// Driver of tests/golden/make_ref_window_golden.py: calls the reference's own
// CT_pts, SAD and SSD (src/cost.cpp, compiled unmodified beside this file) with a
// window handed in at run time, per pixel (and per disparity), as
// Solver::build_cost_table (Solver.cpp:120-140) and Solver::build_dsi
// (Solver.cpp:96-117) call them with WIN_H / scale, WIN_W / scale.
//   driver <request> <result>
// request: 7 int32 (rows, cols, D, scale, e_h, e_w, mode 0 = CT_pts / 1 = SAD / 2 = SSD),
//          then the working-grid images L and R, rows * cols bytes each
// result:  mode 0: the tables of L and of R, rows * cols uint64 each
//          else:   rows * cols * D float32, HWD, index d = disparity d
// TEST INFRASTRUCTURE ONLY; this file holds none of the reference's text.
#include "inc/cost.h"

#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 64;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int head[7];
    if (std::fread(head, sizeof(int), 7, in) != 7) return 2;
    const int rows = head[0], cols = head[1], D = head[2], scale = head[3], e_h = head[4], e_w = head[5];
    const int mode = head[6];
    Mat L(rows, cols, CV_8UC1), R(rows, cols, CV_8UC1);
    for (int i = 0; i < rows; ++i)
        if (std::fread(L.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    for (int i = 0; i < rows; ++i)
        if (std::fread(R.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    std::fclose(in);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 3;
    if (mode == 0) {
        std::vector<uint64_t> ctl((size_t)rows * cols), ctr((size_t)rows * cols);
        for (int v = 0; v < rows; ++v)
            for (int u = 0; u < cols; ++u) CT_pts(L, R, u, v, e_h, e_w, nullptr, ctl.data(), ctr.data());
        if (std::fwrite(ctl.data(), sizeof(uint64_t), ctl.size(), out) != ctl.size()) return 3;
        if (std::fwrite(ctr.data(), sizeof(uint64_t), ctr.size(), out) != ctr.size()) return 3;
    } else {
        std::vector<float> cost((size_t)rows * cols * D);
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                for (int d = 0; d < D; ++d)
                    cost[((size_t)i * cols + j) * D + d] = mode == 2 ? SSD(L, R, Point(j, i), d, e_h, e_w, nullptr, scale)
                                                                     : SAD(L, R, Point(j, i), d, e_h, e_w, nullptr, scale);
        if (std::fwrite(cost.data(), sizeof(float), cost.size(), out) != cost.size()) return 3;
    }
    std::fclose(out);
    return 0;
}
