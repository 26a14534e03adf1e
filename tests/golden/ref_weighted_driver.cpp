// Driver of tests/golden/make_ref_weighted_golden.py: calls the reference's own
// CT_pts, SAD and SSD (src/cost.cpp, compiled unmodified beside this file) with
// WEIGHTED_COST switched on.  The script compiles cost.cpp with
// -D'WEIGHTED_COST=(*ref_weighted_cost)', which turns the constant's definition in
// inc/Solver.h into a global `const bool *ref_weighted_cost` that every
// `if (WEIGHTED_COST)` reads through; this file points it at a true.  The three
// prototypes are declared here instead of including inc/cost.h, whose Solver.h
// would define the pointer a second time.
//   driver <request> <result>
// request: 7 int32 (rows, cols, D, scale, e_h, e_w, mode 0 = CT_pts / 1 = SAD / 2 = SSD /
//          3 = the weight table alone), then the working-grid images L and R, rows * cols
//          bytes each
// result:  mode 0: the tables of L and of R, rows * cols uint64 each
//          mode 1, 2: rows * cols * D float32, HWD, index d = disparity d
//          mode 3: e_h * e_w float32, the table Solver::Solver builds (Solver.cpp:29-45)
// TEST INFRASTRUCTURE ONLY; this file holds none of the reference's text.
#include <opencv2/core/core.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

using cv::Mat;
using cv::Point;

float SAD(const Mat &img_l, const Mat &img_r, const Point &l_pt, int disp, int win_h, int win_w, float *weight,
          int scale);
float SSD(const Mat &img_l, const Mat &img_r, const Point &l_pt, int disp, int win_h, int win_w, float *weight,
          int scale);
void CT_pts(const Mat &img_l, const Mat &img_r, int u, int v, int win_h, int win_w, float *weight,
            uint64_t *cost_table_l, uint64_t *cost_table_r);

extern const bool *ref_weighted_cost;
static const bool kOn = true;

int main(int argc, char **argv) {
    if (argc != 3) return 64;
    ref_weighted_cost = &kOn;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int head[7];
    if (std::fread(head, sizeof(int), 7, in) != 7) return 2;
    const int rows = head[0], cols = head[1], D = head[2], scale = head[3], e_h = head[4], e_w = head[5];
    const int mode = head[6];
    // the window's table, entry by entry as Solver.cpp:40 computes it (double, stored as float)
    std::vector<float> weight((size_t)e_h * e_w);
    for (int a = 0; a < e_h; ++a)
        for (int b = 0; b < e_w; ++b)
            weight[(size_t)a * e_w + b] = std::exp((std::pow(a - e_h / 2, 2) + std::pow(b - e_w / 2, 2)) / -25.0);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 3;
    if (mode == 3) {
        if (std::fwrite(weight.data(), sizeof(float), weight.size(), out) != weight.size()) return 3;
        std::fclose(in);
        std::fclose(out);
        return 0;
    }
    Mat L(rows, cols, CV_8UC1), R(rows, cols, CV_8UC1);
    for (int i = 0; i < rows; ++i)
        if (std::fread(L.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    for (int i = 0; i < rows; ++i)
        if (std::fread(R.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    std::fclose(in);
    if (mode == 0) {
        std::vector<uint64_t> ctl((size_t)rows * cols), ctr((size_t)rows * cols);
        for (int v = 0; v < rows; ++v)
            for (int u = 0; u < cols; ++u) CT_pts(L, R, u, v, e_h, e_w, weight.data(), ctl.data(), ctr.data());
        if (std::fwrite(ctl.data(), sizeof(uint64_t), ctl.size(), out) != ctl.size()) return 3;
        if (std::fwrite(ctr.data(), sizeof(uint64_t), ctr.size(), out) != ctr.size()) return 3;
    } else {
        std::vector<float> cost((size_t)rows * cols * D);
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                for (int d = 0; d < D; ++d)
                    cost[((size_t)i * cols + j) * D + d] =
                        mode == 2 ? SSD(L, R, Point(j, i), d, e_h, e_w, weight.data(), scale)
                                  : SAD(L, R, Point(j, i), d, e_h, e_w, weight.data(), scale);
        if (std::fwrite(cost.data(), sizeof(float), cost.size(), out) != cost.size()) return 3;
    }
    std::fclose(out);
    return 0;
}
