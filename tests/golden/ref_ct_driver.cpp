// Driver of tests/golden/make_ref_ct_golden.py: calls the reference's own CT
// (src/cost.cpp, compiled unmodified beside this file) per pixel and per
// disparity, as Solver::build_dsi (Solver.cpp:96-117) does, with `scale` passed
// (DESIGN.md 5s).  Built twice: plain, and with -DREF_CT_WEIGHTED against a
// cost.o compiled with -D'WEIGHTED_COST=(*ref_weighted_cost)' (see
// ref_weighted_driver.cpp), whose pointer this file then points at a true.  CT's
// prototype is declared here instead of including inc/cost.h, whose Solver.h
// would define that pointer a second time.
//   driver <request> <result>
// request: 7 int32 (rows, cols, D, scale, min_disp, e_h, e_w), then the
//          working-grid images L and R, rows * cols bytes each
// result:  rows * cols * D uint8, HWD, index d = disparity min_disp + d
// TEST INFRASTRUCTURE ONLY; this file holds none of the reference's text.
#include <opencv2/core/core.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

using cv::Mat;
using cv::Point;

int CT(const Mat &img_l, const Mat &img_r, const Point &l_pt, int disp, int win_h, int win_w, float *weight,
       int scale);

#ifdef REF_CT_WEIGHTED
extern const bool *ref_weighted_cost;
static const bool kOn = true;
#endif

int main(int argc, char **argv) {
    if (argc != 3) return 64;
#ifdef REF_CT_WEIGHTED
    ref_weighted_cost = &kOn;
#endif
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int head[7];
    if (std::fread(head, sizeof(int), 7, in) != 7) return 2;
    const int rows = head[0], cols = head[1], D = head[2], scale = head[3], min_disp = head[4];
    const int e_h = head[5], e_w = head[6];
    Mat L(rows, cols, CV_8UC1), R(rows, cols, CV_8UC1);
    for (int i = 0; i < rows; ++i)
        if (std::fread(L.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    for (int i = 0; i < rows; ++i)
        if (std::fread(R.ptr<uchar>(i), 1, (size_t)cols, in) != (size_t)cols) return 2;
    std::fclose(in);
    // the window's table, entry by entry as Solver.cpp:40 computes it (read only when weighted)
    std::vector<float> weight((size_t)e_h * e_w);
    for (int a = 0; a < e_h; ++a)
        for (int b = 0; b < e_w; ++b)
            weight[(size_t)a * e_w + b] = std::exp((std::pow(a - e_h / 2, 2) + std::pow(b - e_w / 2, 2)) / -25.0);
    std::vector<uint8_t> cost((size_t)rows * cols * D);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j)
            for (int d = 0; d < D; ++d) {
                const int c = CT(L, R, Point(j, i), d + min_disp, e_h, e_w, weight.data(), scale);
                if (c < 0 || c > 255) return 4;
                cost[((size_t)i * cols + j) * D + d] = (uint8_t)c;
            }
    FILE *out = std::fopen(argv[2], "wb");
    if (!out || std::fwrite(cost.data(), 1, cost.size(), out) != cost.size()) return 3;
    std::fclose(out);
    return 0;
}
