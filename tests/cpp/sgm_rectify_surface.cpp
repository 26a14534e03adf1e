// Rectification through include/sgm_amd/SGM.h: HipSolver::set_rectify,
// process() on raw camera-size images, HipSolver::remap, rectified() and
// rectify_valid().
//   sgm_rectify_surface bad                          -> bad arguments and a wrong-size image are refused
//   sgm_rectify_surface run L R MAPS SH SW H W D OUT -> SGM(h, w, 1, d) with set_rectify(sh, sw, maps):
//                                                       raw u8 pair and four h x w f32 planes (x_l, y_l,
//                                                       x_r, y_r) in; OUT.disp (get_disp, f32), OUT.left
//                                                       (rectified(0), u8), OUT.right (remap(r, 1), u8)
//                                                       and OUT.valid (rectify_valid(1), u8) out
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <fstream>
#include <vector>

using sgm_amd::Mat;

static bool read_plane(std::ifstream &f, Mat &m, size_t elem) {
    f.read(reinterpret_cast<char *>(m.data), (std::streamsize)((size_t)m.rows * m.cols * elem));
    return (bool)f;
}

static bool read_image(const char *path, Mat &m) {
    std::ifstream f(path, std::ios::binary);
    return read_plane(f, m, 1);
}

static bool write_rows(const std::string &path, const Mat &m, size_t elem) {
    std::ofstream out(path, std::ios::binary);
    for (int i = 0; i < m.rows; ++i)
        out.write(reinterpret_cast<const char *>(m.ptr<unsigned char>(i)), (std::streamsize)(m.cols * elem));
    return (bool)out;
}

template <typename F>
static bool refused(const char *what, F f) {
    try {
        f();
    } catch (const std::runtime_error &e) {
        std::printf("threw as expected: %s\n", e.what());
        return true;
    }
    std::printf("%s did not throw\n", what);
    return false;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "bad") {
        sgm_amd::SGM sgm(24, 80, 1, 32);
        Mat m(24, 80, CV_32FC1), small(24, 79, CV_32FC1), none, dst;
        bool ok = refused("a size above 32767", [&] { sgm.set_rectify(32768, 53, m, m, m, m); });
        ok = refused("one zero size", [&] { sgm.set_rectify(37, 0, m, m, m, m); }) && ok;
        ok = refused("a missing map", [&] { sgm.set_rectify(37, 53, m, m, m, none); }) && ok;
        ok = refused("a map of another size", [&] { sgm.set_rectify(37, 53, m, m, small, m); }) && ok;
        ok = refused("remap without maps", [&] { sgm.remap(Mat(37, 53, CV_8UC1), dst, 0); }) && ok;
        sgm.set_rectify(37, 53, m, m, m, m);
        ok = refused("an input size beside maps", [&] { sgm.set_input_size(40, 60); }) && ok;
        sgm.set_input_size(0, 0);  // switching the other stage off is allowed and changes nothing:
        Mat l(24, 80, CV_8UC1), r(24, 80, CV_8UC1);  // the constructed size is still the wrong one
        ok = refused("a full-size image", [&] { sgm.process(l, r); }) && ok;
        ok = refused("a view that is neither", [&] { sgm.remap(Mat(37, 53, CV_8UC1), dst, 2); }) && ok;
        sgm.set_rectify(0, 0, none, none, none, none);
        sgm.process(l, r);  // off: the constructed size again
        if (!sgm.rectified(0).empty()) ok = false;
        return ok ? 0 : 1;
    }
    if (argc == 11 && std::string(argv[1]) == "run") {
        const int sh = std::atoi(argv[5]), sw = std::atoi(argv[6]);
        const int h = std::atoi(argv[7]), w = std::atoi(argv[8]), d = std::atoi(argv[9]);
        const std::string out = argv[10];
        Mat l(sh, sw, CV_8UC1), r(sh, sw, CV_8UC1), maps[4];
        if (!read_image(argv[2], l) || !read_image(argv[3], r)) return 2;
        std::ifstream f(argv[4], std::ios::binary);
        for (Mat &m : maps) {
            m.create(h, w, CV_32FC1);
            if (!read_plane(f, m, sizeof(float))) return 2;
        }
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm.set_rectify(sh, sw, maps[0], maps[1], maps[2], maps[3]);
        sgm.process(l, r);
        const Mat &disp = sgm.get_disp();
        Mat right;
        sgm.remap(r, right, 1);
        std::printf("rectified %d %d and %d %d\n", sgm.rectified(0).rows, sgm.rectified(0).cols, right.rows,
                    right.cols);
        return write_rows(out + ".disp", disp, sizeof(float)) && write_rows(out + ".left", sgm.rectified(0), 1) &&
                       write_rows(out + ".right", right, 1) && write_rows(out + ".valid", sgm.rectify_valid(1), 1)
                   ? 0
                   : 3;
    }
    std::fprintf(stderr, "usage: %s bad | run L R MAPS SH SW H W D OUT\n", argv[0]);
    return 64;
}
