// The input resize through include/sgm_amd/SGM.h: HipSolver::set_input_size,
// process() on camera-size images, HipSolver::resize and get_resized.
//   sgm_resize_surface bad                          -> bad sizes and a wrong-size image are refused
//   sgm_resize_surface run L R SH SW H W D OUT      -> SGM(h, w, 1, d) with set_input_size(sh, sw):
//                                                      raw u8 pair in; OUT.disp (get_disp, f32),
//                                                      OUT.left (get_resized(0), u8) and OUT.right
//                                                      (resize(r), u8) out
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <fstream>
#include <vector>

using sgm_amd::Mat;

static bool read_image(const char *path, Mat &m) {
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(m.data), (std::streamsize)m.rows * m.cols);
    return (bool)f;
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
        bool ok = refused("a negative size", [&] { sgm.set_input_size(-1, 53); });
        ok = refused("one zero size", [&] { sgm.set_input_size(37, 0); }) && ok;
        sgm.set_input_size(37, 53);
        Mat l(24, 80, CV_8UC1), r(24, 80, CV_8UC1);  // the constructed size is now the wrong one
        ok = refused("a full-size image", [&] { sgm.process(l, r); }) && ok;
        Mat none, dst;
        ok = refused("an empty source", [&] { sgm.resize(none, dst); }) && ok;
        return ok ? 0 : 1;
    }
    if (argc == 10 && std::string(argv[1]) == "run") {
        const int sh = std::atoi(argv[4]), sw = std::atoi(argv[5]);
        const int h = std::atoi(argv[6]), w = std::atoi(argv[7]), d = std::atoi(argv[8]);
        const std::string out = argv[9];
        Mat l(sh, sw, CV_8UC1), r(sh, sw, CV_8UC1);
        if (!read_image(argv[2], l) || !read_image(argv[3], r)) return 2;
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm.set_input_size(sh, sw);
        sgm.process(l, r);
        const Mat &disp = sgm.get_disp();
        Mat right;
        sgm.resize(r, right);
        std::printf("resized %d %d and %d %d\n", sgm.get_resized(0).rows, sgm.get_resized(0).cols,
                    right.rows, right.cols);
        return write_rows(out + ".disp", disp, sizeof(float)) && write_rows(out + ".left", sgm.get_resized(0), 1) &&
                       write_rows(out + ".right", right, 1)
                   ? 0
                   : 3;
    }
    std::fprintf(stderr, "usage: %s bad | run L R SH SW H W D OUT\n", argv[0]);
    return 64;
}
