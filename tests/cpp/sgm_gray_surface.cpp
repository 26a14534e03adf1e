// Colour input through include/sgm_amd/SGM.h: HipSolver::set_input_format,
// process() on CV_8UC3 / CV_8UC4 Mats, HipSolver::gray and input_gray().
//   sgm_gray_surface bad                    -> bad formats and wrong-type images are refused
//   sgm_gray_surface run FMT L R H W D OUT  -> SGM(h, w, 1, d) with set_input_format(FMT): raw colour u8
//                                              pair (h x w x 3 or 4 bytes) in; OUT.disp (get_disp, f32),
//                                              OUT.left (input_gray(0), u8) and OUT.right (gray(r), u8) out
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <fstream>

using sgm_amd::Mat;

static bool read_image(const char *path, Mat &m) {
    std::ifstream f(path, std::ios::binary);
    for (int i = 0; i < m.rows; ++i)
        f.read(reinterpret_cast<char *>(m.ptr<unsigned char>(i)), (std::streamsize)(m.cols * m.channels()));
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
        Mat g(24, 80, CV_8UC1), c3(24, 80, CV_8UC3), c4(24, 80, CV_8UC4), dst;
        bool ok = c3.channels() == 3 && c4.channels() == 4 && c4.step == 320 && c3.step == 240;
        ok = refused("an unknown format", [&] { sgm.set_input_format(5); }) && ok;
        ok = refused("a colour image on a grey handle", [&] { sgm.process(c3, c3); }) && ok;
        ok = refused("gray() of a grey image", [&] { sgm.gray(g, dst, SGM_PIX_GRAY8); }) && ok;
        ok = refused("gray() of three channels as four", [&] { sgm.gray(c3, dst, SGM_PIX_BGRA8); }) && ok;
        if (!sgm.input_gray(0).empty()) ok = false;
        sgm.set_input_format(SGM_PIX_BGR8);
        ok = refused("a grey image on a colour handle", [&] { sgm.process(g, g); }) && ok;
        ok = refused("four channels on a three-channel handle", [&] { sgm.process(c4, c4); }) && ok;
        sgm.process(c3, c3);
        if (sgm.input_gray(1).rows != 24 || sgm.input_gray(1).cols != 80) ok = false;
        sgm.set_input_format(SGM_PIX_RGBA8);
        ok = refused("three channels on a four-channel handle", [&] { sgm.process(c3, c3); }) && ok;
        sgm.process(c4, c4);
        sgm.set_input_format(SGM_PIX_GRAY8);
        sgm.process(g, g);  // off: CV_8UC1 again
        if (!sgm.input_gray(0).empty()) ok = false;
        return ok ? 0 : 1;
    }
    if (argc == 9 && std::string(argv[1]) == "run") {
        const int fmt = std::atoi(argv[2]);
        const int h = std::atoi(argv[5]), w = std::atoi(argv[6]), d = std::atoi(argv[7]);
        const std::string out = argv[8];
        const int type = fmt == SGM_PIX_BGR8 || fmt == SGM_PIX_RGB8 ? CV_8UC3 : CV_8UC4;
        Mat l(h, w, type), r(h, w, type);
        if (!read_image(argv[3], l) || !read_image(argv[4], r)) return 2;
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm.set_input_format(fmt);
        sgm.process(l, r);
        const Mat &disp = sgm.get_disp();
        Mat right;
        sgm.gray(r, right, fmt);
        std::printf("grey %d %d and %d %d\n", sgm.input_gray(0).rows, sgm.input_gray(0).cols, right.rows,
                    right.cols);
        return write_rows(out + ".disp", disp, sizeof(float)) && write_rows(out + ".left", sgm.input_gray(0), 1) &&
                       write_rows(out + ".right", right, 1)
                   ? 0
                   : 3;
    }
    std::fprintf(stderr, "usage: %s bad | run FMT L R H W D OUT\n", argv[0]);
    return 64;
}
