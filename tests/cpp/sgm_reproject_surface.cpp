// Reprojection through include/sgm_amd/SGM.h: HipSolver::set_reproject,
// clear_reproject, reproject(), xyz(), depth(), depth16() and the Mat shim's
// CV_32FC3 / CV_16UC1.
//   sgm_reproject_surface bad                     -> the refusals throw
//   sgm_reproject_surface run L R H W D Q MR OUT  -> SGM(h, w, 1, d) with set_reproject(Q, all three, MR, 1000):
//                                                    a u8 pair (h x w) and Q (16 doubles) in; OUT.disp (get_disp,
//                                                    f32), OUT.xyz (f32 x 3), OUT.depth (f32), OUT.depth16 (u16)
//                                                    and OUT.depth2 (reproject(get_disp) depth, f32) out
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <fstream>

using sgm_amd::Mat;

static bool read_image(const char *path, Mat &m) {
    std::ifstream f(path, std::ios::binary);
    for (int i = 0; i < m.rows; ++i)
        f.read(reinterpret_cast<char *>(m.ptr<unsigned char>(i)), (std::streamsize)m.cols);
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
        double q[16] = {1, 0, 0, -40, 0, 1, 0, -12, 0, 0, 0, 500, 0, 0, 8, 0};
        Mat x3(24, 80, CV_32FC3), u16(24, 80, CV_16UC1), g(24, 80, CV_8UC1), f(24, 80, CV_32FC1), z;
        bool ok = CV_32FC3 == 21 && CV_16UC1 == 2 && x3.channels() == 3 && x3.step == 960 && u16.step == 160 &&
                  u16.channels() == 1;
        ok = refused("xyz() before set_reproject", [&] { sgm.xyz(); }) && ok;
        ok = refused("reproject() before set_reproject", [&] { sgm.reproject(f, nullptr, &z, nullptr); }) && ok;
        ok = refused("unknown output bits", [&] { sgm.set_reproject(q, 8); }) && ok;
        ok = refused("no outputs", [&] { sgm.set_reproject(q, 0); }) && ok;
        ok = refused("a negative range", [&] { sgm.set_reproject(q, SGM_REPROJECT_XYZ, -1.0f); }) && ok;
        ok = refused("a zero depth scale", [&] { sgm.set_reproject(q, SGM_REPROJECT_DEPTH16, 0.0f, 0.0f); }) && ok;
        q[5] = 1.0 / 0.0;
        ok = refused("a Q that is not finite", [&] { sgm.set_reproject(q, SGM_REPROJECT_XYZ); }) && ok;
        q[5] = 1.0;
        sgm.set_reproject(q, SGM_REPROJECT_DEPTH);
        ok = refused("a product not asked for", [&] { sgm.depth16(); }) && ok;
        ok = refused("a map of the wrong type", [&] { sgm.reproject(g, nullptr, &z, nullptr); }) && ok;
        ok = refused("no product at all", [&] { sgm.reproject(f, nullptr, nullptr, nullptr); }) && ok;
        sgm.process(g, g);
        if (sgm.depth().rows != 24 || sgm.depth().cols != 80 || sgm.depth().type() != CV_32FC1) ok = false;
        sgm.clear_reproject();
        ok = refused("depth() after clear_reproject", [&] { sgm.depth(); }) && ok;
        sgm.process(g, g);  // off: frames as before
        return ok ? 0 : 1;
    }
    if (argc == 10 && std::string(argv[1]) == "run") {
        const int h = std::atoi(argv[4]), w = std::atoi(argv[5]), d = std::atoi(argv[6]);
        const float max_range = (float)std::atof(argv[8]);
        const std::string out = argv[9];
        Mat l(h, w, CV_8UC1), r(h, w, CV_8UC1);
        if (!read_image(argv[2], l) || !read_image(argv[3], r)) return 2;
        double q[16];
        std::ifstream fq(argv[7], std::ios::binary);
        if (!fq.read(reinterpret_cast<char *>(q), sizeof(q))) return 2;
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm.set_reproject(q, SGM_REPROJECT_XYZ | SGM_REPROJECT_DEPTH | SGM_REPROJECT_DEPTH16, max_range);
        sgm.process(l, r);
        Mat depth2;
        sgm.reproject(sgm.get_disp(), nullptr, &depth2, nullptr);
        std::printf("xyz %d %d x %d type %d, depth16 type %d\n", sgm.xyz().rows, sgm.xyz().cols,
                    sgm.xyz().channels(), sgm.xyz().type(), sgm.depth16().type());
        return write_rows(out + ".disp", sgm.get_disp(), 4) && write_rows(out + ".xyz", sgm.xyz(), 12) &&
                       write_rows(out + ".depth", sgm.depth(), 4) && write_rows(out + ".depth16", sgm.depth16(), 2) &&
                       write_rows(out + ".depth2", depth2, 4)
                   ? 0
                   : 3;
    }
    std::fprintf(stderr, "usage: %s bad | run L R H W D Q MAX_RANGE OUT\n", argv[0]);
    return 64;
}
