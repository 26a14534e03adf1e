// The hole-filling surface of include/sgm_amd/SGM.h: set_fill(mode); process(l, r);
// get_disp(); get_fill_mask().
//   sgm_fill_surface refuse                          -> BM::set_fill(SGM_FILL_INTERPOLATE) is refused
//   sgm_fill_surface run KIND L R H W D MODE DISP MASK
//       KIND sgm | bm | gpu_sgm at (h, w, 1, d): raw u8 pair in; DISP = get_disp() as f32,
//       MASK = get_fill_mask() as u8; then set_fill(SGM_FILL_OFF) must empty get_fill_mask()
#define SGM_AMD_THROW 1
#include "sgm_amd/GPU_SGM.h"
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <fstream>
#include <string>

using sgm_amd::Mat;

static bool read_image(const char *path, Mat &m) {
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(m.data), (std::streamsize)m.rows * m.cols);
    return (bool)f;
}

template <typename S>
static int run(S &solver, Mat &l, Mat &r, int mode, const char *disp_path, const char *mask_path) {
    if (!solver.get_fill_mask().empty()) return 4;
    solver.set_fill(mode);
    solver.process(l, r);
    const Mat &disp = solver.get_disp();
    const Mat &mask = solver.get_fill_mask();
    if (mask.rows != disp.rows || mask.cols != disp.cols || mask.type() != CV_8UC1 || disp.type() != CV_32FC1) return 5;
    std::ofstream out(disp_path, std::ios::binary), out2(mask_path, std::ios::binary);
    for (int i = 0; i < disp.rows; ++i) {
        out.write(reinterpret_cast<const char *>(disp.template ptr<float>(i)), (std::streamsize)disp.cols * sizeof(float));
        out2.write(reinterpret_cast<const char *>(mask.template ptr<unsigned char>(i)), (std::streamsize)mask.cols);
    }
    solver.set_fill(SGM_FILL_OFF);
    solver.process(l, r);
    if (!solver.get_fill_mask().empty()) return 7;
    return out && out2 ? 0 : 3;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "refuse") {
        try {
            sgm_amd::BM bm(48, 96, 1, 32);
            bm.set_fill(SGM_FILL_INTERPOLATE);
        } catch (const std::runtime_error &e) {
            std::printf("threw as expected: %s\n", e.what());
            return 0;
        }
        std::printf("did not throw\n");
        return 1;
    }
    if (argc == 11 && std::string(argv[1]) == "run") {
        const std::string kind = argv[2];
        const int h = std::atoi(argv[5]), w = std::atoi(argv[6]), d = std::atoi(argv[7]), mode = std::atoi(argv[8]);
        Mat l(h, w, CV_8UC1), r(h, w, CV_8UC1);
        if (!read_image(argv[3], l) || !read_image(argv[4], r)) return 2;
        if (kind == "sgm") {
            sgm_amd::SGM s(h, w, 1, d);
            return run(s, l, r, mode, argv[9], argv[10]);
        }
        if (kind == "bm") {
            sgm_amd::BM s(h, w, 1, d);
            return run(s, l, r, mode, argv[9], argv[10]);
        }
        if (kind == "gpu_sgm") {
            sgm_amd::GPU_SGM s(h, w, 1, d);
            return run(s, l, r, mode, argv[9], argv[10]);
        }
    }
    std::fprintf(stderr, "usage: %s refuse | run KIND L R H W D MODE DISP MASK\n", argv[0]);
    return 64;
}
