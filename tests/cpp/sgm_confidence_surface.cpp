// The match-confidence surface of include/sgm_amd/SGM.h: set_confidence(true);
// process(l, r); get_confidence().
//   sgm_confidence_surface bm                      -> BM::set_confidence is refused
//   sgm_confidence_surface run L R H W D OUT CAPI  -> SGM(h, w, 1, d): raw u8 pair in;
//       OUT = get_confidence() as f32, CAPI = sgm_stage_confidence's left map of
//       the same handle; then set_confidence(false) must empty get_confidence()
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

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "bm") {
        try {
            sgm_amd::BM bm(48, 150, 1, 64);
            bm.set_confidence(true);
        } catch (const std::runtime_error &e) {
            std::printf("threw as expected: %s\n", e.what());
            return 0;
        }
        std::printf("did not throw\n");
        return 1;
    }
    if (argc == 9 && std::string(argv[1]) == "run") {
        const int h = std::atoi(argv[4]), w = std::atoi(argv[5]), d = std::atoi(argv[6]);
        Mat l(h, w, CV_8UC1), r(h, w, CV_8UC1);
        if (!read_image(argv[2], l) || !read_image(argv[3], r)) return 2;
        sgm_amd::SGM sgm(h, w, 1, d);
        if (!sgm.get_confidence().empty()) return 4;
        sgm.set_confidence(true);
        sgm.process(l, r);
        const Mat &conf = sgm.get_confidence();
        if (conf.rows != h || conf.cols != w || conf.type() != CV_32FC1) return 5;
        std::ofstream out(argv[7], std::ios::binary);
        for (int i = 0; i < conf.rows; ++i)
            out.write(reinterpret_cast<const char *>(conf.ptr<float>(i)),
                      (std::streamsize)conf.cols * sizeof(float));
        std::vector<float> capi((size_t)h * w);
        if (sgm_stage_confidence(sgm.handle(), SGM_VIEW_LEFT, capi.data()) != SGM_OK) return 6;
        std::ofstream out2(argv[8], std::ios::binary);
        out2.write(reinterpret_cast<const char *>(capi.data()), (std::streamsize)capi.size() * sizeof(float));
        sgm.set_confidence(false);
        sgm.process(l, r);
        if (!sgm.get_confidence().empty()) return 7;
        return out && out2 ? 0 : 3;
    }
    std::fprintf(stderr, "usage: %s bm | run L R H W D OUT CAPI\n", argv[0]);
    return 64;
}
