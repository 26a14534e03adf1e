// The five-argument SGM constructor of include/sgm_amd/SGM.h: SGM(h, w, s, d,
// paths), the reference class built with USE_8_PATH = false (inc/SGM.h:7).
//   sgm_paths4_surface badpaths               -> SGM(h, w, s, d, 5) is refused
//   sgm_paths4_surface run L R H W D OUT      -> SGM(h, w, 1, d, 4): raw u8 pair
//                                               in, get_disp() as f32 out
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
    if (argc >= 2 && std::string(argv[1]) == "badpaths") {
        try {
            sgm_amd::SGM sgm(48, 150, 1, 64, 5);
        } catch (const std::runtime_error &e) {
            std::printf("threw as expected: %s\n", e.what());
            return 0;
        }
        std::printf("did not throw\n");
        return 1;
    }
    if (argc == 8 && std::string(argv[1]) == "run") {
        const int h = std::atoi(argv[4]), w = std::atoi(argv[5]), d = std::atoi(argv[6]);
        Mat l(h, w, CV_8UC1), r(h, w, CV_8UC1);
        if (!read_image(argv[2], l) || !read_image(argv[3], r)) return 2;
        sgm_amd::SGM sgm(h, w, 1, d, 4);
        sgm.process(l, r);
        const Mat &disp = sgm.get_disp();
        std::ofstream out(argv[7], std::ios::binary);
        for (int i = 0; i < disp.rows; ++i)
            out.write(reinterpret_cast<const char *>(disp.ptr<float>(i)),
                      (std::streamsize)disp.cols * sizeof(float));
        return out ? 0 : 3;
    }
    std::fprintf(stderr, "usage: %s badpaths | run L R H W D OUT\n", argv[0]);
    return 64;
}
