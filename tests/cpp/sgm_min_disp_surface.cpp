// The six-argument SGM constructor of include/sgm_amd/SGM.h: SGM(h, w, s, d,
// paths, min_disp), a matcher that searches disparities [min_disp, min_disp + d).
//   sgm_min_disp_surface bad                    -> min_disp = -1, 1 at scale 2 and
//                                                  65535 - d are refused
//   sgm_min_disp_surface run L R H W D M OUT    -> SGM(h, w, 1, d, 8, m): raw u8 pair
//                                                  in, get_disp() as f32 out, the
//                                                  invalid value on stdout
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

static bool refused(int s, int d, int m) {
    try {
        sgm_amd::SGM sgm(48, 150, s, d, 8, m);
    } catch (const std::runtime_error &e) {
        std::printf("threw as expected: %s\n", e.what());
        return true;
    }
    std::printf("min_disp %d at scale %d, d %d did not throw\n", m, s, d);
    return false;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "bad")
        return refused(1, 64, -1) && refused(2, 64, 1) && refused(1, 64, 65535 - 64) ? 0 : 1;
    if (argc == 9 && std::string(argv[1]) == "run") {
        const int h = std::atoi(argv[4]), w = std::atoi(argv[5]), d = std::atoi(argv[6]);
        const int m = std::atoi(argv[7]);
        Mat l(h, w, CV_8UC1), r(h, w, CV_8UC1);
        if (!read_image(argv[2], l) || !read_image(argv[3], r)) return 2;
        sgm_amd::SGM sgm(h, w, 1, d, 8, m);
        sgm.process(l, r);
        const Mat &disp = sgm.get_disp();
        std::printf("invalid %d min_disp %d\n", sgm.get_invalid_disp(), sgm.get_min_disp());
        std::ofstream out(argv[8], std::ios::binary);
        for (int i = 0; i < disp.rows; ++i)
            out.write(reinterpret_cast<const char *>(disp.ptr<float>(i)),
                      (std::streamsize)disp.cols * sizeof(float));
        return out ? 0 : 3;
    }
    std::fprintf(stderr, "usage: %s bad | run L R H W D M OUT\n", argv[0]);
    return 64;
}
