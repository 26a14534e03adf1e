// The median fill's launch budget through the C++ class surface
// (include/sgm_amd/SGM.h set_post_filter_launches, BatchSGM's constructor
// argument): frames whose post filter never waits on the host.
//   post_filter_async run PREFIX N H W D BUDGET OUT
//       sgm_amd::SGM(h, w, 1, d) with set_post_filter_launches(BUDGET), then
//       process() of pairs PREFIX_l<k>.raw / PREFIX_r<k>.raw, k < N, on the one
//       object; their get_disp() maps to OUT in pair order.  Budgets -1 and
//       4097 must be refused first.
//   post_filter_async batch PREFIX N H W D BUDGET OUT
//       the same pairs through BatchSGM(devices, h, w, 1, d, BUDGET) on the
//       devices of SGM_AMD_DEVICES (default "0")
#define SGM_AMD_THROW 1
#include "sgm_amd/BatchSGM.h"
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <fstream>
#include <vector>

using sgm_amd::Mat;

static bool read_pairs(const std::string &prefix, int n, int h, int w, std::vector<Mat> &ls,
                       std::vector<Mat> &rs) {
    for (int k = 0; k < n; ++k) {
        Mat l(h, w, CV_8UC1), r(h, w, CV_8UC1);
        std::ifstream fl(prefix + "_l" + std::to_string(k) + ".raw", std::ios::binary),
            fr(prefix + "_r" + std::to_string(k) + ".raw", std::ios::binary);
        fl.read(reinterpret_cast<char *>(l.data), (std::streamsize)h * w);
        fr.read(reinterpret_cast<char *>(r.data), (std::streamsize)h * w);
        if (!fl || !fr) return false;
        ls.push_back(l);
        rs.push_back(r);
    }
    return true;
}

static void write_map(std::ofstream &fo, const Mat &disp) {
    for (int i = 0; i < disp.rows; ++i)
        fo.write(reinterpret_cast<const char *>(disp.ptr<float>(i)), (std::streamsize)disp.cols * 4);
}

static int refused(sgm_amd::SGM &sgm, int n) {
    try {
        sgm.set_post_filter_launches(n);
    } catch (const std::runtime_error &e) {
        std::printf("budget %d refused: %s\n", n, e.what());
        return 0;
    }
    std::printf("budget %d was accepted\n", n);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 9) return 64;
    const std::string mode = argv[1], prefix = argv[2];
    const int n = std::atoi(argv[3]), h = std::atoi(argv[4]), w = std::atoi(argv[5]),
              d = std::atoi(argv[6]), budget = std::atoi(argv[7]);
    std::vector<Mat> ls, rs;
    if (!read_pairs(prefix, n, h, w, ls, rs)) return 2;
    std::ofstream fo(argv[8], std::ios::binary);
    if (mode == "run") {
        sgm_amd::SGM sgm(h, w, 1, d);
        if (refused(sgm, -1) + refused(sgm, 4097)) return 3;
        sgm.set_post_filter_launches(budget);
        for (int k = 0; k < n; ++k) {
            sgm.process(ls[k], rs[k]);  // an unproven fill would throw here
            write_map(fo, sgm.get_disp());
        }
        std::printf("%d frames with a budget of %d\n", n, budget);
        return fo ? 0 : 4;
    }
    if (mode == "batch") {
        std::vector<int> devices;
        const char *env = std::getenv("SGM_AMD_DEVICES");
        for (const char *c = env && *env ? env : "0"; *c;) {
            devices.push_back(std::atoi(c));
            while (*c && *c != ',') ++c;
            if (*c == ',') ++c;
        }
        sgm_amd::BatchSGM batch(devices, h, w, 1, d, budget);
        batch.process(ls, rs);
        for (int k = 0; k < n; ++k) write_map(fo, batch.get_disp(k));
        std::printf("batch of %d pairs on %d device(s) with a budget of %d\n", n, batch.devices(), budget);
        return fo ? 0 : 4;
    }
    return 64;
}
