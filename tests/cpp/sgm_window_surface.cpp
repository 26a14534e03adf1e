// The matching window through include/sgm_amd/SGM.h: HipSolver::set_window, get_window.
//   sgm_window_surface bad                 -> the refusals throw and change nothing
//   sgm_window_surface frame <in> <out>    -> in: 5 int32 (h, w, d, win_h, win_w), then the grey
//                                             images l and r, h * w bytes each; out: get_disp()
//                                             of SGM::process(l, r) after set_window, h * w float32
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <cstdio>
#include <vector>

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
    if (argc == 2 && std::string(argv[1]) == "bad") {
        sgm_amd::SGM sgm(24, 80, 1, 32);
        sgm_amd::BM bm(24, 80, 2, 32);
        int wh = 0, ww = 0;
        sgm.get_window(&wh, &ww);
        bool ok = wh == 7 && ww == 9;
        sgm.set_window(5, 7);
        ok = refused("9 x 9", [&] { sgm.set_window(9, 9); }) && ok;
        ok = refused("1 x 1", [&] { sgm.set_window(1, 1); }) && ok;
        ok = refused("a zero height", [&] { sgm.set_window(0, 9); }) && ok;
        ok = refused("a negative width", [&] { sgm.set_window(7, -9); }) && ok;
        ok = refused("11 wide", [&] { sgm.set_window(7, 11); }) && ok;
        sgm.get_window(&wh, &ww);
        ok = ok && wh == 5 && ww == 7;
        // a BM at scale 2: (3, 3) is 1 x 1 there, (18, 18) is 9 x 9, (10, 12) is 5 x 6
        ok = refused("1 x 1 at scale 2", [&] { bm.set_window(3, 3); }) && ok;
        ok = refused("9 x 9 at scale 2", [&] { bm.set_window(18, 18); }) && ok;
        bm.set_window(10, 12);
        bm.get_window(&wh, &ww);
        ok = ok && wh == 10 && ww == 12;
        return ok ? 0 : 1;
    }
    if (argc == 4 && std::string(argv[1]) == "frame") {
        FILE *in = std::fopen(argv[2], "rb");
        int head[5];
        if (!in || std::fread(head, sizeof(int), 5, in) != 5) return 2;
        const int h = head[0], w = head[1], d = head[2];
        sgm_amd::Mat ml(h, w, CV_8UC1), mr(h, w, CV_8UC1);
        for (int i = 0; i < h; ++i)
            if (std::fread(ml.ptr<uint8_t>(i), 1, (size_t)w, in) != (size_t)w) return 2;
        for (int i = 0; i < h; ++i)
            if (std::fread(mr.ptr<uint8_t>(i), 1, (size_t)w, in) != (size_t)w) return 2;
        std::fclose(in);
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm.set_window(head[3], head[4]);
        sgm.process(ml, mr);
        const sgm_amd::Mat &disp = sgm.get_disp();
        FILE *out = std::fopen(argv[3], "wb");
        if (!out) return 3;
        for (int i = 0; i < h; ++i)
            if (std::fwrite(disp.ptr<float>(i), sizeof(float), (size_t)w, out) != (size_t)w) return 3;
        std::fclose(out);
        return 0;
    }
    std::fprintf(stderr, "usage: %s bad | frame <in> <out>\n", argv[0]);
    return 64;
}
