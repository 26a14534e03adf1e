// The CT cost through include/sgm_amd/SGM.h: HipSolver::set_cost, cost and
// window_cost_device with SGM_COST_CT.
//   sgm_ct_cost_surface run -> the refusals throw; a constant pair then runs
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <hip/hip_runtime_api.h>

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
    if (argc >= 2 && std::string(argv[1]) == "run") {
        static_assert(SGM_COST_CT == 4, "3 is no kind");
        const int h = 24, w = 80, d = 32;
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm_amd::BM bm(h, w, 1, d);
        uint8_t *img = nullptr;
        float *vol = nullptr;
        if (hipMalloc((void **)&img, 2 * h * w) != hipSuccess ||
            hipMalloc((void **)&vol, sizeof(float) * h * w * d) != hipSuccess)
            return 2;
        // left all 9, right all 5: no tap is above its centre in either image, every CT cost is 0
        if (hipMemset(img, 9, h * w) != hipSuccess || hipMemset(img + h * w, 5, h * w) != hipSuccess ||
            hipMemset(vol, 0x7f, sizeof(float) * h * w * d) != hipSuccess)
            return 2;
        const uint8_t *l = img, *r = img + h * w;
        bool ok = sgm.cost() == SGM_COST_CENSUS;
        ok = refused("kind 3", [&] { sgm.set_cost(3); }) && ok;
        ok = refused("kind 3 as a window cost", [&] { sgm.window_cost_device(3, l, r, w, vol); }) && ok;
        ok = refused("a BM handle", [&] { bm.set_cost(SGM_COST_CT); }) && ok;
        ok = refused("a NULL image", [&] { sgm.window_cost_device(SGM_COST_CT, nullptr, r, w, vol); }) && ok;
        ok = refused("the legacy stream", [&] { sgm.window_cost_device(SGM_COST_CT, l, r, w, vol, hipStreamLegacy); }) &&
             ok;
        std::vector<float> c((size_t)h * w * d, -1.0f);
        sgm.window_cost_device(SGM_COST_CT, l, r, w, vol);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(c.data(), vol, c.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return 2;
        for (float x : c) ok = ok && x == 0.0f;
        std::printf("constant pair: cost[0] = %g\n", c[0]);
        // a frame on the cost runs, and cost() reads it back
        sgm.set_cost(SGM_COST_CT);
        ok = ok && sgm.cost() == SGM_COST_CT;
        sgm_amd::Mat ml(h, w, CV_8UC1), mr(h, w, CV_8UC1);
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) {
                ml.at<uint8_t>(i, j) = (uint8_t)(9 + (i * 7 + j * 13) % 50);
                mr.at<uint8_t>(i, j) = (uint8_t)(9 + (i * 7 + (j + 3) * 13) % 50);
            }
        sgm.process(ml, mr);
        const sgm_amd::Mat &disp = sgm.get_disp();
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) ok = ok && disp.at<float>(i, j) >= 0.0f && disp.at<float>(i, j) <= (float)(d + 1);
        ok = ok && sgm.cost() == SGM_COST_CT;
        sgm.set_cost(SGM_COST_CENSUS);
        ok = ok && sgm.cost() == SGM_COST_CENSUS;
        hipFree(img);
        hipFree(vol);
        return ok ? 0 : 1;
    }
    std::fprintf(stderr, "usage: %s run\n", argv[0]);
    return 64;
}
