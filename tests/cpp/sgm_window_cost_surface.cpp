// The matching cost through include/sgm_amd/SGM.h: HipSolver::set_cost, cost and
// window_cost_device.
//   sgm_window_cost_surface bad -> the refusals throw; a constant pair then runs
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
    if (argc >= 2 && std::string(argv[1]) == "bad") {
        const int h = 24, w = 80, d = 32;
        sgm_amd::SGM sgm(h, w, 1, d);
        sgm_amd::BM bm(h, w, 1, d);
        uint8_t *img = nullptr;
        float *vol = nullptr, *out = nullptr;
        if (hipMalloc((void **)&img, 2 * h * w) != hipSuccess ||
            hipMalloc((void **)&vol, sizeof(float) * h * w * d) != hipSuccess ||
            hipMalloc((void **)&out, sizeof(float) * h * w) != hipSuccess)
            return 2;
        // left all 9, right all 5: every SAD cost is 4, every SSD cost 16
        if (hipMemset(img, 9, h * w) != hipSuccess || hipMemset(img + h * w, 5, h * w) != hipSuccess) return 2;
        const uint8_t *l = img, *r = img + h * w;
        bool ok = sgm.cost() == SGM_COST_CENSUS;
        ok = refused("a bad kind", [&] { sgm.set_cost(3); }) && ok;
        ok = refused("a BM handle", [&] { bm.set_cost(SGM_COST_SAD); }) && ok;
        ok = refused("the census as a window cost", [&] { sgm.window_cost_device(SGM_COST_CENSUS, l, r, w, vol); }) && ok;
        ok = refused("a NULL image", [&] { sgm.window_cost_device(SGM_COST_SAD, nullptr, r, w, vol); }) && ok;
        ok = refused("a small pitch", [&] { sgm.window_cost_device(SGM_COST_SAD, l, r, w - 1, vol); }) && ok;
        ok = refused("a NULL destination", [&] { sgm.window_cost_device(SGM_COST_SAD, l, r, w, nullptr); }) && ok;
        ok = refused("the legacy stream",
                     [&] { sgm.window_cost_device(SGM_COST_SSD, l, r, w, vol, hipStreamLegacy); }) && ok;
        std::vector<float> c((size_t)h * w * d), map((size_t)h * w, -1.0f);
        const int kinds[2] = {SGM_COST_SAD, SGM_COST_SSD};
        for (int k = 0; k < 2; ++k) {
            sgm.window_cost_device(kinds[k], l, r, w, vol);
            if (hipDeviceSynchronize() != hipSuccess ||
                hipMemcpy(c.data(), vol, c.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                return 2;
            for (float x : c) ok = ok && x == (k ? 16.0f : 4.0f);
            std::printf("constant pair: cost[0] = %g\n", c[0]);
        }
        // the volume goes straight into aggregate_device, and a frame on the same cost runs
        const sgm_volume hwd = {vol, SGM_VOL_F32, (long long)w * d, d, 1};
        sgm.aggregate_device(hwd, out, w);
        sgm.set_cost(SGM_COST_SSD);
        ok = ok && sgm.cost() == SGM_COST_SSD;
        sgm_amd::Mat ml(h, w, CV_8UC1), mr(h, w, CV_8UC1);
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) {
                ml.at<uint8_t>(i, j) = 9;
                mr.at<uint8_t>(i, j) = 5;
            }
        sgm.process(ml, mr);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(map.data(), out, map.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return 2;
        for (float x : map) ok = ok && x >= 0.0f && x <= (float)(d + 1);
        const sgm_amd::Mat &disp = sgm.get_disp();
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) ok = ok && disp.at<float>(i, j) >= 0.0f && disp.at<float>(i, j) <= (float)(d + 1);
        sgm.set_cost(SGM_COST_CENSUS);
        ok = ok && sgm.cost() == SGM_COST_CENSUS;
        hipFree(img);
        hipFree(vol);
        hipFree(out);
        return ok ? 0 : 1;
    }
    std::fprintf(stderr, "usage: %s bad\n", argv[0]);
    return 64;
}
