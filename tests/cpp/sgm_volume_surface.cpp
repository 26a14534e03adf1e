// A caller's cost volume through include/sgm_amd/SGM.h: HipSolver::aggregate_device
// and import_volume_device.
//   sgm_volume_surface bad -> the refusals throw; a constant volume then runs
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
        float *cost = nullptr, *out = nullptr, *vol = nullptr;
        if (hipMalloc((void **)&cost, sizeof(float) * h * w * d) != hipSuccess ||
            hipMalloc((void **)&out, sizeof(float) * h * w) != hipSuccess ||
            hipMalloc((void **)&vol, sizeof(float) * h * w * d) != hipSuccess)
            return 2;
        std::vector<float> ones((size_t)h * w * d, 1.0f), map((size_t)h * w, -1.0f);
        if (hipMemcpy(cost, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 2;
        const sgm_volume hwd = {cost, SGM_VOL_F32, (long long)w * d, d, 1};
        const sgm_volume dhw = {cost, SGM_VOL_F32, w, 1, (long long)h * w};
        sgm_volume v = hwd;
        bool ok = true;
        v.d_cost = nullptr;
        ok = refused("a NULL volume", [&] { sgm.aggregate_device(v, out, w); }) && ok;
        ok = refused("a NULL map", [&] { sgm.aggregate_device(hwd, nullptr, w); }) && ok;
        ok = refused("a small pitch", [&] { sgm.aggregate_device(hwd, out, w - 1); }) && ok;
        v = hwd;
        v.dtype = 2;
        ok = refused("a bad dtype", [&] { sgm.aggregate_device(v, out, w); }) && ok;
        v = hwd;
        v.stride_col = 1;
        ok = refused("both strides 1", [&] { sgm.aggregate_device(v, out, w); }) && ok;
        v = dhw;
        v.stride_col = 2;
        ok = refused("neither stride 1", [&] { sgm.aggregate_device(v, out, w); }) && ok;
        v = hwd;
        v.stride_row -= 1;
        ok = refused("overlapping strides", [&] { sgm.import_volume_device(v, SGM_VIEW_LEFT, vol); }) && ok;
        v = dhw;
        v.stride_disp = -v.stride_disp;
        ok = refused("a negative stride", [&] { sgm.import_volume_device(v, SGM_VIEW_LEFT, vol); }) && ok;
        ok = refused("a bad view", [&] { sgm.import_volume_device(hwd, 2, vol); }) && ok;
        ok = refused("a NULL destination", [&] { sgm.import_volume_device(hwd, SGM_VIEW_RIGHT, nullptr); }) && ok;
        ok = refused("the legacy stream", [&] { sgm.aggregate_device(hwd, out, w, nullptr, hipStreamLegacy); }) && ok;
        // a constant volume runs through both calls: every pixel of the map is a disparity or d + 1
        sgm.import_volume_device(dhw, SGM_VIEW_RIGHT, vol);
        sgm.aggregate_device(dhw, out, w);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(map.data(), out, map.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return 2;
        for (float x : map) ok = ok && x >= 0.0f && x <= (float)(d + 1);
        std::printf("constant volume: map[0] = %g\n", map[0]);
        hipFree(cost);
        hipFree(out);
        hipFree(vol);
        return ok ? 0 : 1;
    }
    std::fprintf(stderr, "usage: %s bad\n", argv[0]);
    return 64;
}
