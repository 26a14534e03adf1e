// The cost filters on a finished volume through include/sgm_amd/SGM.h:
// HipSolver::set_volume_filter, volume_filter and filter_volume_device.
//   sgm_volume_filter_surface run <volume.f32> <map.f32> h w d
//     -> the refusals throw; the volume file (h x w x d floats) goes through
//        aggregate_device with both filters set, and through filter_volume_device
//        followed by an unfiltered aggregate_device; the map file takes both maps
#define SGM_AMD_THROW 1
#include "sgm_amd/SGM.h"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
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
    if (argc == 7 && std::string(argv[1]) == "run") {
        const int h = std::atoi(argv[4]), w = std::atoi(argv[5]), d = std::atoi(argv[6]);
        const size_t nvol = (size_t)h * w * d, npx = (size_t)h * w;
        std::vector<float> host(nvol), a(npx), b(npx);
        FILE *f = std::fopen(argv[2], "rb");
        if (!f || std::fread(host.data(), sizeof(float), nvol, f) != nvol) return 2;
        std::fclose(f);
        sgm_amd::SGM sgm(h, w, 1, d);
        float *cost = nullptr, *out = nullptr;
        if (hipMalloc((void **)&cost, sizeof(float) * nvol) != hipSuccess ||
            hipMalloc((void **)&out, sizeof(float) * npx) != hipSuccess ||
            hipMemcpy(cost, host.data(), nvol * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return 2;
        const sgm_volume vol = {cost, SGM_VOL_F32, (long long)w * d, d, 1};
        bool ok = sgm.volume_filter() == 0;
        ok = refused("unknown bits", [&] { sgm.set_volume_filter(4); }) && ok;
        ok = refused("no bits", [&] { sgm.filter_volume_device(cost, 0); }) && ok;
        ok = refused("a NULL volume", [&] { sgm.filter_volume_device(nullptr); }) && ok;
        ok = refused("the legacy stream", [&] { sgm.filter_volume_device(cost, SGM_FILTER_H, hipStreamLegacy); }) && ok;
        ok = ok && sgm.volume_filter() == 0;
        sgm.set_volume_filter(SGM_FILTER_H | SGM_FILTER_V);
        ok = ok && sgm.volume_filter() == (SGM_FILTER_H | SGM_FILTER_V);
        sgm.aggregate_device(vol, out, w);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(a.data(), out, npx * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return 2;
        sgm.set_volume_filter(0);
        sgm.filter_volume_device(cost);
        sgm.aggregate_device(vol, out, w);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(b.data(), out, npx * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return 2;
        f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(a.data(), sizeof(float), npx, f) != npx ||
            std::fwrite(b.data(), sizeof(float), npx, f) != npx)
            return 2;
        std::fclose(f);
        hipFree(cost);
        hipFree(out);
        return ok ? 0 : 1;
    }
    std::fprintf(stderr, "usage: %s run <volume.f32> <map.f32> h w d\n", argv[0]);
    return 64;
}
