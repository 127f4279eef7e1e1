// skeleton.cpp -- VOX::Skeletonize back ends: the host restatement of vp_skeleton (include/vphip.h) and the marshalling of the GPU
// variants onto the C ABI.
//
// The host path is the plain sequential form: the grid as a byte volume with one empty layer around it, per iteration the border voxels
// listed once by subfield, then subfield after subfield every listed voxel that is still set examined against the volume as it is and
// deleted at once if the plain (flood-fill) simple() of csrc/skeleton_simple.h allows it.  Two voxels of one subfield are never
// 26-neighbours, so deleting them one after the other equals deleting them together: the result equals the kernels' bit for bit.  Any
// side n is served (the GPU variants need n % 32 == 0, n <= 1024).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../csrc/skeleton_simple.h"
#include "debug_utils.h"
#include "profiling.h"
#include "vox/skeleton.h"
#include "vp_runtime.h"

namespace VOX::detail {

SkeletonStats SkeletonHost(bool parallel, const uint32_t* words, const uint32_t* anchor, size_t n, int mode, uint32_t maxIters, uint32_t* out)
{
    cpuAssert(mode == SKELETON_KERNEL || mode == SKELETON_CURVE, "Unknown skeleton mode\n");
    PROFILING_SCOPE(parallel ? "OpenMPSkeleton" : "SequentialSkeleton");
    const int64_t N = static_cast<int64_t>(n), P = N + 2, plane = P * P;
    std::vector<uint8_t> vol(static_cast<size_t>(plane * P), 0);   // bit 0: set, bit 1: anchor
    auto bit = [&](const uint32_t* w, int64_t x, int64_t y, int64_t z) {
        const size_t i = static_cast<size_t>(x + N * (y + N * z));
        return (w[i >> 5] >> (i & 31)) & 1u;
    };
    auto at = [&](int64_t x, int64_t y, int64_t z) { return (x + 1) + P * (y + 1) + plane * (z + 1); };
#pragma omp parallel for schedule(static) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x)
                vol[static_cast<size_t>(at(x, y, z))] = static_cast<uint8_t>(bit(words, x, y, z) | (anchor ? bit(anchor, x, y, z) << 1 : 0u));
    int64_t offset[27];
    for (int i = 0; i < 27; ++i) offset[i] = (i % 3 - 1) + P * ((i / 3) % 3 - 1) + plane * (i / 9 - 1);

    SkeletonStats st{0, 0, 0};
    std::vector<int64_t> border[8];
    while (maxIters == 0 || st.iterations < maxIters) {
        for (auto& b : border) b.clear();
        for (int64_t z = 0; z < N; ++z)
            for (int64_t y = 0; y < N; ++y) {
                const uint8_t* row = vol.data() + at(0, y, z);
                for (int64_t x = 0; x < N; ++x) {
                    if (row[x] != 1) continue;                     // unset, or an anchor
                    if ((row[x - 1] & row[x + 1] & row[x - P] & row[x + P] & row[x - plane] & row[x + plane] & 1) != 0) continue;
                    border[(x & 1) | ((y & 1) << 1) | ((z & 1) << 2)].push_back(at(x, y, z));
                }
            }
        uint64_t lost = 0;
        for (int s = 0; s < 8; ++s) {
            const std::vector<int64_t>& list = border[s];
            const int64_t count = static_cast<int64_t>(list.size());
#pragma omp parallel for schedule(static) reduction(+ : lost) if (parallel)
            for (int64_t k = 0; k < count; ++k) {
                uint8_t* c = vol.data() + list[static_cast<size_t>(k)];
                uint32_t m = 0;
                for (int i = 0; i < 27; ++i) m |= static_cast<uint32_t>(c[offset[i]] & 1) << i;
                if (vp::sk_deletable<false>(m, mode)) {
                    *c = 0;
                    ++lost;
                }
            }
        }
        ++st.iterations;
        st.deleted += lost;
        if (lost == 0) break;
    }
    const size_t voxels = n * n * n;
    std::fill(out, out + (voxels + 31) / 32, 0u);
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x)
                if (vol[static_cast<size_t>(at(x, y, z))] & 1) {
                    const size_t i = static_cast<size_t>(x + N * (y + N * z));
                    out[i >> 5] |= 1u << (i & 31);
                    ++st.voxels;
                }
    return st;
}

SkeletonStats SkeletonDevice(int algo, const char* label, const uint32_t* words, const uint32_t* anchor, size_t n, float vs, const float origin[3],
                             int mode, uint32_t maxIters, uint32_t* out)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The skeleton runs on one device (no -g > 1)\n");
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    vp_ctx* ctx = vplib::Context();
    uint64_t stats[3] = {0, 0, 0};
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_skeleton_host(ctx, &f, words, anchor, mode, maxIters, algo, out, stats));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return SkeletonStats{stats[0], stats[1], stats[2]};
}

}  // namespace VOX::detail
