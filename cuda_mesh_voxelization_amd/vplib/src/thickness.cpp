// thickness.cpp -- VOX::LocalThickness back ends: the host restatement of vp_thickness (include/vphip.h) and the marshalling of the GPU
// variants onto the C ABI.
//
// The host path is the definition by loops: D(c) = min(E(c), W(c), rmax^2) from the host distance transform, then for every target plane z
// the centres of the planes z - r .. z + r paint the disc their ball cuts out of it, T2 = the maximum of what reaches a voxel.  A plane is
// written by one thread only (OPENMP: planes in parallel).  Integer arithmetic: the result equals the kernels' bit for bit.  Any side n is
// served (the GPU variants need n % 32 == 0, n <= 1024).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace VOX::detail {

uint64_t ThicknessHost(bool parallel, const uint32_t* words, size_t n, uint32_t rmax, uint32_t thin2, uint32_t* t2, uint32_t* thin)
{
    cpuAssert(rmax >= 1 && rmax <= 32, "Thickness band outside 1..32\n");
    cpuAssert(thin2 <= rmax * rmax, "Thin threshold above the squared band\n");
    const int N = static_cast<int>(n);
    const size_t plane = n * n, voxels = plane * n;
    std::vector<uint32_t> dist(voxels);
    EdtHost(parallel, words, n, VP_EDT_SEEDS_UNSET, dist.data());
    PROFILING_SCOPE(parallel ? "OpenMPThickness" : "SequentialThickness");
    const uint32_t rmax2 = rmax * rmax;
    std::vector<uint16_t> D(voxels);
    uint32_t top = 0;
#pragma omp parallel for schedule(static) reduction(max : top) if (parallel)
    for (int z = 0; z < N; ++z)
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                const size_t i = static_cast<size_t>(x) + n * (static_cast<size_t>(y) + n * static_cast<size_t>(z));
                uint32_t d = 0;
                if (dist[i] != 0) {                                // a set voxel (an unset one is its own seed)
                    const uint32_t m = 1u + static_cast<uint32_t>(std::min({x, N - 1 - x, y, N - 1 - y, z, N - 1 - z}));
                    d = std::min({dist[i], m * m, rmax2});
                }
                D[i] = static_cast<uint16_t>(d);
                top = std::max(top, d);
            }
    int r = 0;                                                     // the largest r with r^2 < the largest D
    while (static_cast<uint32_t>((r + 1) * (r + 1)) < top) ++r;
    std::fill(t2, t2 + voxels, 0u);
#pragma omp parallel for schedule(dynamic) if (parallel)
    for (int z = 0; z < N; ++z) {
        uint32_t* out = t2 + static_cast<size_t>(z) * plane;
        for (int cz = std::max(0, z - r); cz <= std::min(N - 1, z + r); ++cz) {
            const uint32_t qz = static_cast<uint32_t>((z - cz) * (z - cz));
            const uint16_t* Dp = D.data() + static_cast<size_t>(cz) * plane;
            for (int cy = 0; cy < N; ++cy)
                for (int cx = 0; cx < N; ++cx) {
                    const uint32_t d = Dp[static_cast<size_t>(cy) * n + cx];
                    if (d <= qz) continue;
                    // every p with |p - c|^2 < d lies in the grid: d <= W(c)
                    int s = 0;
                    while (static_cast<uint32_t>((s + 1) * (s + 1)) + qz < d) ++s;
                    for (int dy = -s; dy <= s; ++dy) {
                        const uint32_t qzy = qz + static_cast<uint32_t>(dy * dy);
                        uint32_t* row = out + static_cast<size_t>(cy + dy) * n + cx;
                        for (int dx = -s; dx <= s; ++dx)
                            if (qzy + static_cast<uint32_t>(dx * dx) < d && row[dx] < d) row[dx] = d;
                    }
                }
        }
    }
    uint64_t count = 0;
    const size_t nwords = (voxels + 31) / 32;
    if (thin) std::fill(thin, thin + nwords, 0u);
    for (size_t i = 0; i < voxels; ++i)
        if (t2[i] != 0 && t2[i] < thin2) {
            ++count;
            if (thin) thin[i >> 5] |= 1u << (i & 31);
        }
    return count;
}

uint64_t ThicknessDevice(int algo, const char* label, const uint32_t* words, size_t n, float vs, const float origin[3], uint32_t rmax,
                         uint32_t thin2, uint32_t* t2, uint32_t* thin)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The local thickness runs on one device (no -g > 1)\n");
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    vp_ctx* ctx = vplib::Context();
    uint64_t count = 0;
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_thickness_host(ctx, &f, words, rmax, thin2, algo, t2, thin, &count));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return count;
}

}  // namespace VOX::detail
