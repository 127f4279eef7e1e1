// geodesic.cpp -- VOX::GeodesicDistance back ends: the host restatement of vp_geodesic (include/vphip.h) and the marshalling of the GPU
// variants onto the C ABI.
//
// The host path is Dial's algorithm: the distances are small integers and a step costs at most 5, so a ring of 8 buckets holds every
// level that can be open at once.  The levels are settled in ascending order -- a listed voxel whose distance is no longer the level it
// was listed for has been lowered since and is skipped -- on a volume padded by one layer of voxels outside the mask, so no step tests a
// bound.  The add is min(d + w, 0xFFFFFFFE) as in every form.  The minimum over paths is unique: the bytes equal the kernels'.  Any side n
// is served (the GPU variants need n % 32 == 0, n <= 1024).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/geodesic.h"
#include "vp_runtime.h"

namespace VOX::detail {

GeodesicStats GeodesicHost(bool parallel, const uint32_t* mask, const uint32_t* seeds, size_t n, int metric, uint32_t* dist, uint32_t* reach)
{
    cpuAssert(metric == GEODESIC_6 || metric == GEODESIC_26 || metric == GEODESIC_CHAMFER, "Unknown geodesic metric\n");
    PROFILING_SCOPE(parallel ? "OpenMPGeodesic" : "SequentialGeodesic");
    constexpr uint32_t kNone = GEODESIC_NONE, kMax = 0xFFFFFFFEu, kRing = 8;
    const int64_t N = static_cast<int64_t>(n), P = N + 2, plane = P * P;
    const uint32_t weight[3][3] = {{1, 0, 0}, {1, 1, 1}, {3, 4, 5}};
    std::vector<uint8_t> in(static_cast<size_t>(plane * P), 0);    // bit 0: in the mask, bit 1: a seed
    std::vector<uint32_t> d(static_cast<size_t>(plane * P), kNone);
    auto bit = [&](const uint32_t* w, int64_t x, int64_t y, int64_t z) {
        const size_t i = static_cast<size_t>(x + N * (y + N * z));
        return (w[i >> 5] >> (i & 31)) & 1u;
    };
    auto at = [&](int64_t x, int64_t y, int64_t z) { return (x + 1) + P * (y + 1) + plane * (z + 1); };
#pragma omp parallel for schedule(static) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x)
                in[static_cast<size_t>(at(x, y, z))] = static_cast<uint8_t>(bit(mask, x, y, z) | (bit(seeds, x, y, z) << 1));
    int64_t offset[26];
    uint32_t cost[26];
    int steps = 0;
    for (int i = 0; i < 27; ++i) {
        const int dx = i % 3 - 1, dy = (i / 3) % 3 - 1, dz = i / 9 - 1, k = (dx != 0) + (dy != 0) + (dz != 0);
        if (k == 0 || weight[metric][k - 1] == 0) continue;
        offset[steps] = dx + P * dy + plane * dz;
        cost[steps++] = weight[metric][k - 1];
    }

    GeodesicStats st{0, 0, 0, 0};
    std::vector<int64_t> ring[kRing];
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x)
                if (in[static_cast<size_t>(at(x, y, z))] == 3) {
                    d[static_cast<size_t>(at(x, y, z))] = 0;
                    ring[0].push_back(at(x, y, z));
                    ++st.seeds;
                }
    size_t open = ring[0].size();                                  // entries in the ring
    std::vector<int64_t> cur;
    for (uint64_t level = 0; open != 0; ++level) {
        cur.clear();
        cur.swap(ring[level % kRing]);
        open -= cur.size();
        for (const int64_t p : cur) {
            if (d[static_cast<size_t>(p)] != level) continue;       // lowered after it was listed
            for (int k = 0; k < steps; ++k) {
                const size_t q = static_cast<size_t>(p + offset[k]);
                const uint32_t t = static_cast<uint32_t>(std::min<uint64_t>(level + cost[k], kMax));
                if ((in[q] & 1) && d[q] > t) {
                    d[q] = t;
                    ring[t % kRing].push_back(static_cast<int64_t>(q));
                    ++open;
                }
            }
        }
    }

    const size_t voxels = n * n * n;
    if (reach) std::fill(reach, reach + (voxels + 31) / 32, 0u);
    uint64_t reached = 0;
#pragma omp parallel for schedule(static) reduction(+ : reached) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x) {
                const uint32_t v = d[static_cast<size_t>(at(x, y, z))];
                dist[static_cast<size_t>(x + N * (y + N * z))] = v;
                reached += v != kNone;
            }
    st.reached = reached;
    for (size_t i = 0; i < voxels; ++i) {                          // ascending: the first voxel that attains the maximum keeps it
        if (dist[i] == kNone) continue;
        if (reach) reach[i >> 5] |= 1u << (i & 31);
        if (dist[i] > st.maxDist) { st.maxDist = dist[i]; st.maxIndex = i; }
    }
    if (st.reached && st.maxDist == 0) {                            // every reached voxel is a seed: the lowest of them
        for (size_t i = 0; i < voxels; ++i)
            if (dist[i] == 0) { st.maxIndex = i; break; }
    }
    return st;
}

GeodesicStats GeodesicDevice(int algo, const char* label, const uint32_t* mask, const uint32_t* seeds, size_t n, float vs, const float origin[3],
                             int metric, uint32_t* dist, uint32_t* reach)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The geodesic distance runs on one device (no -g > 1)\n");
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    vp_ctx* ctx = vplib::Context();
    uint64_t stats[4] = {0, 0, 0, 0};
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_geodesic_host(ctx, &f, mask, seeds, metric, algo, dist, reach, stats));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return GeodesicStats{stats[0], stats[1], stats[2], stats[3]};
}

}  // namespace VOX::detail
