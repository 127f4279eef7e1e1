// watershed.cpp -- VOX::Watershed back ends: the host restatement of vp_watershed (include/vphip.h) and the marshalling of the GPU variants
// onto the C ABI.
//
// The host path is a hierarchical queue: one FIFO per level rank (the level counted in flood order).  A voxel that gets its label enters,
// once per unlabelled neighbour w whose level is still to come, the FIFO of w's level: there it waits as a SOURCE.  A level pops its FIFO
// and grows breadth-first layers from it; every voxel holds the explicit key [arrival time : 30 | rank of the source : 14 | label : 20]
// of include/vphip.h, and a voxel reached twice inside one layer (equal arrival time) keeps the smaller key.  Layer by layer the keys
// are final, so nothing is ever re-queued.  A level needs no other sources than those in its FIFO: when a level ends, every voxel of its
// set A next to a labelled voxel has been labelled, so a voxel still unlabelled next to a labelled one has a later level -- and the
// labelled one waits in that level's FIFO.  The volume is padded by one layer of voxels outside the mask, so no step tests a bound.  Any
// side n is served (the GPU variants need n % 32 == 0, n <= 1024).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/watershed.h"
#include "vp_runtime.h"

namespace VOX::detail {

WatershedStats WatershedHost(bool parallel, const uint32_t* mask, const uint32_t* markers, const uint32_t* priority, size_t n, int order,
                             uint32_t quantum, int connectivity, uint32_t* labels, uint32_t* cut)
{
    cpuAssert(connectivity == 6 || connectivity == 26, "Unknown watershed connectivity\n");
    cpuAssert(!priority || order == WATERSHED_ASCENDING || order == WATERSHED_DESCENDING, "Unknown watershed order\n");
    cpuAssert(!priority || quantum >= 1, "The watershed quantum must be at least 1\n");
    PROFILING_SCOPE(parallel ? "OpenMPWatershed" : "SequentialWatershed");
    constexpr uint16_t kOut = 0xFFFF;                              // rank of a voxel outside the mask: its level never comes
    constexpr uint64_t kHop = 1ull << 34, kLabel = WATERSHED_LABEL_MAX;
    const int64_t N = static_cast<int64_t>(n), P = N + 2, plane = P * P;
    const uint32_t q = priority ? quantum : 1u;
    auto bit = [&](int64_t x, int64_t y, int64_t z) {
        const size_t i = static_cast<size_t>(x + N * (y + N * z));
        return (mask[i >> 5] >> (i & 31)) & 1u;
    };
    auto at = [&](int64_t x, int64_t y, int64_t z) { return (x + 1) + P * (y + 1) + plane * (z + 1); };

    // the levels: range, presence, refusals
    uint32_t lo = 0xFFFFFFFFu, hi = 0, top = 0;
    WatershedStats st{0, 0, 0, 0};
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x)
                if (bit(x, y, z)) {
                    const size_t i = static_cast<size_t>(x + N * (y + N * z));
                    const uint32_t level = (priority ? priority[i] : 0u) / q;
                    lo = std::min(lo, level); hi = std::max(hi, level); top = std::max(top, markers[i]);
                    st.markers += markers[i] != 0;
                }
    const bool empty = lo > hi;
    cpuAssert(top <= WATERSHED_LABEL_MAX, "A marker label lies above WATERSHED_LABEL_MAX\n");
    cpuAssert(empty || hi - lo < WATERSHED_MAX_SPAN, "The levels span WATERSHED_MAX_SPAN or more: use a larger quantum\n");
    const bool flip = priority && order == WATERSHED_DESCENDING;
    const uint32_t span = empty ? 0u : hi - lo + 1u;

    std::vector<uint16_t> rank(static_cast<size_t>(plane * P), kOut);
    std::vector<uint64_t> key(static_cast<size_t>(plane * P), 0);   // 0: no label
    std::vector<uint8_t> present(span, 0);
#pragma omp parallel for schedule(static) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x)
                if (bit(x, y, z)) {
                    const size_t i = static_cast<size_t>(x + N * (y + N * z));
                    const uint32_t level = (priority ? priority[i] : 0u) / q;
                    const uint32_t r = flip ? hi - level : level - lo;
                    rank[static_cast<size_t>(at(x, y, z))] = static_cast<uint16_t>(r);
                    key[static_cast<size_t>(at(x, y, z))] = markers[i];   // arrival time 0; the rank field of a source is read from rank[]
#pragma omp atomic write
                    present[r] = 1;
                }
    for (uint32_t r = 0; r < span; ++r) st.levels += present[r];

    int64_t offset[26];
    int steps = 0;
    for (int i = 0; i < 27; ++i) {
        const int dx = i % 3 - 1, dy = (i / 3) % 3 - 1, dz = i / 9 - 1, k = (dx != 0) + (dy != 0) + (dz != 0);
        if (k == 0 || (k > 1 && connectivity == 6)) continue;
        offset[steps++] = dx + P * dy + plane * dz;
    }

    // the FIFOs: a labelled voxel waits in the level of every unlabelled neighbour whose level is later than `now`
    std::vector<std::vector<int64_t>> fifo(span);
    auto enlist = [&](int64_t p, uint32_t now, bool all) {
        for (int k = 0; k < steps; ++k) {
            const size_t w = static_cast<size_t>(p + offset[k]);
            if (rank[w] != kOut && key[w] == 0 && (all || rank[w] > now)) fifo[rank[w]].push_back(p);
        }
    };
    if (st.markers)
        for (int64_t z = 0; z < N; ++z)
            for (int64_t y = 0; y < N; ++y)
                for (int64_t x = 0; x < N; ++x)
                    if (key[static_cast<size_t>(at(x, y, z))] != 0) enlist(at(x, y, z), 0, true);

    uint64_t base = 0;                                             // the largest arrival time so far
    std::vector<int64_t> layer, next;
    for (uint32_t h = 0; h < span && st.markers; ++h) {
        if (fifo[h].empty()) continue;
        layer.clear();
        layer.swap(fifo[h]);
        uint64_t t = base;                                         // arrival time of the voxels of `layer`
        bool sources = true;
        while (!layer.empty()) {
            next.clear();
            for (const int64_t p : layer) {
                const uint64_t mine = key[static_cast<size_t>(p)];
                const uint64_t carried = sources ? (static_cast<uint64_t>(rank[static_cast<size_t>(p)]) << 20) | (mine & kLabel) : mine & (kHop - 1);
                const uint64_t offer = ((t + 1) << 34) | carried;
                for (int k = 0; k < steps; ++k) {
                    const size_t w = static_cast<size_t>(p + offset[k]);
                    if (rank[w] > h) continue;                      // outside the mask, or its level is still to come
                    if (key[w] == 0) { key[w] = offer; next.push_back(static_cast<int64_t>(w)); }
                    else if ((key[w] >> 34) == t + 1 && offer < key[w]) key[w] = offer;   // reached in this layer already: the smaller key
                }
            }
            if (!sources)
                for (const int64_t p : layer) enlist(p, h, false);   // from the next level on it is a source
            if (!next.empty()) base = t + 1;
            layer.swap(next);
            sources = false;
            ++t;
        }
    }

    const size_t voxels = n * n * n;
    if (cut) std::fill(cut, cut + (voxels + 31) / 32, 0u);
    uint64_t labelled = 0, kept = 0;
#pragma omp parallel for schedule(static) reduction(+ : labelled) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x) {
                const uint32_t l = static_cast<uint32_t>(key[static_cast<size_t>(at(x, y, z))] & kLabel);
                labels[static_cast<size_t>(x + N * (y + N * z))] = l;
                labelled += l != 0;
            }
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x) {
                const int64_t p = at(x, y, z);
                const uint64_t l = key[static_cast<size_t>(p)] & kLabel;
                bool keep = l != 0;
                for (int k = 0; keep && k < steps; ++k) keep = (key[static_cast<size_t>(p + offset[k])] & kLabel) <= l;
                if (keep) {
                    ++kept;
                    const size_t i = static_cast<size_t>(x + N * (y + N * z));
                    if (cut) cut[i >> 5] |= 1u << (i & 31);
                }
            }
    st.labelled = labelled;
    st.cutVoxels = labelled - kept;
    return st;
}

WatershedStats WatershedDevice(int algo, const char* label, const uint32_t* mask, const uint32_t* markers, const uint32_t* priority, size_t n, float vs,
                               const float origin[3], int order, uint32_t quantum, int connectivity, uint32_t* labels, uint32_t* cut)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The watershed runs on one device (no -g > 1)\n");
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
        gpuAssert(vp_watershed_host(ctx, &f, mask, markers, priority, order, quantum, connectivity, algo, labels, cut, stats));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return WatershedStats{stats[0], stats[1], stats[2], stats[3]};
}

}  // namespace VOX::detail
