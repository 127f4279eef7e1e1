// regions.cpp -- VOX::AnalyzeRegions back ends: the host restatement of vp_regions (include/vphip.h) and the marshalling of the GPU variants
// onto the C ABI.
//
// The host path is one pass over the effective labels on a volume padded by one layer of zeros, so no step tests a bound.  A row is walked
// along x; the voxels of a run -- consecutive voxels of one label -- are added up in a local record in grid coordinates, and the record is
// merged into the table when the label changes.  A voxel counts a lattice point (edge) of its label iff none of the other seven (three)
// voxels incident on it carries the same label at a lower index: the incident voxel of the label with the lowest index is the one that
// counts it, so every point (edge) with a voxel of the label on it is counted once.  Sums add, minima and maxima combine: the order in which
// runs are merged does not show, which is what lets OPENMP deal the planes to threads.  Any side n is served (the GPU variants need
// n % 32 == 0, n <= 1024).
#include <omp.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/regions.h"
#include "vp_runtime.h"

namespace VOX::detail {

namespace {

constexpr uint64_t kNone = ~0ull;
constexpr bool kIsMin[REGION_WORDS] = {false, true, true, true, false, false, false, false, false, false, false, false, false,
                                       false, false, false, false, false, false, false, false, false, false, true, false, true};
constexpr bool kIsMax[REGION_WORDS] = {false, false, false, false, true, true, true, false, false, false, false, false, false,
                                       false, false, false, false, false, false, false, false, false, false, false, true, false};

void Clear(RegionStats& r)
{
    for (uint32_t j = 0; j < REGION_WORDS; ++j) r.w[j] = kIsMin[j] ? kNone : 0;
}

void Merge(RegionStats& into, const RegionStats& r)
{
    for (uint32_t j = 0; j < REGION_WORDS; ++j)
        into.w[j] = kIsMin[j] ? std::min(into.w[j], r.w[j]) : kIsMax[j] ? std::max(into.w[j], r.w[j]) : into.w[j] + r.w[j];
}

}  // namespace

RegionTotals RegionsHost(bool parallel, const uint32_t* labels, uint32_t count, const uint32_t* values, size_t n, RegionStats* table)
{
    cpuAssert(count <= REGIONS_MAX, "More labels than REGIONS_MAX: filter the small components out first\n");
    PROFILING_SCOPE(parallel ? "OpenMPRegions" : "SequentialRegions");
    const int64_t N = static_cast<int64_t>(n), P = N + 2, plane = P * P;
    std::vector<uint32_t> L(static_cast<size_t>(plane * P), 0u);
    uint64_t ignored = 0;
#pragma omp parallel for schedule(static) reduction(+ : ignored) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x) {
                const uint32_t l = labels[static_cast<size_t>(x + N * (y + N * z))];
                ignored += l > count;
                L[static_cast<size_t>((x + 1) + P * (y + 1) + plane * (z + 1))] = l <= count ? l : 0u;
            }
    for (uint32_t k = 0; k < count; ++k) Clear(table[k]);

    // the voxels incident on the eight corners (seven others each) and the twelve edges (three others each) of a voxel, as index offsets
    int64_t corner[8][7], edge[12][3];
    for (int c = 0; c < 8; ++c) {
        int m = 0;
        for (int a = 0; a < 8; ++a) {
            const int dx = (c & 1) - 1 + (a & 1), dy = ((c >> 1) & 1) - 1 + ((a >> 1) & 1), dz = ((c >> 2) & 1) - 1 + ((a >> 2) & 1);
            if (dx || dy || dz) corner[c][m++] = dx + P * dy + plane * dz;
        }
    }
    for (int e = 0; e < 12; ++e) {
        int m = 0;
        for (int a = 0; a < 4; ++a) {
            const int d1 = (e & 1) - 1 + (a & 1), d2 = ((e >> 1) & 1) - 1 + ((a >> 1) & 1), axis = e >> 2;
            const int dx = axis == 0 ? 0 : d1, dy = axis == 0 ? d1 : axis == 1 ? 0 : d2, dz = axis == 2 ? 0 : d2;
            if (dx || dy || dz) edge[e][m++] = dx + P * dy + plane * dz;
        }
    }
    const int64_t face[3][2] = {{-1, 1}, {-P, P}, {-plane, plane}};

    constexpr int kLocks = 64;
    omp_lock_t locks[kLocks];
    for (omp_lock_t& l : locks) omp_init_lock(&l);
#pragma omp parallel for schedule(static) if (parallel)
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y) {
            RegionStats run;
            uint32_t cur = 0;
            auto flush = [&] {
                if (cur == 0) return;
                omp_lock_t* lock = &locks[cur % kLocks];
                omp_set_lock(lock);
                Merge(table[cur - 1], run);
                omp_unset_lock(lock);
            };
            for (int64_t x = 0; x < N; ++x) {
                const int64_t p = (x + 1) + P * (y + 1) + plane * (z + 1);
                const uint32_t k = L[static_cast<size_t>(p)];
                if (k != cur) {
                    flush();
                    cur = k;
                    Clear(run);
                }
                if (k == 0) continue;
                const uint64_t X = static_cast<uint64_t>(x), Y = static_cast<uint64_t>(y), Z = static_cast<uint64_t>(z);
                const uint64_t index = X + n * (Y + n * Z);
                uint64_t* w = run.w;
                w[0] += 1;
                w[1] = std::min(w[1], X); w[2] = std::min(w[2], Y); w[3] = std::min(w[3], Z);
                w[4] = std::max(w[4], X); w[5] = std::max(w[5], Y); w[6] = std::max(w[6], Z);
                w[7] += X; w[8] += Y; w[9] += Z;
                w[10] += X * X; w[11] += Y * Y; w[12] += Z * Z; w[13] += X * Y; w[14] += X * Z; w[15] += Y * Z;
                for (int a = 0; a < 3; ++a)
                    for (int s = 0; s < 2; ++s) {
                        const uint32_t other = L[static_cast<size_t>(p + face[a][s])];
                        w[16 + a] += other != k;
                        w[19] += other != k && other != 0;
                    }
                for (int c = 0; c < 8; ++c) {
                    bool mine = true;
                    for (int m = 0; m < 7; ++m) mine = mine && !(corner[c][m] < 0 && L[static_cast<size_t>(p + corner[c][m])] == k);
                    w[20] += mine;
                }
                for (int e = 0; e < 12; ++e) {
                    bool mine = true;
                    for (int m = 0; m < 3; ++m) mine = mine && !(edge[e][m] < 0 && L[static_cast<size_t>(p + edge[e][m])] == k);
                    w[21] += mine;
                }
                if (values) {
                    const uint64_t v = values[index];
                    w[22] += v; w[23] = std::min(w[23], v); w[24] = std::max(w[24], v);
                }
                w[25] = std::min(w[25], index);
            }
            flush();
        }
    for (omp_lock_t& l : locks) omp_destroy_lock(&l);

    RegionTotals t{0, 0, ignored, 0};
    for (uint32_t k = 0; k < count; ++k) {
        RegionStats& r = table[k];
        if (r.w[0] == 0) std::fill(r.w, r.w + REGION_WORDS, 0ull);
        else if (!values) r.w[23] = 0;
        t.voxels += r.w[0];
        t.labels += r.w[0] != 0;
        t.interfaces += r.w[19];
    }
    t.interfaces /= 2;
    return t;
}

RegionTotals RegionsDevice(int algo, const char* label, const uint32_t* labels, uint32_t count, const uint32_t* values, size_t n, RegionStats* table)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The region analysis runs on one device (no -g > 1)\n");
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = 1.0f;           // the words are voxel indices: the frame's origin and voxel size do not enter
    f.z0 = 0; f.z1 = f.n;
    vp_ctx* ctx = vplib::Context();
    uint64_t stats[4] = {0, 0, 0, 0};
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_regions_host(ctx, &f, labels, count, values, algo, count ? reinterpret_cast<uint64_t*>(table) : nullptr, stats));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return RegionTotals{stats[0], stats[1], stats[2], stats[3]};
}

}  // namespace VOX::detail
