// reconstruct.cpp -- VOX::Reconstruct / VOX::Extrema back ends: the host restatement of vp_reconstruct and vp_extrema (include/vphip.h)
// and the marshalling of the GPU variants onto the C ABI.
//
// The host path works on the work values (v for dilation, ~v for erosion, 0 off the domain) of a volume padded by one layer of zeros, so no
// step tests a bound.  Reconstruction is a widest-path search with a priority queue: the voxels are taken from the largest value down; a
// voxel taken with the value it still holds is final, and it offers min(its value, g(q)) to its neighbours q.  An entry whose voxel has
// been raised since it was pushed is skipped.  The extended extrema are found from the definition, not from a second reconstruction: every
// plateau of the flattened field is flooded once, and it is an extremum iff no voxel of it has a larger neighbour.  The fixed point is
// unique: the bytes equal the kernels'.  Any side n is served (the GPU variants need n % 32 == 0, n <= 1024).
#include <algorithm>
#include <cstdint>
#include <queue>
#include <string>
#include <utility>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/reconstruct.h"
#include "vp_runtime.h"

namespace VOX {

uint32_t Sqrt16(uint32_t v)
{
    const uint64_t x = static_cast<uint64_t>(v) << 8;
    uint64_t lo = 0, hi = 1u << 20;                                // lo^2 <= x < hi^2
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (mid * mid <= x) lo = mid; else hi = mid;
    }
    return static_cast<uint32_t>(lo);
}

namespace detail {

namespace {

struct Padded {
    int64_t N, P, plane;
    int64_t offset[26];
    int steps = 0;
    Padded(size_t n, int connectivity) : N(static_cast<int64_t>(n)), P(N + 2), plane(P * P)
    {
        cpuAssert(connectivity == 6 || connectivity == 26, "Unknown connectivity (6 or 26)\n");
        for (int i = 0; i < 27; ++i) {
            const int dx = i % 3 - 1, dy = (i / 3) % 3 - 1, dz = i / 9 - 1, k = (dx != 0) + (dy != 0) + (dz != 0);
            if (k == 0 || (k > 1 && connectivity == 6)) continue;
            offset[steps++] = dx + P * dy + plane * dz;
        }
    }
    size_t size() const { return static_cast<size_t>(plane * P); }
    int64_t at(int64_t x, int64_t y, int64_t z) const { return (x + 1) + P * (y + 1) + plane * (z + 1); }
    template <typename F> void each(bool parallel, F f) const
    {
#pragma omp parallel for schedule(static) if (parallel)
        for (int64_t z = 0; z < N; ++z)
            for (int64_t y = 0; y < N; ++y)
                for (int64_t x = 0; x < N; ++x) f(static_cast<size_t>(x + N * (y + N * z)), static_cast<size_t>(at(x, y, z)));
    }
};

bool inside(const uint32_t* domain, size_t i) { return !domain || ((domain[i >> 5] >> (i & 31)) & 1u); }

// r (padded, work values: R0 on entry) is raised to the reconstruction under g (padded, work values)
void widest_paths(const Padded& pd, const std::vector<uint32_t>& g, std::vector<uint32_t>& r)
{
    std::priority_queue<std::pair<uint32_t, int64_t>> heap;
    for (size_t p = 0; p < r.size(); ++p)
        if (r[p]) heap.emplace(r[p], static_cast<int64_t>(p));
    while (!heap.empty()) {
        const auto [value, p] = heap.top();
        heap.pop();
        if (r[static_cast<size_t>(p)] != value) continue;          // raised after it was pushed
        for (int k = 0; k < pd.steps; ++k) {
            const size_t q = static_cast<size_t>(p + pd.offset[k]);
            const uint32_t c = std::min(value, g[q]);
            if (c > r[q]) {
                r[q] = c;
                heap.emplace(c, static_cast<int64_t>(q));
            }
        }
    }
}

// field = the real values of r; the statistics against r0 (both padded, work values)
ReconstructStats finish(const Padded& pd, bool parallel, const uint32_t* domain, uint32_t flip, const std::vector<uint32_t>& r0,
                        const std::vector<uint32_t>& r, uint32_t* field)
{
    uint64_t count = 0, changed = 0, sum = 0;
    uint32_t top = 0;
    pd.each(false, [&](size_t i, size_t p) {
        field[i] = r[p] ^ flip;
        if (!inside(domain, i)) return;
        ++count;
        changed += r[p] != r0[p];
        sum += field[i];
        top = std::max(top, r[p]);
    });
    (void)parallel;
    return ReconstructStats{count, changed, sum, count ? static_cast<uint64_t>(top ^ flip) : 0};
}

ReconstructStats reconstruct(bool parallel, const uint32_t* domain, const uint32_t* marker, const uint32_t* mask, size_t n, int mode, int connectivity,
                             uint32_t* field)
{
    cpuAssert(mode == RECONSTRUCT_DILATION || mode == RECONSTRUCT_EROSION, "Unknown reconstruction mode\n");
    const Padded pd(n, connectivity);
    const uint32_t flip = mode == RECONSTRUCT_EROSION ? 0xFFFFFFFFu : 0u;
    std::vector<uint32_t> g(pd.size(), 0u), r0(pd.size(), 0u);
    pd.each(parallel, [&](size_t i, size_t p) {
        if (!inside(domain, i)) return;
        g[p] = mask[i] ^ flip;
        r0[p] = std::min(marker[i] ^ flip, g[p]);
    });
    std::vector<uint32_t> r(r0);
    widest_paths(pd, g, r);
    return finish(pd, parallel, domain, flip, r0, r, field);
}

uint32_t shift(uint32_t v, uint32_t h, bool up) { return up ? (v > 0xFFFFFFFFu - h ? 0xFFFFFFFFu : v + h) : (v < h ? 0u : v - h); }

}  // namespace

ReconstructStats ReconstructHost(bool parallel, const uint32_t* domain, const uint32_t* marker, const uint32_t* mask, size_t n, int mode,
                                 int connectivity, uint32_t* field)
{
    PROFILING_SCOPE(parallel ? "OpenMPReconstruct" : "SequentialReconstruct");
    return reconstruct(parallel, domain, marker, mask, n, mode, connectivity, field);
}

ExtremaStats ExtremaHost(bool parallel, const uint32_t* domain, const uint32_t* values, size_t n, int kind, int scale, uint32_t h, int connectivity,
                         uint32_t* scaled, uint32_t* flat, uint32_t* extrema)
{
    cpuAssert(kind == EXTREMA_MAXIMA || kind == EXTREMA_MINIMA, "Unknown extrema kind\n");
    cpuAssert(scale == EXTREMA_LINEAR || scale == EXTREMA_SQRT16, "Unknown extrema scale\n");
    PROFILING_SCOPE(parallel ? "OpenMPExtrema" : "SequentialExtrema");
    const bool minima = kind == EXTREMA_MINIMA;
    const size_t voxels = n * n * n;
    std::vector<uint32_t> marker(voxels);
#pragma omp parallel for schedule(static) if (parallel)
    for (int64_t i = 0; i < static_cast<int64_t>(voxels); ++i) {
        scaled[i] = scale == EXTREMA_SQRT16 ? Sqrt16(values[i]) : values[i];
        marker[static_cast<size_t>(i)] = shift(scaled[i], h, minima);
    }
    const ReconstructStats rs = reconstruct(parallel, domain, marker.data(), scaled, n, minima ? RECONSTRUCT_EROSION : RECONSTRUCT_DILATION,
                                            connectivity, flat);
    // the plateaus of the work values of H: flooded once each, an extremum iff nothing next to it is larger
    const Padded pd(n, connectivity);
    const uint32_t flip = minima ? 0xFFFFFFFFu : 0u;
    std::vector<uint32_t> w(pd.size(), 0u);
    std::vector<uint8_t> seen(pd.size(), 0);
    uint64_t flattened = 0;
    pd.each(false, [&](size_t i, size_t p) {
        if (!inside(domain, i)) return;
        w[p] = flat[i] ^ flip;
        flattened += flat[i] != scaled[i];
    });
    std::fill(extrema, extrema + (voxels + 31) / 32, 0u);
    std::vector<int64_t> plateau;
    uint64_t count = 0;
    const int64_t N = static_cast<int64_t>(n);
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x) {
                const int64_t start = pd.at(x, y, z);
                const uint32_t value = w[static_cast<size_t>(start)];
                if (value == 0 || seen[static_cast<size_t>(start)]) continue;
                plateau.assign(1, start);
                seen[static_cast<size_t>(start)] = 1;
                bool top = true;
                for (size_t k = 0; k < plateau.size(); ++k)
                    for (int s = 0; s < pd.steps; ++s) {
                        const size_t q = static_cast<size_t>(plateau[k] + pd.offset[s]);
                        if (w[q] > value) top = false;
                        if (w[q] == value && !seen[q]) { seen[q] = 1; plateau.push_back(static_cast<int64_t>(q)); }
                    }
                if (!top) continue;
                count += plateau.size();
                for (const int64_t p : plateau) {
                    const int64_t px = p % pd.P - 1, py = (p / pd.P) % pd.P - 1, pz = p / pd.plane - 1;
                    const size_t i = static_cast<size_t>(px + N * (py + N * pz));
                    extrema[i >> 5] |= 1u << (i & 31);
                }
            }
    return ExtremaStats{rs.domain, count, rs.top, flattened};
}

static vp_frame frame_of(size_t n, float vs, const float origin[3])
{
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    return f;
}

ReconstructStats ReconstructDevice(int algo, const char* label, const uint32_t* domain, const uint32_t* marker, const uint32_t* mask, size_t n,
                                   float vs, const float origin[3], int mode, int connectivity, uint32_t* field)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The reconstruction runs on one device (no -g > 1)\n");
    const vp_frame f = frame_of(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
    uint64_t stats[4] = {0, 0, 0, 0};
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_reconstruct_host(ctx, &f, domain, marker, mask, mode, connectivity, algo, field, stats));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return ReconstructStats{stats[0], stats[1], stats[2], stats[3]};
}

ExtremaStats ExtremaDevice(int algo, const char* label, const uint32_t* domain, const uint32_t* values, size_t n, float vs, const float origin[3],
                           int kind, int scale, uint32_t h, int connectivity, uint32_t* scaled, uint32_t* flat, uint32_t* extrema)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The extrema run on one device (no -g > 1)\n");
    const vp_frame f = frame_of(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
    uint64_t stats[4] = {0, 0, 0, 0};
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_extrema_host(ctx, &f, domain, values, kind, scale, h, connectivity, algo, scaled, flat, extrema, stats));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return ExtremaStats{stats[0], stats[1], stats[2], stats[3]};
}

}  // namespace detail

}  // namespace VOX
