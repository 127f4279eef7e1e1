// fill.cpp -- VOX::FillInterior back ends: the host flood (the reference of vp_fill_interior, include/vphip.h) and the marshalling of
// the GPU variants onto the C ABI.
//
// The host path is the plain definition: an explicit-stack search from every empty boundary voxel, one voxel and its six face
// neighbours at a time, over a visited bit grid.  It takes none of the GPU's shortcuts (no run fills, no sweeps, no rounds), so it
// checks them.
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace VOX::detail {

namespace {

template <typename Index>
void Flood(uint32_t* words, size_t n)
{
    const Index N = static_cast<Index>(n), N2 = N * N, N3 = N2 * N;
    std::vector<uint32_t> outside(static_cast<size_t>(N3 / 32), 0u);   // the exterior found so far (same layout as the grid)
    auto isSet = [&](const std::vector<uint32_t>& g, Index v) { return (g[v >> 5] >> (v & 31)) & 1u; };
    auto wall = [&](Index v) { return (words[v >> 5] >> (v & 31)) & 1u; };
    std::vector<Index> stack;
    auto visit = [&](Index v) {
        if (wall(v) || isSet(outside, v)) return;
        outside[v >> 5] |= 1u << (v & 31);
        stack.push_back(v);
    };
    for (Index z = 0; z < N; ++z)
        for (Index y = 0; y < N; ++y)
            for (Index x = 0; x < N; ++x)
                if (x == 0 || y == 0 || z == 0 || x == N - 1 || y == N - 1 || z == N - 1) visit(x + N * y + N2 * z);
    while (!stack.empty()) {
        const Index v = stack.back();
        stack.pop_back();
        const Index x = v % N, y = (v / N) % N, z = v / N2;
        if (x > 0) visit(v - 1);
        if (x < N - 1) visit(v + 1);
        if (y > 0) visit(v - N);
        if (y < N - 1) visit(v + N);
        if (z > 0) visit(v - N2);
        if (z < N - 1) visit(v + N2);
    }
    for (size_t i = 0; i < outside.size(); ++i) words[i] = ~outside[i];
}

}  // namespace

void FillHost(uint32_t* words, size_t n)
{
    PROFILING_SCOPE("SequentialFill");
    if (n <= 1024) Flood<uint32_t>(words, n);          // n^3 <= 2^30 voxel indices
    else Flood<uint64_t>(words, n);
}

void FillDevice(const char* label, uint32_t* words, size_t n, float vs, const float origin[3])
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The interior fill runs on one device (no -g > 1)\n");
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    vp_ctx* ctx = vplib::Context();
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_fill_interior_host(ctx, &f, words, words));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

}  // namespace VOX::detail
