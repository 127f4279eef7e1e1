// components.cpp -- VOX::LabelComponents / VOX::FilterComponents back ends: the host restatement of vp_components_label and
// vp_components_filter (include/vphip.h) and the marshalling of the GPU variants onto the C ABI.
//
// The host path is a different formulation from the kernels (a union-find over x runs): one scan over the voxels in linear index order
// that starts an explicit-stack flood at every set voxel without a label yet and gives the whole flood the next label.  The scan meets
// each component first at its lowest voxel index, so the labels come out in the contract's order by construction, with no ranking step.
// Sizes are counted by the flood; the filter keeps the m largest (ties: the lower label) or those of at least v voxels.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace VOX::detail {

namespace {

// labels (n^3, zeroed here) and the sizes of the components in label order
std::vector<uint32_t> Flood(const uint32_t* words, size_t n, uint32_t* labels, int conn)
{
    const long N = static_cast<long>(n);
    const size_t voxels = n * n * n;
    std::fill_n(labels, voxels, 0u);
    auto isSet = [&](size_t v) { return (words[v >> 5] >> (v & 31)) & 1u; };
    std::vector<uint32_t> sizes;
    std::vector<size_t> stack;
    for (size_t seed = 0; seed < voxels; ++seed) {
        if (!isSet(seed) || labels[seed]) continue;
        const uint32_t label = static_cast<uint32_t>(sizes.size()) + 1u;
        uint32_t count = 0;
        labels[seed] = label;
        stack.push_back(seed);
        while (!stack.empty()) {
            const size_t v = stack.back();
            stack.pop_back();
            ++count;
            const long x = static_cast<long>(v % n), y = static_cast<long>((v / n) % n), z = static_cast<long>(v / (n * n));
            for (long dz = -1; dz <= 1; ++dz)
                for (long dy = -1; dy <= 1; ++dy)
                    for (long dx = -1; dx <= 1; ++dx) {
                        const int steps = (dx != 0) + (dy != 0) + (dz != 0);
                        if (steps == 0 || (conn == VP_CONN_6 && steps != 1)) continue;
                        const long xx = x + dx, yy = y + dy, zz = z + dz;
                        if (xx < 0 || xx >= N || yy < 0 || yy >= N || zz < 0 || zz >= N) continue;
                        const size_t u = static_cast<size_t>(xx) + n * (static_cast<size_t>(yy) + n * static_cast<size_t>(zz));
                        if (!isSet(u) || labels[u]) continue;
                        labels[u] = label;
                        stack.push_back(u);
                    }
        }
        sizes.push_back(count);
    }
    return sizes;
}

vp_frame WholeFrame(size_t n, float vs, const float origin[3])
{
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    return f;
}

void CheckArguments(int conn, int mode, uint32_t param)
{
    cpuAssert(conn == VP_CONN_6 || conn == VP_CONN_26, "Connectivity must be 6 or 26\n");
    cpuAssert(mode == VP_COMP_KEEP_LARGEST || mode == VP_COMP_MIN_VOXELS, "Unknown component filter mode\n");
    cpuAssert(mode != VP_COMP_KEEP_LARGEST || (param >= 1 && param <= 16), "KEEP_LARGEST keeps 1 .. 16 components\n");
}

}  // namespace

uint32_t LabelHost(bool parallel, const uint32_t* words, size_t n, uint32_t* labels, int conn)
{
    PROFILING_SCOPE(parallel ? "OpenMPComponents" : "SequentialComponents");
    CheckArguments(conn, VP_COMP_MIN_VOXELS, 0);
    return static_cast<uint32_t>(Flood(words, n, labels, conn).size());     // the flood is one sequential scan under both host types
}

ComponentStats FilterHost(bool parallel, uint32_t* words, size_t n, int mode, uint32_t param, int conn)
{
    PROFILING_SCOPE(parallel ? "OpenMPComponents" : "SequentialComponents");
    CheckArguments(conn, mode, param);
    const size_t voxels = n * n * n;
    std::vector<uint32_t> labels(voxels);
    const std::vector<uint32_t> sizes = Flood(words, n, labels.data(), conn);
    const size_t K = sizes.size();
    std::vector<uint8_t> keep(K + 1, 0);                                    // by label; 0 = background
    if (mode == VP_COMP_MIN_VOXELS) {
        for (size_t k = 0; k < K; ++k) keep[k + 1] = sizes[k] >= param;
    } else {
        std::vector<size_t> order(K);
        std::iota(order.begin(), order.end(), size_t{0});
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return sizes[a] > sizes[b]; });   // stable: ties keep label order
        for (size_t i = 0; i < std::min<size_t>(param, K); ++i) keep[order[i] + 1] = 1;
    }
    ComponentStats st{static_cast<uint32_t>(K), 0};
#pragma omp parallel for schedule(static) if (parallel)
    for (long long i = 0; i < static_cast<long long>((voxels + 31) / 32); ++i) {
        uint32_t wout = 0u;
        for (size_t b = 0; b < 32 && static_cast<size_t>(i) * 32 + b < voxels; ++b)
            if (keep[labels[static_cast<size_t>(i) * 32 + b]]) wout |= 1u << b;
        words[i] = wout;
    }
    for (size_t k = 0; k < K; ++k) if (keep[k + 1]) st.kept += sizes[k];
    return st;
}

uint32_t LabelDevice(int algo, const char* label, const uint32_t* words, size_t n, float vs, const float origin[3], uint32_t* labels, int conn)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The component labelling runs on one device (no -g > 1)\n");
    const vp_frame f = WholeFrame(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
    uint32_t count = 0;
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_components_label_host(ctx, &f, words, labels, conn, algo, &count));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return count;
}

ComponentStats FilterDevice(int algo, const char* label, uint32_t* words, size_t n, float vs, const float origin[3], int mode, uint32_t param,
                            int conn)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The component filter runs on one device (no -g > 1)\n");
    const vp_frame f = WholeFrame(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
    ComponentStats st{0, 0};
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_components_filter_host(ctx, &f, words, words, conn, mode, param, algo, &st.count, &st.kept));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
    return st;
}

}  // namespace VOX::detail
