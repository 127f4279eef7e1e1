// edt.cpp -- VOX::DistanceTransform, VOX::MorphExact and JFA::ComputeExact back ends: the host restatement of vp_edt / vp_edt_morph /
// vp_edt_sdf (include/vphip.h) and the marshalling of the GPU variants onto the C ABI.
//
// The host path is a different formulation from the kernels (which search outwards from every voxel while d^2 is below the best so far):
//   x   two sweeps per row, carrying the position of the last seed seen from the left and from the right
//   y, z   the lower envelope of the parabolas g(j) + (i - j)^2 of a column (Meijster, Roerdink and Hesselink 2000), with the integer
//          separator Sep(i, u) = (u^2 - i^2 + g(u) - g(i)) div 2 (u - i); entries without a seed carry no parabola
// Everything is integer arithmetic in 64 bits, so the result equals the kernels' bit for bit.  Any side n is served (the GPU variants
// need n % 32 == 0, n <= 1024).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "jfa/jfa.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace {

constexpr uint32_t kNone = VP_EDT_NONE;

inline bool Bit(const uint32_t* w, size_t i) { return (w[i >> 5] >> (i & 31)) & 1u; }

// out[i] = min over j of g(j) + (i - j)^2 for the n entries g(j) = in[j * stride]; kNone where no entry has a seed
void Envelope(const uint32_t* in, uint32_t* out, size_t stride, int n, std::vector<int>& s, std::vector<int>& t, std::vector<int64_t>& g)
{
    for (int i = 0; i < n; ++i) g[i] = in[static_cast<size_t>(i) * stride];
    auto F = [&](int64_t x, int i) { return (x - i) * (x - i) + g[i]; };
    int q = -1;
    for (int u = 0; u < n; ++u) {
        if (g[u] == kNone) continue;
        while (q >= 0 && F(t[q], s[q]) > F(t[q], u)) --q;
        if (q < 0) { q = 0; s[0] = u; t[0] = 0; continue; }
        const int i = s[q];
        // s[q] is no worse than u at t[q] >= 0 and u > i, so the numerator is not negative
        const int64_t w = 1 + (static_cast<int64_t>(u) * u - static_cast<int64_t>(i) * i + g[u] - g[i]) / (2 * static_cast<int64_t>(u - i));
        if (w < n) { ++q; s[q] = u; t[q] = static_cast<int>(w); }
    }
    for (int u = n - 1; u >= 0; --u) {
        out[u] = q < 0 ? kNone : static_cast<uint32_t>(F(u, s[q]));
        if (q >= 0 && u == t[q]) --q;
    }
}

// seeds: bit i of `mask` XOR inv, voxels in linear order
void TransformHost(bool parallel, const uint32_t* mask, bool inv, size_t n, uint32_t* dist)
{
    const int N = static_cast<int>(n);
    const size_t plane = n * n;
#pragma omp parallel for schedule(static) if (parallel)
    for (int z = 0; z < N; ++z) {
        std::vector<int> s(n), t(n);
        std::vector<int64_t> g(n);
        std::vector<uint32_t> col(n);
        for (int y = 0; y < N; ++y) {
            const size_t row = static_cast<size_t>(z) * plane + static_cast<size_t>(y) * n;
            int last = -1;
            for (int x = 0; x < N; ++x) {
                if (Bit(mask, row + x) != inv) last = x;
                dist[row + x] = last < 0 ? kNone : static_cast<uint32_t>((x - last) * (x - last));
            }
            last = -1;
            for (int x = N - 1; x >= 0; --x) {
                if (Bit(mask, row + x) != inv) last = x;
                if (last >= 0) dist[row + x] = std::min(dist[row + x], static_cast<uint32_t>((last - x) * (last - x)));
            }
        }
        for (int x = 0; x < N; ++x) {
            uint32_t* c = dist + static_cast<size_t>(z) * plane + x;
            Envelope(c, col.data(), n, N, s, t, g);
            for (int y = 0; y < N; ++y) c[static_cast<size_t>(y) * n] = col[y];
        }
    }
#pragma omp parallel for schedule(static) if (parallel)
    for (int y = 0; y < N; ++y) {
        std::vector<int> s(n), t(n);
        std::vector<int64_t> g(n);
        std::vector<uint32_t> col(n);
        for (int x = 0; x < N; ++x) {
            uint32_t* c = dist + static_cast<size_t>(y) * n + x;
            Envelope(c, col.data(), plane, N, s, t, g);
            for (int z = 0; z < N; ++z) c[static_cast<size_t>(z) * plane] = col[z];
        }
    }
}

// the JFA's seeds (vplib/src/jfa.cpp, ::Initialization): set voxels with an unset 26-neighbour or one outside the grid
std::vector<uint32_t> BorderMask(bool parallel, const uint32_t* words, size_t n)
{
    const int N = static_cast<int>(n);
    std::vector<uint32_t> mask((n * n * n + 31) / 32, 0u);
    uint32_t* bits = mask.data();
    auto at = [&](int x, int y, int z) { return static_cast<size_t>(x) + (static_cast<size_t>(y) + static_cast<size_t>(z) * n) * n; };
#pragma omp parallel for schedule(static) if (parallel)
    for (int z = 0; z < N; ++z)
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                if (!Bit(words, at(x, y, z))) continue;
                bool border = false;
                for (int dz = -1; dz <= 1 && !border; ++dz)
                    for (int dy = -1; dy <= 1 && !border; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int nx = x + dx, ny = y + dy, nz = z + dz;
                            if (nx < 0 || nx >= N || ny < 0 || ny >= N || nz < 0 || nz >= N || !Bit(words, at(nx, ny, nz))) { border = true; break; }
                        }
                if (border) {
                    const size_t i = at(x, y, z);
#pragma omp atomic
                    bits[i >> 5] |= 1u << (i & 31);
                }
            }
    return mask;
}

void SeedTransformHost(bool parallel, const uint32_t* words, size_t n, int seeds, uint32_t* dist)
{
    cpuAssert(seeds == VP_EDT_SEEDS_SET || seeds == VP_EDT_SEEDS_UNSET || seeds == VP_EDT_SEEDS_BORDER, "Unknown distance transform seeds\n");
    if (seeds == VP_EDT_SEEDS_BORDER) {
        const std::vector<uint32_t> mask = BorderMask(parallel, words, n);
        TransformHost(parallel, mask.data(), false, n, dist);
    } else {
        TransformHost(parallel, words, seeds == VP_EDT_SEEDS_UNSET, n, dist);
    }
}

vp_frame WholeFrame(size_t n, float vs, const float origin[3])
{
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    return f;
}

// runs `call` on the one-device context between the timer brackets every GPU variant of the library prints
template <class Call>
void OnDevice(const char* label, const char* what, Call call)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, std::string(what) + " runs on one device (no -g > 1)\n");
    vp_ctx* ctx = vplib::Context();
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(call(ctx));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

}  // namespace

namespace VOX::detail {

void EdtHost(bool parallel, const uint32_t* words, size_t n, int seeds, uint32_t* dist)
{
    PROFILING_SCOPE(parallel ? "OpenMPEdt" : "SequentialEdt");
    SeedTransformHost(parallel, words, n, seeds, dist);
}

void EdtDevice(int algo, const char* label, const uint32_t* words, size_t n, float vs, const float origin[3], int seeds, uint32_t* dist)
{
    const vp_frame f = WholeFrame(n, vs, origin);
    OnDevice(label, "The distance transform", [&](vp_ctx* ctx) { return vp_edt_host(ctx, &f, words, seeds, dist, algo); });
}

void MorphExactHost(bool parallel, uint32_t* words, size_t n, int op, uint32_t radius)
{
    PROFILING_SCOPE(parallel ? "OpenMPMorphExact" : "SequentialMorphExact");
    cpuAssert(op >= VP_MORPH_DILATE && op <= VP_MORPH_CLOSE, "Unknown morphology op\n");
    cpuAssert(radius <= 65535u, "Morphology radius outside 0..65535\n");
    if (radius == 0) return;
    const size_t voxels = n * n * n;
    const uint32_t r2 = radius * radius;
    std::vector<uint32_t> dist(voxels);
    auto one = [&](bool erode) {
        TransformHost(parallel, words, erode, n, dist.data());
        std::fill(words, words + (voxels + 31) / 32, 0u);
        for (size_t i = 0; i < voxels; ++i)
            if (erode ? dist[i] > r2 : dist[i] <= r2) words[i >> 5] |= 1u << (i & 31);
    };
    switch (op) {
        case VP_MORPH_DILATE: one(false); break;
        case VP_MORPH_ERODE:  one(true); break;
        case VP_MORPH_OPEN:   one(true); one(false); break;
        default:              one(false); one(true); break;
    }
}

void MorphExactDevice(int algo, const char* label, uint32_t* words, size_t n, float vs, const float origin[3], int op, uint32_t radius)
{
    const vp_frame f = WholeFrame(n, vs, origin);
    OnDevice(label, "The morphology", [&](vp_ctx* ctx) { return vp_edt_morph_host(ctx, &f, words, words, op, radius, algo); });
}

}  // namespace VOX::detail

namespace JFA::detail {

void ExactHost(bool parallel, const uint32_t* words, size_t n, float vs, float* sdf)
{
    PROFILING_SCOPE(parallel ? "OpenmpExactSDF" : "SequentialExactSDF");
    const size_t voxels = n * n * n;
    std::vector<uint32_t> dist(voxels);
    SeedTransformHost(parallel, words, n, VP_EDT_SEEDS_BORDER, dist.data());
    const float vs2 = vs * vs;
    for (size_t i = 0; i < voxels; ++i) {
        const bool set = Bit(words, i);
        if (dist[i] == kNone) { if (set) sdf[i] = INFINITY; continue; }   // unset voxels keep the caller's fill
        const float d = static_cast<float>(dist[i]) * vs2;
        sdf[i] = set ? d : std::copysign(d, sdf[i]);
    }
}

void ExactDevice(int algo, const char* label, const uint32_t* words, size_t n, float vs, const float origin[3], float* sdf)
{
    const vp_frame f = WholeFrame(n, vs, origin);
    // the sign of unset voxels comes from the caller's pre-fill, as in JFA::Compute
    float fill = -INFINITY;
    const size_t voxels = n * n * n;
    for (size_t i = 0; i < voxels; ++i)
        if (!Bit(words, i)) { fill = sdf[i]; break; }
    OnDevice(label, "The exact distance field", [&](vp_ctx* ctx) { return vp_edt_sdf_host(ctx, &f, words, fill, sdf, algo); });
}

}  // namespace JFA::detail
