// morph.cpp -- VOX::Morph back ends: the host restatement of vp_morph (include/vphip.h) and the marshalling of the GPU variants onto
// the C ABI.
//
// The host path is a different formulation from the kernels (which stack x segments of the ball): the exact squared distance to the
// nearest set voxel, capped, in three separable integer passes --
//   g1(x, y, z) = min over |dx| <= r, x + dx in the grid and set, of dx^2
//   g2(x, y, z) = min over |dy| <= r, y + dy in the grid, of g1(x, y + dy, z) + dy^2
//   g3(x, y, z) = min over |dz| <= r, z + dz in the grid, of g2(x, y, z + dz) + dz^2
// -- and dilate = (g3 <= r^2).  "No set voxel in reach" is kInf, larger than any sum that can pass the test.  Erosion complements
// the grid before and after; voxels outside the grid are never visited, so they read as empty after the complement, i.e. as set.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace VOX::detail {

namespace {

constexpr uint16_t kInf = 4096;     // > 32^2; three of them still fit 16 bits

void DilateHost(bool parallel, uint32_t* words, size_t n, int r)
{
    const int N = static_cast<int>(n);
    const size_t plane = n * n;
    std::vector<uint16_t> g2(plane * n);
#pragma omp parallel for schedule(static) if (parallel)
    for (int z = 0; z < N; ++z) {
        std::vector<uint16_t> g1(plane);
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                uint16_t best = kInf;
                for (int dx = -r; dx <= r; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= N) continue;
                    const size_t v = static_cast<size_t>(z) * plane + static_cast<size_t>(y) * n + static_cast<size_t>(xx);
                    if ((words[v >> 5] >> (v & 31)) & 1u) best = std::min<uint16_t>(best, static_cast<uint16_t>(dx * dx));
                }
                g1[static_cast<size_t>(y) * n + x] = best;
            }
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                uint16_t best = kInf;
                for (int dy = -r; dy <= r; ++dy) {
                    const int yy = y + dy;
                    if (yy < 0 || yy >= N) continue;
                    best = std::min<uint16_t>(best, static_cast<uint16_t>(g1[static_cast<size_t>(yy) * n + x] + dy * dy));
                }
                g2[static_cast<size_t>(z) * plane + static_cast<size_t>(y) * n + x] = best;
            }
    }
    const int r2 = r * r;
#pragma omp parallel for schedule(static) if (parallel)
    for (int z = 0; z < N; ++z) {
        // the bits of one word are gathered and ORed in at once; atomically, because a word straddles two planes where n^2 % 32 != 0
        uint32_t acc = 0u;
        for (size_t i = 0; i < plane; ++i) {
            int best = kInf;
            for (int dz = -r; dz <= r; ++dz) {
                const int zz = z + dz;
                if (zz < 0 || zz >= N) continue;
                best = std::min(best, static_cast<int>(g2[static_cast<size_t>(zz) * plane + i]) + dz * dz);
            }
            const size_t v = static_cast<size_t>(z) * plane + i;
            if (best <= r2) acc |= 1u << (v & 31);
            if ((v & 31) == 31 || i + 1 == plane) {
                if (acc) {
#pragma omp atomic
                    words[v >> 5] |= acc;
                }
                acc = 0u;
            }
        }
    }
}

void Complement(uint32_t* words, size_t n)
{
    const size_t voxels = n * n * n, full = voxels / 32;
    for (size_t i = 0; i < full; ++i) words[i] = ~words[i];
    if (voxels % 32) words[full] = ~words[full] & ((1u << (voxels % 32)) - 1u);
}

}  // namespace

void MorphHost(bool parallel, uint32_t* words, size_t n, int op, uint32_t radius)
{
    PROFILING_SCOPE(parallel ? "OpenMPMorph" : "SequentialMorph");
    const int r = static_cast<int>(radius);
    if (r == 0) return;
    auto dilate = [&] { DilateHost(parallel, words, n, r); };
    auto erode = [&] { Complement(words, n); DilateHost(parallel, words, n, r); Complement(words, n); };
    switch (op) {
        case VP_MORPH_DILATE: dilate(); break;
        case VP_MORPH_ERODE:  erode(); break;
        case VP_MORPH_OPEN:   erode(); dilate(); break;
        case VP_MORPH_CLOSE:  dilate(); erode(); break;
        default: cpuAssert(false, "Unknown morphology op\n");
    }
}

void MorphDevice(int algo, const char* label, uint32_t* words, size_t n, float vs, const float origin[3], int op, uint32_t radius)
{
    const std::string L(label);
    PROFILING_SCOPE(L);
    cpuAssert(vplib::Multi() == nullptr, "The morphology runs on one device (no -g > 1)\n");
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
        gpuAssert(vp_morph_host(ctx, &f, words, words, op, radius, algo));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

}  // namespace VOX::detail
