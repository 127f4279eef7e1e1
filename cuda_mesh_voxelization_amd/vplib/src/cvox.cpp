// cvox.cpp -- VOX::ComputeConservative back ends: the host restatement of the conservative (26-separating) predicate of
// include/vphip.h (vp_voxelize_conservative) and the marshalling of the GPU variants onto the C ABI.  Build with -ffp-contract=off:
// the float32 expressions and their association are the contract, bit for bit with csrc/cvox.hip.
//
// The host walks every voxel of each triangle's bounding-box index range and evaluates the WHOLE predicate there (box test included);
// it takes none of the GPU's per-row plane intervals, so it checks them.
#include <atomic>
#include <cmath>
#include <cstdio>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace VOX::detail {

namespace {

inline float Corner(float o, long i, float vs) { return o + (static_cast<float>(i) * vs); }
inline float Pos(float x) { return x > 0.0f ? x : 0.0f; }

// The index range [lo, hi] in [0, n) of voxels whose box test passes on one axis (corner monotone in the index: the guess is stepped).
bool AxisRange(float mn, float mx, float o, float vs, long n, long& lo, long& hi)
{
    lo = static_cast<long>(std::fmin(std::fmax(std::floor((mn - o) / vs), 0.0f), static_cast<float>(n)));
    while (lo > 0 && Corner(o, lo - 1, vs) + vs >= mn) --lo;
    while (lo < n && !(Corner(o, lo, vs) + vs >= mn)) ++lo;
    hi = static_cast<long>(std::fmin(std::fmax(std::floor((mx - o) / vs), -1.0f), static_cast<float>(n - 1)));
    while (hi < n - 1 && Corner(o, hi + 1, vs) <= mx) ++hi;
    while (hi >= 0 && !(Corner(o, hi, vs) <= mx)) --hi;
    return lo <= hi;
}

void Triangle(const Mesh& mesh, size_t t, uint32_t* words, size_t n, float vs, const float o[3], bool atomic)
{
    const uint32_t* idx = &mesh.FacesCoords[3 * t];
    if (idx[0] >= mesh.Coords.size() || idx[1] >= mesh.Coords.size() || idx[2] >= mesh.Coords.size()) return;
    float v[3][3];
    for (int k = 0; k < 3; ++k) {
        const Position& P = mesh.Coords[idx[k]];
        v[k][0] = P.X; v[k][1] = P.Y; v[k][2] = P.Z;
        for (int a = 0; a < 3; ++a) if (!std::isfinite(v[k][a])) return;
    }
    float e[3][3];
    for (int a = 0; a < 3; ++a) { e[0][a] = v[1][a] - v[0][a]; e[1][a] = v[2][a] - v[1][a]; e[2][a] = v[0][a] - v[2][a]; }
    const Position nrmP = Position::Cross(Position(e[0][0], e[0][1], e[0][2]), Position(e[1][0], e[1][1], e[1][2]));
    const float nrm[3] = {nrmP.X, nrmP.Y, nrmP.Z};
    if (nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f) return;
    float mn[3], mx[3], c[3], co[3];
    for (int a = 0; a < 3; ++a) {
        mn[a] = std::min(std::min(v[0][a], v[1][a]), v[2][a]);
        mx[a] = std::max(std::max(v[0][a], v[1][a]), v[2][a]);
        c[a] = nrm[a] > 0.0f ? vs : 0.0f;
        co[a] = vs - c[a];
    }
    const float d1 = Position::Dot(nrmP, Position(c[0] - v[0][0], c[1] - v[0][1], c[2] - v[0][2]));
    const float d2 = Position::Dot(nrmP, Position(co[0] - v[0][0], co[1] - v[0][1], co[2] - v[0][2]));
    float ne[3][3][3];
    for (int q = 0; q < 3; ++q) {
        const int U = q, V = (q + 1) % 3, S = (q + 2) % 3;
        const float sg = nrm[S] >= 0.0f ? 1.0f : -1.0f;
        for (int i = 0; i < 3; ++i) {
            const float nu = (-e[i][V]) * sg, nv = e[i][U] * sg;
            ne[q][i][0] = nu; ne[q][i][1] = nv;
            ne[q][i][2] = ((-((nu * v[i][U]) + (nv * v[i][V]))) + Pos(vs * nu)) + Pos(vs * nv);
        }
    }
    long lo[3], hi[3];
    const long N = static_cast<long>(n);
    for (int a = 0; a < 3; ++a) if (!AxisRange(mn[a], mx[a], o[a], vs, N, lo[a], hi[a])) return;
    for (long k = lo[2]; k <= hi[2]; ++k)
        for (long j = lo[1]; j <= hi[1]; ++j)
            for (long i = lo[0]; i <= hi[0]; ++i) {
                const float p[3] = {Corner(o[0], i, vs), Corner(o[1], j, vs), Corner(o[2], k, vs)};
                bool ok = true;
                for (int a = 0; a < 3; ++a) ok = ok && p[a] <= mx[a] && p[a] + vs >= mn[a];
                if (!ok) continue;
                const float t = Position::Dot(nrmP, Position(p[0], p[1], p[2]));
                const float s1 = t + d1, s2 = t + d2;
                if ((s1 > 0.0f && s2 > 0.0f) || (s1 < 0.0f && s2 < 0.0f)) continue;
                for (int q = 0; q < 3 && ok; ++q) {
                    const int U = q, V = (q + 1) % 3;
                    for (int m = 0; m < 3 && ok; ++m) ok = ((ne[q][m][0] * p[U]) + (ne[q][m][1] * p[V])) + ne[q][m][2] >= 0.0f;
                }
                if (!ok) continue;
                const size_t bit = static_cast<size_t>(i) + n * (static_cast<size_t>(j) + n * static_cast<size_t>(k));
                const uint32_t m = 1u << (bit & 31);
                if (atomic) std::atomic_ref<uint32_t>(words[bit >> 5]).fetch_or(m, std::memory_order_relaxed);
                else words[bit >> 5] |= m;
            }
}

}  // namespace

void ConservativeHost(bool parallel, uint32_t* words, size_t n, float vs, const float origin[3], const Mesh& mesh)
{
    const std::string L = parallel ? "OpenMPConservativeVox" : "SequentialConservativeVox";
    PROFILING_SCOPE(L + "(" + mesh.Name + ")");
    PROFILING_SCOPE(L + "::Processing");
    const long numTriangle = static_cast<long>(mesh.TrianglesSize());
    if (parallel) {
#pragma omp parallel for schedule(dynamic, 64)
        for (long t = 0; t < numTriangle; ++t) Triangle(mesh, static_cast<size_t>(t), words, n, vs, origin, true);     // OR commutes
    } else {
        for (long t = 0; t < numTriangle; ++t) Triangle(mesh, static_cast<size_t>(t), words, n, vs, origin, false);
    }
}

void ConservativeDevice(int algo, const char* label, uint32_t* words, size_t n, float vs, const float origin[3], const Mesh& mesh)
{
    const std::string L(label);
    PROFILING_SCOPE(L + "(" + mesh.Name + ")");
    cpuAssert(vplib::Multi() == nullptr, "The conservative voxelizer runs on one device (no -g > 1)\n");
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
        gpuAssert(vp_voxelize_conservative_host(ctx, &f, words, reinterpret_cast<const float*>(mesh.Coords.data()), mesh.Coords.size(),
                                                mesh.FacesCoords.data(), mesh.TrianglesSize(), algo));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

}  // namespace VOX::detail
