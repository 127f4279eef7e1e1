// meshdist.cpp -- VOX::MeshDistance back ends: the host restatement of vp_mesh_distance (include/vphip.h) and the marshalling of the GPU
// variants onto the C ABI.
//
// The host path is plain loops: every valid triangle over the voxels of its band box -- per axis the centres within B (1 + 2^-18) of the
// vertex bounding box grown by 2^-19 of the largest |coordinate|, the margin argued in DESIGN.md section 15 -- with the header's float32
// expressions (this file is compiled with -ffp-contract=off), a 64-bit key (D2 bits << 32) | index per voxel and a minimum over it.  No
// plane test, no bricks: it is the form the kernels are pinned to.  Any grid side is served.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/vox.h"
#include "vp_runtime.h"

namespace {

inline float Centre(float o, int i, float vs) { return o + ((static_cast<float>(i) * vs) + (vs / 2.0f)); }
inline float Dot(const float* a, const float* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }

// D2(p, t) of the contract: the region walk of Ericson 5.1.5
float TriD2(const float* p, const float* a, const float* b, const float* c)
{
    float ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
    for (int i = 0; i < 3; ++i) { ab[i] = b[i] - a[i]; ac[i] = c[i] - a[i]; ap[i] = p[i] - a[i]; bp[i] = p[i] - b[i]; cp[i] = p[i] - c[i]; }
    const float d1 = Dot(ab, ap), d2 = Dot(ac, ap), d3 = Dot(ab, bp), d4 = Dot(ac, bp), d5 = Dot(ab, cp), d6 = Dot(ac, cp);
    const float vc = (d1 * d4) - (d3 * d2), vb = (d5 * d2) - (d1 * d6), va = (d3 * d6) - (d5 * d4);
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        for (int i = 0; i < 3; ++i) q[i] = a[i];
    } else if (d3 >= 0.0f && d4 <= d3) {
        for (int i = 0; i < 3; ++i) q[i] = b[i];
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = d1 / (d1 - d3);
        for (int i = 0; i < 3; ++i) q[i] = a[i] + (ab[i] * v);
    } else if (d6 >= 0.0f && d5 <= d6) {
        for (int i = 0; i < 3; ++i) q[i] = c[i];
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = d2 / (d2 - d6);
        for (int i = 0; i < 3; ++i) q[i] = a[i] + (ac[i] * w);
    } else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
        const float w = e43 / (e43 + e56);
        for (int i = 0; i < 3; ++i) q[i] = b[i] + ((c[i] - b[i]) * w);
    } else {
        const float den = (va + vb) + vc;
        const float v0 = vb / den, w0 = vc / den;
        float v = v0 > 0.0f ? v0 : 0.0f;
        v = v < 1.0f ? v : 1.0f;
        const float wl = 1.0f - v;
        float w = w0 > 0.0f ? w0 : 0.0f;
        w = w < wl ? w : wl;
        for (int i = 0; i < 3; ++i) q[i] = (a[i] + (ab[i] * v)) + (ac[i] * w);
    }
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

struct HostTri {
    float v[3][3];
    uint32_t index;
    int lo[3], hi[3];                                              // voxel range of the band box, inclusive
};

// the indices in [0, n) whose centre lies in [L, H]
bool CentreRange(double L, double H, float o, float vs, int n, int& lo, int& hi)
{
    lo = 0;
    while (lo < n && !(static_cast<double>(Centre(o, lo, vs)) >= L)) ++lo;
    hi = n - 1;
    while (hi >= 0 && !(static_cast<double>(Centre(o, hi, vs)) <= H)) --hi;
    return lo <= hi;
}

vp_frame WholeFrame(size_t n, float vs, const float origin[3])
{
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    return f;
}

}  // namespace

namespace VOX::detail {

void MeshDistanceHost(bool parallel, const uint32_t* sign, size_t n, float vs, const float origin[3], const Mesh& mesh, uint32_t band,
                      float* dist2, uint32_t* nearest)
{
    const std::string L = parallel ? "OpenMPMeshDistance" : "SequentialMeshDistance";
    PROFILING_SCOPE(L + "(" + mesh.Name + ")");
    cpuAssert(band >= 1 && band <= 32, "Mesh distance band outside 1..32\n");
    const float B = static_cast<float>(band) * vs;
    const float B2 = B * B;
    const double reach = std::sqrt(static_cast<double>(B2)) * (1.0 + 1.0 / 262144.0);
    const int N = static_cast<int>(n);

    std::vector<HostTri> tris;
    const size_t ntris = mesh.TrianglesSize();
    for (size_t t = 0; t < ntris; ++t) {
        const uint32_t* idx = &mesh.FacesCoords[3 * t];
        if (idx[0] >= mesh.Coords.size() || idx[1] >= mesh.Coords.size() || idx[2] >= mesh.Coords.size()) continue;
        HostTri h;
        bool finite = true;
        float mt = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const Position& P = mesh.Coords[idx[k]];
            h.v[k][0] = P.X; h.v[k][1] = P.Y; h.v[k][2] = P.Z;
            for (int a = 0; a < 3; ++a) { finite = finite && std::isfinite(h.v[k][a]); mt = std::max(mt, std::fabs(h.v[k][a])); }
        }
        if (!finite) continue;
        float e0[3], e1[3];
        for (int a = 0; a < 3; ++a) { e0[a] = h.v[1][a] - h.v[0][a]; e1[a] = h.v[2][a] - h.v[1][a]; }
        const float nx = (e0[1] * e1[2]) - (e0[2] * e1[1]);
        const float ny = (e0[2] * e1[0]) - (e0[0] * e1[2]);
        const float nz = (e0[0] * e1[1]) - (e0[1] * e1[0]);
        if (nx == 0.0f && ny == 0.0f && nz == 0.0f) continue;
        const double e = static_cast<double>(mt) * (1.0 / 524288.0);
        bool any = true;
        for (int a = 0; a < 3 && any; ++a) {
            const double mn = std::min({h.v[0][a], h.v[1][a], h.v[2][a]}), mx = std::max({h.v[0][a], h.v[1][a], h.v[2][a]});
            any = CentreRange(mn - e - reach, mx + e + reach, origin[a], vs, N, h.lo[a], h.hi[a]);
        }
        if (!any) continue;
        h.index = static_cast<uint32_t>(t);
        tris.push_back(h);
    }

    uint32_t b2bits;
    std::memcpy(&b2bits, &B2, 4);
    const uint64_t none = (static_cast<uint64_t>(b2bits) << 32) | VP_MESH_NONE;
    std::vector<uint64_t> keys(n * n * n, none);
#pragma omp parallel for schedule(dynamic, 1) if (parallel)
    for (int z = 0; z < N; ++z) {
        for (const HostTri& h : tris) {
            if (z < h.lo[2] || z > h.hi[2]) continue;
            for (int y = h.lo[1]; y <= h.hi[1]; ++y)
                for (int x = h.lo[0]; x <= h.hi[0]; ++x) {
                    const float p[3] = {Centre(origin[0], x, vs), Centre(origin[1], y, vs), Centre(origin[2], z, vs)};
                    const float d = TriD2(p, h.v[0], h.v[1], h.v[2]);
                    if (!(d < B2)) continue;                       // NaN and infinity fail as well
                    uint32_t bits;
                    std::memcpy(&bits, &d, 4);
                    uint64_t& k = keys[static_cast<size_t>(x) + n * (static_cast<size_t>(y) + n * static_cast<size_t>(z))];
                    k = std::min(k, (static_cast<uint64_t>(bits) << 32) | h.index);
                }
        }
    }
    for (size_t i = 0; i < keys.size(); ++i) {
        const uint32_t bits = static_cast<uint32_t>(keys[i] >> 32);
        float m;
        std::memcpy(&m, &bits, 4);
        const bool set = !sign || ((sign[i >> 5] >> (i & 31)) & 1u);
        dist2[i] = set ? m : -m;
        if (nearest) nearest[i] = static_cast<uint32_t>(keys[i]);
    }
}

void MeshDistanceDevice(int algo, const char* label, const uint32_t* sign, size_t n, float vs, const float origin[3], const Mesh& mesh,
                        uint32_t band, float* dist2, uint32_t* nearest)
{
    const std::string L(label);
    PROFILING_SCOPE(L + "(" + mesh.Name + ")");
    cpuAssert(vplib::Multi() == nullptr, "The mesh distance field runs on one device (no -g > 1)\n");
    const vp_frame f = WholeFrame(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_mesh_distance_host(ctx, &f, reinterpret_cast<const float*>(mesh.Coords.data()), mesh.Coords.size(), mesh.FacesCoords.data(),
                                        mesh.TrianglesSize(), sign, band, dist2, nearest, algo));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

}  // namespace VOX::detail
