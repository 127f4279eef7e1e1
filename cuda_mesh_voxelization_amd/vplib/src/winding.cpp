// winding.cpp -- VOX::ComputeWinding back ends: the host restatement of vp_winding (include/vphip.h) and the marshalling of the GPU
// variants onto the C ABI.
//
// The host path is the contract in plain C++ (this file is compiled with -ffp-contract=off): the pyramid is built by loops over the
// triangles and the levels, and every brick walks it by recursion into two lists -- far nodes and near leaves -- which its 512 voxels
// then evaluate one at a time with the header's float32 expressions, every term quantised to a 64-bit integer before it is added.  The
// sums are integers, so the order of the lists cannot matter.  n must be a multiple of 8.
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
inline float Max2(float a, float b) { return a > b ? a : b; }

inline uint32_t Ord(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float Unord(uint32_t k)
{
    const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}

float Atan2W(float y, float x)
{
    const float ax = std::fabs(x), ay = std::fabs(y);
    const float t = std::min(ax, ay) / std::max(ax, ay);
    const float s = t * t;
    float q = VP_WN_ATAN_C9;
    q = (q * s) + VP_WN_ATAN_C8; q = (q * s) + VP_WN_ATAN_C7; q = (q * s) + VP_WN_ATAN_C6;
    q = (q * s) + VP_WN_ATAN_C5; q = (q * s) + VP_WN_ATAN_C4; q = (q * s) + VP_WN_ATAN_C3;
    q = (q * s) + VP_WN_ATAN_C2; q = (q * s) + VP_WN_ATAN_C1; q = (q * s) + VP_WN_ATAN_C0;
    float r = q * t;
    if (ay > ax) r = VP_WN_HALF_PI - r;
    if (x < 0.0f) r = VP_WN_PI - r;
    return y < 0.0f ? -r : r;
}

inline int64_t Quantise(float omega) { return std::llrint(static_cast<double>(omega) * 68719476736.0); }

int64_t ExactTerm(const float* p, const float* tri)
{
    float a[3], b[3], c[3];
    for (int i = 0; i < 3; ++i) { a[i] = tri[i] - p[i]; b[i] = tri[3 + i] - p[i]; c[i] = tri[6 + i] - p[i]; }
    const float la = std::sqrt(Dot(a, a)), lb = std::sqrt(Dot(b, b)), lc = std::sqrt(Dot(c, c));
    const float x[3] = {(b[1] * c[2]) - (b[2] * c[1]), (b[2] * c[0]) - (b[0] * c[2]), (b[0] * c[1]) - (b[1] * c[0])};
    const float det = Dot(a, x);
    const float den = ((((la * lb) * lc) + (Dot(a, b) * lc)) + (Dot(b, c) * la)) + (Dot(c, a) * lb);
    if (det == 0.0f || !std::isfinite(det) || !std::isfinite(den)) return 0;
    return Quantise(2.0f * Atan2W(det, den));
}

struct Node {
    uint32_t count = 0;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};   // the box in the integer order of floats
    uint64_t area[3] = {0, 0, 0};                                  // sums modulo 2^64
    float c[3] = {0, 0, 0}, r = 0, nv[3] = {0, 0, 0};
};

int64_t FarTerm(const float* p, const Node& nd)
{
    const float d[3] = {nd.c[0] - p[0], nd.c[1] - p[1], nd.c[2] - p[2]};
    const float r2 = Dot(d, d);
    const float om = Dot(d, nd.nv) / (r2 * std::sqrt(r2));
    return std::isfinite(om) ? Quantise(om) : 0;
}

struct Pyramid {
    uint32_t nb = 0;
    std::vector<uint32_t> dim;
    std::vector<std::vector<Node>> level;
    std::vector<uint32_t> leafOff;                                 // nb^3 + 1
    std::vector<float> rec;                                        // nine floats per valid triangle, sorted by leaf
};

int64_t QuantiseArea(float nrm, double u)
{
    double s = (static_cast<double>(nrm) * 8388608.0) / u;
    if (s > 4611686018427387904.0) s = 4611686018427387904.0;
    if (s < -4611686018427387904.0) s = -4611686018427387904.0;
    if (s != s) s = 0.0;
    return std::llrint(s);
}

Pyramid BuildPyramid(size_t n, float vs, const float origin[3], const Mesh& mesh)
{
    Pyramid py;
    py.nb = static_cast<uint32_t>(n / 8);
    for (int k = 0;; ++k) {
        py.dim.push_back((py.nb + (1u << k) - 1u) >> k);
        if (py.dim.back() == 1) break;
    }
    for (uint32_t d : py.dim) py.level.emplace_back(static_cast<size_t>(d) * d * d);
    const uint32_t nb = py.nb;
    const double u = static_cast<double>(vs) * static_cast<double>(vs);
    std::vector<uint32_t> leafOf;
    std::vector<float> verts;                                      // nine floats per valid triangle, input order
    const size_t ntris = mesh.TrianglesSize();
    for (size_t t = 0; t < ntris; ++t) {
        const uint32_t* idx = &mesh.FacesCoords[3 * t];
        if (idx[0] >= mesh.Coords.size() || idx[1] >= mesh.Coords.size() || idx[2] >= mesh.Coords.size()) continue;
        float v[3][3];
        bool finite = true;
        for (int k = 0; k < 3; ++k) {
            const Position& P = mesh.Coords[idx[k]];
            v[k][0] = P.X; v[k][1] = P.Y; v[k][2] = P.Z;
            for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(v[k][a]);
        }
        if (!finite) continue;
        float e0[3], e1[3];
        for (int a = 0; a < 3; ++a) { e0[a] = v[1][a] - v[0][a]; e1[a] = v[2][a] - v[1][a]; }
        const float nrm[3] = {(e0[1] * e1[2]) - (e0[2] * e1[1]), (e0[2] * e1[0]) - (e0[0] * e1[2]), (e0[0] * e1[1]) - (e0[1] * e1[0])};
        if (nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f) continue;
        uint32_t b[3];
        for (int a = 0; a < 3; ++a) {
            const float g = ((v[0][a] + v[1][a]) + v[2][a]) / 3.0f;
            const float q = std::floor(((g - origin[a]) / vs) / 8.0f);
            b[a] = q >= static_cast<float>(nb - 1u) ? nb - 1u : (q > 0.0f ? static_cast<uint32_t>(q) : 0u);
        }
        const uint32_t leaf = b[0] + nb * (b[1] + nb * b[2]);
        Node& nd = py.level[0][leaf];
        ++nd.count;
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 3; ++k) { nd.lo[a] = std::min(nd.lo[a], Ord(v[k][a])); nd.hi[a] = std::max(nd.hi[a], Ord(v[k][a])); }
            nd.area[a] += static_cast<uint64_t>(QuantiseArea(nrm[a], u));
        }
        leafOf.push_back(leaf);
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) verts.push_back(v[k][a]);
    }
    py.leafOff.assign(static_cast<size_t>(nb) * nb * nb + 1, 0u);
    for (uint32_t l : leafOf) ++py.leafOff[l + 1];
    for (size_t i = 1; i < py.leafOff.size(); ++i) py.leafOff[i] += py.leafOff[i - 1];
    std::vector<uint32_t> cur(py.leafOff.begin(), py.leafOff.end() - 1);
    py.rec.resize(verts.size());
    for (size_t t = 0; t < leafOf.size(); ++t) std::memcpy(&py.rec[9 * static_cast<size_t>(cur[leafOf[t]]++)], &verts[9 * t], 36);
    for (size_t k = 0; k + 1 < py.dim.size(); ++k) {
        const uint32_t dl = py.dim[k], du = py.dim[k + 1];
        for (uint32_t z = 0; z < dl; ++z)
            for (uint32_t y = 0; y < dl; ++y)
                for (uint32_t x = 0; x < dl; ++x) {
                    const Node& c = py.level[k][x + static_cast<size_t>(dl) * (y + static_cast<size_t>(dl) * z)];
                    if (!c.count) continue;
                    Node& p = py.level[k + 1][(x >> 1) + static_cast<size_t>(du) * ((y >> 1) + static_cast<size_t>(du) * (z >> 1))];
                    p.count += c.count;
                    for (int a = 0; a < 3; ++a) { p.lo[a] = std::min(p.lo[a], c.lo[a]); p.hi[a] = std::max(p.hi[a], c.hi[a]); p.area[a] += c.area[a]; }
                }
    }
    const double unit = u * (1.0 / 16777216.0);
    for (auto& lv : py.level)
        for (Node& nd : lv) {
            if (!nd.count) continue;
            float h[3];
            for (int a = 0; a < 3; ++a) {
                const float lo = Unord(nd.lo[a]), hi = Unord(nd.hi[a]);
                h[a] = (hi - lo) / 2.0f;
                nd.c[a] = lo + h[a];
                nd.nv[a] = static_cast<float>(static_cast<double>(static_cast<int64_t>(nd.area[a])) * unit);
            }
            nd.r = std::sqrt(Dot(h, h));
        }
    return py;
}

struct BrickLists { std::vector<const Node*> far; std::vector<uint32_t> leaves; };

void Walk(const Pyramid& py, int k, uint32_t x, uint32_t y, uint32_t z, const float* blo, const float* bhi, float beta, BrickLists& out)
{
    const uint32_t d = py.dim[k];
    const size_t at = x + static_cast<size_t>(d) * (y + static_cast<size_t>(d) * z);
    const Node& nd = py.level[k][at];
    if (!nd.count) return;
    float g[3];
    for (int a = 0; a < 3; ++a) g[a] = Max2(0.0f, Max2(blo[a] - nd.c[a], nd.c[a] - bhi[a]));
    const float br = beta * nd.r;
    if (Dot(g, g) > br * br && beta > 0.0f) { out.far.push_back(&nd); return; }
    if (k == 0) { out.leaves.push_back(static_cast<uint32_t>(at)); return; }
    const uint32_t dl = py.dim[k - 1];
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t cx = 2 * x + (j & 1u), cy = 2 * y + ((j >> 1) & 1u), cz = 2 * z + (j >> 2);
        if (cx < dl && cy < dl && cz < dl) Walk(py, k - 1, cx, cy, cz, blo, bhi, beta, out);
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

}  // namespace

namespace VOX::detail {

void WindingHost(bool parallel, uint32_t* words, size_t n, float vs, const float origin[3], const Mesh& mesh, float beta, float level, float* w)
{
    const std::string L = parallel ? "OpenMPWinding" : "SequentialWinding";
    PROFILING_SCOPE(L + "(" + mesh.Name + ")");
    cpuAssert(n % 8 == 0 && n >= 8, "Winding number: the grid side must be a multiple of 8\n");
    cpuAssert((beta == 0.0f || (beta >= 1.0f && beta <= 64.0f)) && std::isfinite(level), "Winding number: beta is 0 or 1..64, the level finite\n");
    const Pyramid py = BuildPyramid(n, vs, origin, mesh);
    const int nb = static_cast<int>(py.nb), top = static_cast<int>(py.dim.size()) - 1;
    std::vector<uint8_t> inside(n * n * n, 0);
#pragma omp parallel for schedule(dynamic, 1) if (parallel)
    for (int brick = 0; brick < nb * nb * nb; ++brick) {
        const int b[3] = {brick % nb, (brick / nb) % nb, brick / (nb * nb)};
        float blo[3], bhi[3];
        for (int a = 0; a < 3; ++a) { blo[a] = Centre(origin[a], 8 * b[a], vs); bhi[a] = Centre(origin[a], 8 * b[a] + 7, vs); }
        BrickLists lists;
        Walk(py, top, 0, 0, 0, blo, bhi, beta, lists);
        for (int v = 0; v < 512; ++v) {
            const int x = 8 * b[0] + (v & 7), y = 8 * b[1] + ((v >> 3) & 7), z = 8 * b[2] + (v >> 6);
            const float p[3] = {Centre(origin[0], x, vs), Centre(origin[1], y, vs), Centre(origin[2], z, vs)};
            uint64_t s = 0;                                        // modulo 2^64, like every form
            for (const Node* nd : lists.far) s += static_cast<uint64_t>(FarTerm(p, *nd));
            for (uint32_t leaf : lists.leaves)
                for (uint32_t j = py.leafOff[leaf]; j < py.leafOff[leaf + 1]; ++j) s += static_cast<uint64_t>(ExactTerm(p, &py.rec[9 * static_cast<size_t>(j)]));
            const float wv = static_cast<float>((static_cast<double>(static_cast<int64_t>(s)) * (1.0 / 68719476736.0)) / VP_WN_FOUR_PI);
            const size_t i = static_cast<size_t>(x) + n * (static_cast<size_t>(y) + n * static_cast<size_t>(z));
            if (w) w[i] = wv;
            inside[i] = wv >= level ? 1 : 0;
        }
    }
    if (words) {
        const size_t total = n * n * n;
        for (size_t i = 0; i < (total + 31) / 32; ++i) {
            uint32_t bits = 0;
            for (size_t k = 0; k < 32 && i * 32 + k < total; ++k) bits |= static_cast<uint32_t>(inside[i * 32 + k]) << k;
            words[i] = bits;
        }
    }
}

void WindingDevice(int algo, const char* label, uint32_t* words, size_t n, float vs, const float origin[3], const Mesh& mesh, float beta,
                   float level, float* w)
{
    const std::string L(label);
    PROFILING_SCOPE(L + "(" + mesh.Name + ")");
    cpuAssert(vplib::Multi() == nullptr, "The winding number runs on one device (no -g > 1)\n");
    const vp_frame f = WholeFrame(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(L + "::Processing");
        gpuAssert(vp_winding_host(ctx, &f, reinterpret_cast<const float*>(mesh.Coords.data()), mesh.Coords.size(), mesh.FacesCoords.data(),
                                  mesh.TrianglesSize(), beta, level, algo, w, words, nullptr));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

}  // namespace VOX::detail
