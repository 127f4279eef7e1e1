// meshdist.hip -- narrow-band squared distance from voxel centres to the TRIANGLES of a mesh, with the nearest face, for gfx950 (MI355X).
//
// Per (voxel, triangle) pair the squared distance is one fixed float32 expression (tri_d2 below: the region walk of Ericson, Real-Time
// Collision Detection 5.1.5, every operation one IEEE operation, no FMA contraction); the field is min(B2, the minimum over the triangles)
// and the nearest face the lowest index that attains it -- the lexicographic minimum of (D2 bits, index), which does not depend on the order
// of evaluation or on which pairs were culled.  The contract is in include/vphip.h (vp_mesh_distance) and DESIGN.md section 15; this file,
// the host restatement (vplib/src/meshdist.cpp) and the tests' numpy restatement agree bit for bit.
//
// Candidate ranges never decide a value: every cull below only skips pairs whose computed D2 provably fails D2 < B2.  The closest point q
// the walk returns lies in the vertex bounding box grown by e = 2^-19 Mt (Mt = the triangle's largest |coordinate|) and within 2^-17 M of
// the plane (DESIGN.md section 15 has the argument), so a pair is skipped when
//   box    the squared gap between p and that grown box exceeds B2c = B2 (1 + 2^-18), or
//   plane  |N . p - k| > Bp = B (1 + 2^-18) + 2^-16 M, N the unit normal and k = N . a computed in double (no plane test for a sliver whose
//          normal double cannot resolve).
// The same two bounds serve the voxel ranges of a triangle (per axis, in double), the brick test of the binning (in double, over the
// brick's centres) and the per-pair test of the gather (in float).
//
// NAIVE: md_naive -- one thread per triangle over the voxels of its band box, one 64-bit atomicMin per accepted pair on the key
//        (D2 bits << 32) | index in an 8 n^3-byte volume of the context; md_split turns keys into the two outputs.
// TILED: md_setup   one thread per triangle: the record (vertices, grown box, plane) and its range of 8 x 8 x 8 bricks
//        md_scan    exclusive scan of the BRICK ROWS of all triangles, from the compact row counts md_setup leaves (one workgroup, wg_scan.h)
//        md_bin     count, then write: one lane per (triangle, brick row) over the whole device, found by a binary search of the scan; the
//                   lane walks the bricks of its row along x (at most n / 8) -- a triangle that spans the grid is thousands of rows
//        md_offsets exclusive scan of the brick counts of a z range of bricks (booked under the scan's timing key)
//        md_brick   one workgroup per brick, bricks with an empty list leave at once: records staged through LDS 64 at a time, every lane
//                   owns two voxels and keeps (D2, index) in registers; one plain store per voxel and output
//        md_fill    streaming fill of the bricks with an empty list: s B2 / NONE
// The list of a z range of bricks is capped (kListCap entries); a grid whose lists are longer runs in several ranges.
#include "vp_internal.h"
#include "wg_scan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

namespace vp {

namespace {

constexpr uint32_t kNoTri = VP_MESH_NONE;
constexpr int kBatch = 64;                      // records per LDS batch
constexpr int kRecU4 = 6;                       // record: 24 dwords = 6 x 16 B; a batch is 6 KiB of LDS
constexpr uint64_t kListCap = 1ull << 27;       // list entries (4 B each) per z range of bricks: 512 MiB

struct MRec {
    float a[3], b[3], c[3];
    float lo[3], hi[3];                         // vertex bounding box grown by e
    float nrm[3], k, bp;                        // plane bound: |nrm . p - k| > bp is out of the band (nrm = 0, bp = inf: no plane test)
    uint32_t idx;                               // the triangle's index, kNoTri: contributes nothing
    uint32_t bxy, bz;                           // brick range: bx0 | bx1 << 8 | by0 << 16 | by1 << 24, bz0 | bz1 << 8; bz = ~0: none
    uint32_t pad;
};
static_assert(sizeof(MRec) == kRecU4 * 16, "record layout");

struct Band {
    float b2;                                   // B2 = B * B, B = (float)band * vs
    float b2c;                                  // B2 (1 + 2^-18), rounded up
    float bm;                                   // B (1 + 2^-18), rounded up
    float mp;                                   // largest |coordinate| of a voxel centre
    double bd;                                  // sqrt(b2c)
};

__device__ __forceinline__ float centre(float o, int i, float vs) { return o + (((float)i * vs) + (vs / 2.0f)); }
__device__ __forceinline__ float dot3(const float* a, const float* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }

// D2(p, t) of the contract.  The result may be NaN or infinite; the caller drops whatever fails D2 < B2.
__device__ __forceinline__ float tri_d2(const float* p, const float* a, const float* b, const float* c)
{
    float ab[3], ac[3], ap[3], q[3];
    for (int i = 0; i < 3; ++i) { ab[i] = b[i] - a[i]; ac[i] = c[i] - a[i]; ap[i] = p[i] - a[i]; }
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    bool done = false;
    if (d1 <= 0.0f && d2 <= 0.0f) { for (int i = 0; i < 3; ++i) q[i] = a[i]; done = true; }                     // vertex a
    float d3 = 0.0f, d4 = 0.0f, d5 = 0.0f, d6 = 0.0f, vc = 0.0f, vb = 0.0f;
    if (!done) {
        float bp[3];
        for (int i = 0; i < 3; ++i) bp[i] = p[i] - b[i];
        d3 = dot3(ab, bp); d4 = dot3(ac, bp);
        if (d3 >= 0.0f && d4 <= d3) { for (int i = 0; i < 3; ++i) q[i] = b[i]; done = true; }                   // vertex b
    }
    if (!done) {
        vc = (d1 * d4) - (d3 * d2);
        if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {                                                          // edge ab
            const float v = d1 / (d1 - d3);
            for (int i = 0; i < 3; ++i) q[i] = a[i] + (ab[i] * v);
            done = true;
        }
    }
    if (!done) {
        float cp[3];
        for (int i = 0; i < 3; ++i) cp[i] = p[i] - c[i];
        d5 = dot3(ab, cp); d6 = dot3(ac, cp);
        if (d6 >= 0.0f && d5 <= d6) { for (int i = 0; i < 3; ++i) q[i] = c[i]; done = true; }                   // vertex c
    }
    if (!done) {
        vb = (d5 * d2) - (d1 * d6);
        if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {                                                          // edge ac
            const float w = d2 / (d2 - d6);
            for (int i = 0; i < 3; ++i) q[i] = a[i] + (ac[i] * w);
            done = true;
        }
    }
    if (!done) {
        const float va = (d3 * d6) - (d5 * d4);
        const float e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {                                                        // edge bc
            const float w = e43 / (e43 + e56);
            for (int i = 0; i < 3; ++i) q[i] = b[i] + ((c[i] - b[i]) * w);
        } else {                                                                                               // face
            const float den = (va + vb) + vc;
            const float v0 = vb / den, w0 = vc / den;
            float v = v0 > 0.0f ? v0 : 0.0f;                      // the clamps are the identity in exact arithmetic; NaN -> 0
            v = v < 1.0f ? v : 1.0f;
            const float wl = 1.0f - v;
            float w = w0 > 0.0f ? w0 : 0.0f;
            w = w < wl ? w : wl;
            for (int i = 0; i < 3; ++i) q[i] = (a[i] + (ab[i] * v)) + (ac[i] * w);
        }
    }
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// the two lower bounds in float: true = the pair provably fails D2 < B2
__device__ __forceinline__ bool pair_out(const float* p, const float* lo, const float* hi, const float* nrm, float k, float bp, float b2c)
{
    float g[3];
    for (int i = 0; i < 3; ++i) g[i] = fmaxf(fmaxf(lo[i] - p[i], p[i] - hi[i]), 0.0f);
    if (dot3(g, g) > b2c) return true;
    return fabsf(dot3(nrm, p) - k) > bp;
}

// [lo, hi] = the indices in [0, n) whose centre lies in [L, H]; the centre is monotone in the index, so a guess corrected by stepping is exact
__device__ __forceinline__ bool centre_range(double L, double H, float o, float vs, int n, int& lo, int& hi)
{
    const double gl = floor((L - (double)o) / (double)vs - 0.5), gh = floor((H - (double)o) / (double)vs - 0.5);
    lo = (int)fmin(fmax(gl, 0.0), (double)n);
    while (lo > 0 && (double)centre(o, lo - 1, vs) >= L) --lo;
    while (lo < n && !((double)centre(o, lo, vs) >= L)) ++lo;
    hi = (int)fmin(fmax(gh, -1.0), (double)(n - 1));
    while (hi < n - 1 && (double)centre(o, hi + 1, vs) <= H) ++hi;
    while (hi >= 0 && !((double)centre(o, hi, vs) <= H)) --hi;
    return lo <= hi;
}

// Triangle setup: validity (the three rules of vp_voxelize_conservative), the record and the voxel range of the band box.  false: the
// triangle contributes nothing, or no centre of the grid is within its band box.
__device__ __forceinline__ bool mtri_setup(const Frame& f, const Band& bn, const float* __restrict__ xyz, size_t nverts,
                                           const uint32_t* __restrict__ tri, size_t t, MRec& r, int* vl, int* vh)
{
    const uint32_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (id[0] >= nverts || id[1] >= nverts || id[2] >= nverts) return false;
    float v[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            v[k][a] = xyz[3 * (size_t)id[k] + a];
            if (!__builtin_isfinite(v[k][a])) return false;
        }
    float e0[3], e1[3];
    for (int a = 0; a < 3; ++a) { e0[a] = v[1][a] - v[0][a]; e1[a] = v[2][a] - v[1][a]; }
    const float nx = (e0[1] * e1[2]) - (e0[2] * e1[1]);
    const float ny = (e0[2] * e1[0]) - (e0[0] * e1[2]);
    const float nz = (e0[0] * e1[1]) - (e0[1] * e1[0]);
    if (nx == 0.0f && ny == 0.0f && nz == 0.0f) return false;
    float mt = 0.0f;
    for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) mt = fmaxf(mt, fabsf(v[k][a]));
    const double e = (double)mt * (1.0 / 524288.0);                      // 2^-19 Mt
    for (int a = 0; a < 3; ++a) {
        r.a[a] = v[0][a]; r.b[a] = v[1][a]; r.c[a] = v[2][a];
        r.lo[a] = (float)((double)fminf(fminf(v[0][a], v[1][a]), v[2][a]) - e);
        r.hi[a] = (float)((double)fmaxf(fmaxf(v[0][a], v[1][a]), v[2][a]) + e);
    }
    // the plane in double; a sliver whose normal is below 2^-20 |ab| |ac| gets no plane test
    double ab[3], ac[3];
    for (int a = 0; a < 3; ++a) { ab[a] = (double)v[1][a] - (double)v[0][a]; ac[a] = (double)v[2][a] - (double)v[0][a]; }
    const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
    const double l2 = cx * cx + cy * cy + cz * cz;
    const double s2 = (ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]) * (ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]);
    r.nrm[0] = r.nrm[1] = r.nrm[2] = 0.0f; r.k = 0.0f; r.bp = __builtin_inff();
    if (l2 > 0.0 && __builtin_isfinite(l2) && __builtin_isfinite(s2) && l2 >= s2 * (1.0 / 1099511627776.0)) {
        const double il = 1.0 / sqrt(l2);
        const double n0 = cx * il, n1 = cy * il, n2 = cz * il;
        r.nrm[0] = (float)n0; r.nrm[1] = (float)n1; r.nrm[2] = (float)n2;
        r.k = (float)(n0 * (double)v[0][0] + n1 * (double)v[0][1] + n2 * (double)v[0][2]);
        r.bp = (float)((double)bn.bm + (double)fmaxf(mt, bn.mp) * (1.0 / 65536.0));      // + 2^-16 M: twice what the argument needs
    }
    r.idx = (uint32_t)t; r.pad = 0;
    const float o[3] = {f.ox, f.oy, f.oz};
    for (int a = 0; a < 3; ++a)
        if (!centre_range((double)r.lo[a] - bn.bd, (double)r.hi[a] + bn.bd, o[a], f.vs, (int)f.n, vl[a], vh[a])) return false;
    r.bxy = (uint32_t)(vl[0] >> 3) | ((uint32_t)(vh[0] >> 3) << 8) | ((uint32_t)(vl[1] >> 3) << 16) | ((uint32_t)(vh[1] >> 3) << 24);
    r.bz = (uint32_t)(vl[2] >> 3) | ((uint32_t)(vh[2] >> 3) << 8);
    return true;
}

__device__ __forceinline__ uint32_t rec_rows(const MRec& r)
{
    if (r.idx == kNoTri) return 0u;
    return (((r.bxy >> 24) & 0xFFu) - ((r.bxy >> 16) & 0xFFu) + 1u) * (((r.bz >> 8) & 0xFFu) - (r.bz & 0xFFu) + 1u);
}

// ---- NAIVE ------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
md_prefill(unsigned long long* __restrict__ keys, size_t voxels, unsigned long long v)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < voxels; i += stride) keys[i] = v;
}

__global__ void __launch_bounds__(256)
md_naive(Frame f, Band bn, const float* __restrict__ xyz, size_t nverts, const uint32_t* __restrict__ tri, size_t ntris,
         unsigned long long* __restrict__ keys)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    MRec r;
    int vl[3], vh[3];
    if (!mtri_setup(f, bn, xyz, nverts, tri, t, r, vl, vh)) return;
    for (int z = vl[2]; z <= vh[2]; ++z)
        for (int y = vl[1]; y <= vh[1]; ++y)
            for (int x = vl[0]; x <= vh[0]; ++x) {
                const float p[3] = {centre(f.ox, x, f.vs), centre(f.oy, y, f.vs), centre(f.oz, z, f.vs)};
                if (pair_out(p, r.lo, r.hi, r.nrm, r.k, r.bp, bn.b2c)) continue;
                const float d = tri_d2(p, r.a, r.b, r.c);
                if (!(d < bn.b2)) continue;                                       // NaN and infinity fail as well
                atomicMin(&keys[(size_t)x + (size_t)f.n * ((size_t)y + (size_t)f.n * (size_t)z)],
                          ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(uint32_t)t);
            }
}

__device__ __forceinline__ bool sign_bit(const uint32_t* __restrict__ words, size_t i) { return (words[i >> 5] >> (i & 31)) & 1u; }

__global__ void __launch_bounds__(256)
md_split(const unsigned long long* __restrict__ keys, size_t voxels, const uint32_t* __restrict__ words, float* __restrict__ dist,
         uint32_t* __restrict__ nearest)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < voxels; i += stride) {
        const unsigned long long k = keys[i];
        const float m = __uint_as_float((uint32_t)(k >> 32));
        dist[i] = (!words || sign_bit(words, i)) ? m : -m;
        if (nearest) nearest[i] = (uint32_t)k;
    }
}

// ---- TILED ------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
md_setup(Frame f, Band bn, const float* __restrict__ xyz, size_t nverts, const uint32_t* __restrict__ tri, size_t ntris, MRec* __restrict__ rec,
         uint32_t* __restrict__ rows)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    MRec r = {};
    int vl[3], vh[3];
    if (!mtri_setup(f, bn, xyz, nverts, tri, t, r, vl, vh)) { r.idx = kNoTri; r.bxy = 0u; r.bz = 0u; r.pad = 0u; }
    rec[t] = r;
    rows[t] = rec_rows(r);                                        // compact, for the scan
}

// One workgroup: base[t] = brick rows of the triangles before t (64-bit), base[ntris] = all of them.
__global__ void __launch_bounds__(1024)
md_scan(const uint32_t* __restrict__ rows, size_t ntris, unsigned long long* __restrict__ base)
{
    __shared__ unsigned long long part[1024];
    const unsigned long long total = wg_scan_1024(part, (unsigned long long)ntris, [&](unsigned long long i) { return (unsigned long long)rows[i]; },
                                                  [&](unsigned long long i, unsigned long long before) { base[i] = before; });
    if (threadIdx.x == 1023) base[ntris] = total;
}

// the two lower bounds over all the centres of one brick, in double: true = no voxel of the brick can take this triangle
__device__ __forceinline__ bool brick_out(const Frame& f, const Band& bn, const MRec& r, int bx, int by, int bz)
{
    const float o[3] = {f.ox, f.oy, f.oz};
    const int b[3] = {bx, by, bz};
    double g2 = 0.0, sc = -(double)r.k, rad = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double c0 = (double)centre(o[a], b[a] * 8, f.vs), c1 = (double)centre(o[a], b[a] * 8 + 7, f.vs);
        const double g = fmax(fmax((double)r.lo[a] - c1, c0 - (double)r.hi[a]), 0.0);
        g2 += g * g;
        sc += (double)r.nrm[a] * (0.5 * (c0 + c1));
        rad += fabs((double)r.nrm[a]) * (0.5 * (c1 - c0));
    }
    if (g2 > (double)bn.b2c * (1.0 + 1e-9)) return true;
    return fabs(sc) - rad > (double)r.bp;
}

// One lane per (triangle, brick row), grid-stride over all of them; the lane walks the bricks of its row along x.
// WRITE = false: cnt[brick] += 1 per passing brick; true: the triangle goes into the brick's list at off[brick] - off0 + cur[brick]++.
template <bool WRITE>
__global__ void __launch_bounds__(256)
md_bin(Frame f, Band bn, const MRec* __restrict__ rec, size_t ntris, const unsigned long long* __restrict__ base, int zlo, int zhi,
       uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ off, unsigned long long off0, uint32_t* __restrict__ list)
{
    const unsigned long long total = base[ntris];
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const int nb = (int)f.n / 8;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
        size_t lo = 0, hi = ntris - 1;                             // the last triangle whose base is <= q: it has rows
        while (lo < hi) {
            const size_t mid = (lo + hi + 1) >> 1;
            if (base[mid] <= q) lo = mid; else hi = mid - 1;
        }
        const MRec& r = rec[lo];
        const uint32_t k = (uint32_t)(q - base[lo]);
        const int bx0 = (int)(r.bxy & 0xFFu), bx1 = (int)((r.bxy >> 8) & 0xFFu), by0 = (int)((r.bxy >> 16) & 0xFFu), by1 = (int)(r.bxy >> 24);
        const int ny = by1 - by0 + 1;
        const int by = by0 + (int)(k % (uint32_t)ny), bz = (int)(r.bz & 0xFFu) + (int)(k / (uint32_t)ny);
        if (bz < zlo || bz > zhi) continue;
        for (int bx = bx0; bx <= bx1; ++bx) {
            if (brick_out(f, bn, r, bx, by, bz)) continue;
            const size_t brick = (size_t)bx + (size_t)nb * ((size_t)by + (size_t)nb * (size_t)bz);
            const uint32_t slot = atomicAdd(&cnt[brick], 1u);
            if (WRITE) list[off[brick] - off0 + slot] = r.idx;
        }
    }
}

// sums[bz] = list entries of the bricks of plane bz
__global__ void __launch_bounds__(256)
md_plane_sums(const uint32_t* __restrict__ cnt, uint32_t per_plane, unsigned long long* __restrict__ sums)
{
    __shared__ unsigned long long smem[4];
    unsigned long long s = 0;
    for (uint32_t i = threadIdx.x; i < per_plane; i += 256) s += cnt[(size_t)blockIdx.x * per_plane + i];
    s = wg_sum_256(s, smem);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// One workgroup: off[i] = start + list entries of the bricks [first, i), for the m bricks from `first` on
__global__ void __launch_bounds__(1024)
md_offsets(const uint32_t* __restrict__ cnt, uint32_t first, uint32_t m, unsigned long long start, unsigned long long* __restrict__ off)
{
    __shared__ unsigned long long part[1024];
    wg_scan_1024(part, m, [&](uint32_t i) { return (unsigned long long)cnt[first + i]; },
                 [&](uint32_t i, unsigned long long before) { off[first + i] = start + before; });
}

// One workgroup per brick of [brick0, brick0 + gridDim.x).  Lane t owns the voxels (t & 7, (t >> 3) & 7, t >> 6) and the one four planes up.
__global__ void __launch_bounds__(256)
md_brick(Frame f, Band bn, const uint32_t* __restrict__ words, const MRec* __restrict__ rec, const uint32_t* __restrict__ list,
         const unsigned long long* __restrict__ off, unsigned long long off0, const uint32_t* __restrict__ cnt, uint32_t brick0,
         float* __restrict__ dist, uint32_t* __restrict__ nearest)
{
    __shared__ uint4 srec[kBatch * kRecU4];
    const uint32_t brick = brick0 + blockIdx.x;
    const uint32_t m = cnt[brick];
    if (!m) return;                                                // md_fill writes this brick
    const uint32_t nb = f.n / 8;
    const int t = (int)threadIdx.x;
    const int x = (int)(brick % nb) * 8 + (t & 7), y = (int)((brick / nb) % nb) * 8 + ((t >> 3) & 7), z = (int)(brick / (nb * nb)) * 8 + (t >> 6);
    const float p0[3] = {centre(f.ox, x, f.vs), centre(f.oy, y, f.vs), centre(f.oz, z, f.vs)};
    const float p1[3] = {p0[0], p0[1], centre(f.oz, z + 4, f.vs)};
    float d0 = bn.b2, d1 = bn.b2;
    uint32_t i0 = kNoTri, i1 = kNoTri;
    const uint32_t* mine = list + (off[brick] - off0);
    const uint4* rec4 = reinterpret_cast<const uint4*>(rec);
    for (uint32_t b = 0; b < m; b += kBatch) {
        const uint32_t nrec = min((uint32_t)kBatch, m - b);
        __syncthreads();                                           // the previous batch has been read
        for (uint32_t j = (uint32_t)t; j < nrec * kRecU4; j += 256)
            srec[j] = rec4[(size_t)mine[b + j / kRecU4] * kRecU4 + j % kRecU4];
        __syncthreads();
        for (uint32_t j = 0; j < nrec; ++j) {
            const MRec& r = *reinterpret_cast<const MRec*>(&srec[j * kRecU4]);
            if (!pair_out(p0, r.lo, r.hi, r.nrm, r.k, r.bp, bn.b2c)) {
                const float d = tri_d2(p0, r.a, r.b, r.c);
                if (d < bn.b2 && (d < d0 || (d == d0 && r.idx < i0))) { d0 = d; i0 = r.idx; }
            }
            if (!pair_out(p1, r.lo, r.hi, r.nrm, r.k, r.bp, bn.b2c)) {
                const float d = tri_d2(p1, r.a, r.b, r.c);
                if (d < bn.b2 && (d < d1 || (d == d1 && r.idx < i1))) { d1 = d; i1 = r.idx; }
            }
        }
    }
    const size_t v0 = (size_t)x + (size_t)f.n * ((size_t)y + (size_t)f.n * (size_t)z), v1 = v0 + (size_t)4 * f.n * f.n;
    dist[v0] = (!words || sign_bit(words, v0)) ? d0 : -d0;
    dist[v1] = (!words || sign_bit(words, v1)) ? d1 : -d1;
    if (nearest) { nearest[v0] = i0; nearest[v1] = i1; }
}

// Streaming fill: four voxels of one x row per lane (they share a brick); bricks with a list are md_brick's.  cnt = nullptr: every brick.
__global__ void __launch_bounds__(256)
md_fill(Frame f, float b2, const uint32_t* __restrict__ words, const uint32_t* __restrict__ cnt, float4* __restrict__ dist, uint4* __restrict__ nearest)
{
    const size_t n = f.n, quads = n * n * n / 4, stride = (size_t)gridDim.x * 256;
    const size_t nb = n / 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += stride) {
        const size_t v = i * 4, x = v % n, y = (v / n) % n, z = v / (n * n);
        if (cnt && cnt[(x >> 3) + nb * ((y >> 3) + nb * (z >> 3))]) continue;
        float s[4];
        const uint32_t w = words ? (words[v >> 5] >> (v & 31)) : 0xFu;
        for (int k = 0; k < 4; ++k) s[k] = ((w >> k) & 1u) ? b2 : -b2;
        dist[i] = make_float4(s[0], s[1], s[2], s[3]);
        if (nearest) nearest[i] = make_uint4(kNoTri, kNoTri, kNoTri, kNoTri);
    }
}

Band make_band(const Frame& f, uint32_t band)
{
    Band bn;
    const float B = (float)band * f.vs;
    bn.b2 = B * B;
    const float up = 1.0f + 1.0f / 262144.0f;                                  // 1 + 2^-18, exact in float
    bn.b2c = std::nextafter((float)((double)bn.b2 * (double)up), INFINITY);
    bn.bm = std::nextafter((float)((double)B * (double)up), INFINITY);
    bn.bd = std::sqrt((double)bn.b2c);
    float mp = 0.0f;
    const float o[3] = {f.ox, f.oy, f.oz};
    for (int a = 0; a < 3; ++a) mp = std::max(mp, std::max(std::fabs(o[a]), std::fabs(o[a] + (float)f.n * f.vs)));
    bn.mp = mp;
    return bn;
}

}  // namespace

int launch_mesh_distance(vp_ctx* ctx, const Frame& f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris,
                         const uint32_t* d_sign, uint32_t band, float* d_dist, uint32_t* d_nearest, int algo)
{
    hipStream_t st = ctx->stream;
    const Band bn = make_band(f, band);
    const size_t voxels = (size_t)f.n * f.n * f.n;
    const unsigned sblocks = (unsigned)std::min<size_t>((voxels / 4 + 255) / 256, (size_t)ctx->cus * 16);
    const unsigned tblocks = (unsigned)((ntris + 255) / 256);

    if (!ntris) {                                                  // s B2 / NONE everywhere
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(md_fill, dim3(sblocks), dim3(256), 0, st, f, bn.b2, d_sign, (const uint32_t*)nullptr, (float4*)d_dist, (uint4*)d_nearest);
        VP_HIP(hipGetLastError());
        return 0;
    }

    if (algo == VP_ALGO_NAIVE) {
        VP_TRY(reserve(ctx, ctx->md.keys, voxels * 8, false));
        unsigned long long* keys = (unsigned long long*)ctx->md.keys.ptr;
        uint32_t b2bits;
        memcpy(&b2bits, &bn.b2, 4);
        {
            ProfScope p(ctx, VP_K_MD_PREFILL);
            hipLaunchKernelGGL(md_prefill, dim3(sblocks), dim3(256), 0, st, keys, voxels, ((unsigned long long)b2bits << 32) | (unsigned long long)kNoTri);
        }
        {
            ProfScope p(ctx, VP_K_MD_NAIVE);
            hipLaunchKernelGGL(md_naive, dim3(tblocks), dim3(256), 0, st, f, bn, d_xyz, nverts, d_tri, ntris, keys);
        }
        {
            ProfScope p(ctx, VP_K_MD_SPLIT);
            hipLaunchKernelGGL(md_split, dim3(sblocks), dim3(256), 0, st, (const unsigned long long*)keys, voxels, d_sign, d_dist, d_nearest);
        }
        VP_HIP(hipGetLastError());
        return 0;
    }

    // ---- TILED ----
    const uint32_t nb = f.n / 8, per_plane = nb * nb, bricks = per_plane * nb;
    VP_TRY(reserve(ctx, ctx->md.rec, ntris * sizeof(MRec)));
    VP_TRY(reserve(ctx, ctx->md.base, (ntris + 1) * 8 + ntris * 4));            // the row scan, then the row counts
    VP_TRY(reserve(ctx, ctx->md.cnt, (size_t)bricks * 8 + (size_t)nb * 8));         // counts, write cursors, plane sums
    VP_TRY(reserve(ctx, ctx->md.off, (size_t)bricks * 8));
    VP_TRY(ctx->md.host.need(128));
    MRec* rec = (MRec*)ctx->md.rec.ptr;
    unsigned long long* base = (unsigned long long*)ctx->md.base.ptr;
    uint32_t* rows = (uint32_t*)(base + ntris + 1);
    unsigned long long* sums = (unsigned long long*)ctx->md.cnt.ptr;                 // 8-byte aligned at the front
    uint32_t* cnt = (uint32_t*)(sums + nb);
    uint32_t* cur = cnt + bricks;
    unsigned long long* off = (unsigned long long*)ctx->md.off.ptr;
    const unsigned bblocks = (unsigned)ctx->cus * 8u;

    VP_HIP(hipMemsetAsync(cnt, 0, (size_t)bricks * 8, st));
    {
        ProfScope p(ctx, VP_K_MD_SETUP);
        hipLaunchKernelGGL(md_setup, dim3(tblocks), dim3(256), 0, st, f, bn, d_xyz, nverts, d_tri, ntris, rec, rows);
    }
    {
        ProfScope p(ctx, VP_K_MD_SCAN);
        hipLaunchKernelGGL(md_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)rows, ntris, base);
    }
    {
        ProfScope p(ctx, VP_K_MD_COUNT);
        hipLaunchKernelGGL(md_bin<false>, dim3(bblocks), dim3(256), 0, st, f, bn, (const MRec*)rec, ntris, (const unsigned long long*)base, 0, (int)nb - 1,
                           cnt, (const unsigned long long*)nullptr, 0ull, (uint32_t*)nullptr);
        hipLaunchKernelGGL(md_plane_sums, dim3(nb), dim3(256), 0, st, (const uint32_t*)cnt, per_plane, sums);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->md.host, sums, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));                              // the one read-back: the plane totals size the lists

    uint64_t cap = kListCap;
#ifdef VP_TEST_HOOKS   // test builds only (libvphip_hooks.so): force the z ranges
    if (const char* e = getenv("VP_MESHDIST_LIST_CAP")) cap = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
#endif
    // z ranges of brick planes whose lists fit the cap (a single plane above the cap is a range of its own)
    uint64_t longest = 0, total = 0;
    for (uint32_t z = 0; z < nb;) {
        uint64_t s = ctx->md.host[z];
        uint32_t e = z + 1;
        while (e < nb && s + ctx->md.host[e] <= cap) s += ctx->md.host[e++];
        longest = std::max(longest, s);
        total += s;
        z = e;
    }
    ctx->md.last_total = total;
    VP_TRY(reserve(ctx, ctx->md.list, std::max<uint64_t>(longest, 4) * 4));
    uint32_t* list = (uint32_t*)ctx->md.list.ptr;
    for (uint32_t z = 0; z < nb;) {
        uint64_t s = ctx->md.host[z];
        uint32_t e = z + 1;
        while (e < nb && s + ctx->md.host[e] <= cap) s += ctx->md.host[e++];
        if (s) {
            const uint32_t first = z * per_plane, m = (e - z) * per_plane;
            {
                ProfScope p(ctx, VP_K_MD_SCAN);
                hipLaunchKernelGGL(md_offsets, dim3(1), dim3(1024), 0, st, (const uint32_t*)cnt, first, m, 0ull, off);
            }
            {
                ProfScope p(ctx, VP_K_MD_WRITE);
                hipLaunchKernelGGL(md_bin<true>, dim3(bblocks), dim3(256), 0, st, f, bn, (const MRec*)rec, ntris, (const unsigned long long*)base, (int)z,
                                   (int)e - 1, cur, (const unsigned long long*)off, 0ull, list);
            }
            {
                ProfScope p(ctx, VP_K_MD_BRICK);
                hipLaunchKernelGGL(md_brick, dim3(m), dim3(256), 0, st, f, bn, d_sign, (const MRec*)rec, (const uint32_t*)list,
                                   (const unsigned long long*)off, 0ull, (const uint32_t*)cnt, first, d_dist, d_nearest);
            }
        }
        z = e;
    }
    {
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(md_fill, dim3(sblocks), dim3(256), 0, st, f, bn.b2, d_sign, (const uint32_t*)cnt, (float4*)d_dist, (uint4*)d_nearest);
    }
    VP_HIP(hipGetLastError());
    return 0;
}

}  // namespace vp
