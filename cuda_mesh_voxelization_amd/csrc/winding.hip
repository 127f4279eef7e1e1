// winding.hip -- generalized winding number of a triangle mesh at the voxel centres, and its inside grid, for gfx950 (MI355X).
//
// w(p) = (1 / 4 pi) sum of the signed solid angles of the triangles seen from p (Jacobson et al. 2013), with the dipole far field of
// Barill et al. 2018 over a pyramid of 8 x 8 x 8-voxel bricks.  The contract is in include/vphip.h (vp_winding) and DESIGN.md section 17:
// every term is one fixed float32 expression, quantised to a 64-bit integer before it is added, so the sum does not depend on the order
// of the triangles, on atomics or on how a list was built; which terms exist is decided per (brick of voxels, node) by a float32 test
// that is part of the contract.  This file, the host restatement (vplib/src/winding.cpp) and the tests' numpy restatement agree bit for bit.
//
// Setup (both algos; nothing is read back):
//   wn_setup   one thread per triangle: validity, the leaf that holds the centroid, the leaf's count (+1), its box (integer-ordered float
//              min / max by atomicMax) and its area vector (three 64-bit adds of the quantised components)
//   wn_scan    exclusive scan of the leaf counts (one workgroup, wg_scan.h)
//   wn_write   one thread per triangle: its nine coordinates into its leaf's run of the record array (any order inside a leaf)
//   wn_reduce  one launch per level: a node's count, box and area vector from its up to eight children
//   wn_nodes   every node of every level: centre, radius, the area vector as float32 and the mask of its non-empty children -- the 32-byte
//              record the walks read
// TILED: wn_brick -- one workgroup per brick, lane t owns voxel (t & 7, (t >> 3) & 7, t >> 6) and the one four planes up.  The walk of the
//        pyramid is the same for the whole workgroup (stackless, over the non-empty nodes only: level, node coordinates and one 64-bit word of
//        pending siblings, all scalar); node records are broadcast loads; the
//        records of a near leaf go through LDS 64 at a time; two 64-bit accumulators per lane (unsigned: the sum is defined for any
//        number of triangles); one store of w per voxel, the inside bits by ballot (one byte per x row of the brick).
// NAIVE: wn_naive -- one thread per voxel walks the same pyramid from global memory on its own; the inside words by ballot.
// wn_count (only when the caller asks for the number of inside voxels): popcount of the grid, one add per workgroup.
#include "vp_internal.h"
#include "wg_scan.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace vp {

namespace {

constexpr uint32_t kNoLeaf = 0xFFFFFFFFu;
constexpr int kBatch = 64;                      // records per LDS batch
constexpr int kRecU4 = 3;                       // record: a, b, c and three pad words = 12 dwords; a batch is 3 KiB of LDS
constexpr int kMaxLevels = 8;                   // n = 1024: 128, 64, 32, 16, 8, 4, 2, 1

struct WNode {
    float c[3], r;                              // centre and radius of the box of the node's triangles
    float nv[3];                                // area vector
    uint32_t mask;                              // bit 8: the node has triangles (0: it contributes nothing); bits 0 .. 7: its non-empty children
};
static_assert(sizeof(WNode) == 32, "node layout");

struct Pyr {
    uint32_t nb, levels;                        // bricks per side, levels (level 0 = the leaves, levels - 1 = the root)
    uint32_t off[kMaxLevels + 1];               // first node of a level; off[levels] = all nodes
};

__host__ __device__ __forceinline__ uint32_t level_dim(uint32_t nb, int k) { return (nb + (1u << k) - 1u) >> k; }

__device__ __forceinline__ float centre(float o, int i, float vs) { return o + (((float)i * vs) + (vs / 2.0f)); }
__device__ __forceinline__ float dot3(const float* a, const float* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }
__device__ __forceinline__ float sel_max(float a, float b) { return a > b ? a : b; }

// the integer order of floats: -inf < ... < -0 < +0 < ... < +inf as unsigned
__device__ __forceinline__ uint32_t ord(float v) { const uint32_t b = __float_as_uint(v); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ float unord(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// atan2 of the contract: the header's odd polynomial on [0, 1] and the octant fix-ups.  x and y finite, not both zero.
__device__ __forceinline__ float wn_atan2(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const float t = fminf(ax, ay) / fmaxf(ax, ay);
    const float s = t * t;
    float p = VP_WN_ATAN_C9;
    p = (p * s) + VP_WN_ATAN_C8; p = (p * s) + VP_WN_ATAN_C7; p = (p * s) + VP_WN_ATAN_C6;
    p = (p * s) + VP_WN_ATAN_C5; p = (p * s) + VP_WN_ATAN_C4; p = (p * s) + VP_WN_ATAN_C3;
    p = (p * s) + VP_WN_ATAN_C2; p = (p * s) + VP_WN_ATAN_C1; p = (p * s) + VP_WN_ATAN_C0;
    float r = p * t;
    r = ay > ax ? VP_WN_HALF_PI - r : r;
    r = x < 0.0f ? VP_WN_PI - r : r;
    return y < 0.0f ? -r : r;
}

// a term as it is added: two's complement in 64 bits, so the sums wrap modulo 2^64 like the area sums (defined in every form)
__device__ __forceinline__ unsigned long long quantise(float omega) { return (unsigned long long)__double2ll_rn((double)omega * 68719476736.0); }   // 2^36

// exact term: the quantised solid angle of triangle (A, B, C) seen from p
__device__ __forceinline__ unsigned long long exact_term(const float* p, const float* A, const float* B, const float* C)
{
    float a[3], b[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a[i] = A[i] - p[i]; b[i] = B[i] - p[i]; c[i] = C[i] - p[i]; }
    const float la = sqrtf(dot3(a, a)), lb = sqrtf(dot3(b, b)), lc = sqrtf(dot3(c, c));
    const float x[3] = {(b[1] * c[2]) - (b[2] * c[1]), (b[2] * c[0]) - (b[0] * c[2]), (b[0] * c[1]) - (b[1] * c[0])};
    const float det = dot3(a, x);
    const float den = ((((la * lb) * lc) + (dot3(a, b) * lc)) + (dot3(b, c) * la)) + (dot3(c, a) * lb);
    const bool ok = det != 0.0f && finite_f(det) && finite_f(den);
    const float om = 2.0f * wn_atan2(det, den);
    return quantise(ok ? om : 0.0f);
}

// far term: the dipole of a node seen from p
__device__ __forceinline__ unsigned long long far_term(const float* p, const WNode& nd)
{
    const float d[3] = {nd.c[0] - p[0], nd.c[1] - p[1], nd.c[2] - p[2]};
    const float r2 = dot3(d, d);
    const float om = dot3(d, nd.nv) / (r2 * sqrtf(r2));
    return quantise(finite_f(om) ? om : 0.0f);
}

// the far test of a (brick, node) pair: blo / bhi = the centres of the brick's first and last voxel
__device__ __forceinline__ bool node_far(const float* blo, const float* bhi, const WNode& nd, float beta)
{
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = sel_max(0.0f, sel_max(blo[a] - nd.c[a], nd.c[a] - bhi[a]));
    const float br = beta * nd.r;
    return dot3(g, g) > br * br && beta > 0.0f;
}

// Stackless walk over the non-empty nodes only.  `pending` holds, per level k in byte k, the non-empty children of the current ancestor at
// level k + 1 that are still to be visited (eight levels at the most: 64 bits).
// walk_down: from a node with children mask m to its first non-empty child, the others noted as pending.
__device__ __forceinline__ void walk_down(uint32_t m, int& k, uint32_t& x, uint32_t& y, uint32_t& z, unsigned long long& pending)
{
    const uint32_t j = (uint32_t)__ffs((int)m) - 1u;               // m != 0: a node with triangles has a child with triangles
    --k;
    pending = (pending & ~(0xFFull << (8 * k))) | ((unsigned long long)(m & (m - 1u)) << (8 * k));
    x = 2u * x + (j & 1u); y = 2u * y + ((j >> 1) & 1u); z = 2u * z + (j >> 2);
}
// walk_next: the node after (k, x, y, z) when that node is done with -- its next pending sibling, else the one after its parent.  false: the
// root is done.
__device__ __forceinline__ bool walk_next(const Pyr& py, int& k, uint32_t& x, uint32_t& y, uint32_t& z, unsigned long long& pending)
{
    while (k < (int)py.levels - 1) {
        const uint32_t m = (uint32_t)(pending >> (8 * k)) & 0xFFu;
        if (m) {
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
            pending &= ~(1ull << (8 * k + (int)j));
            x = (x & ~1u) | (j & 1u); y = (y & ~1u) | ((j >> 1) & 1u); z = (z & ~1u) | (j >> 2);
            return true;
        }
        x >>= 1; y >>= 1; z >>= 1; ++k;
    }
    return false;
}

__device__ __forceinline__ float final_w(unsigned long long s) { return (float)(((double)(long long)s * (1.0 / 68719476736.0)) / VP_WN_FOUR_PI); }

// ---- setup ------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ long long quantise_area(float nrm, double u)
{
    double s = ((double)nrm * 8388608.0) / u;                      // (nrm / 2) in units of vs^2 2^-24
    s = s > 4611686018427387904.0 ? 4611686018427387904.0 : s;
    s = s < -4611686018427387904.0 ? -4611686018427387904.0 : s;
    s = s != s ? 0.0 : s;
    return __double2ll_rn(s);
}

__global__ void __launch_bounds__(256)
wn_setup(Frame f, uint32_t nb, const float* __restrict__ xyz, size_t nverts, const uint32_t* __restrict__ tri, size_t ntris,
         uint32_t* __restrict__ key, uint32_t* __restrict__ count, uint32_t* __restrict__ box, unsigned long long* __restrict__ sum)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    key[t] = kNoLeaf;
    const uint32_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (id[0] >= nverts || id[1] >= nverts || id[2] >= nverts) return;
    float v[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            v[k][a] = xyz[3 * (size_t)id[k] + a];
            if (!finite_f(v[k][a])) return;
        }
    float e0[3], e1[3];
    for (int a = 0; a < 3; ++a) { e0[a] = v[1][a] - v[0][a]; e1[a] = v[2][a] - v[1][a]; }
    const float nrm[3] = {(e0[1] * e1[2]) - (e0[2] * e1[1]), (e0[2] * e1[0]) - (e0[0] * e1[2]), (e0[0] * e1[1]) - (e0[1] * e1[0])};
    if (nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f) return;
    const float o[3] = {f.ox, f.oy, f.oz};
    uint32_t b[3];
    for (int a = 0; a < 3; ++a) {
        const float g = ((v[0][a] + v[1][a]) + v[2][a]) / 3.0f;
        const float q = floorf(((g - o[a]) / f.vs) / 8.0f);
        b[a] = q >= (float)(nb - 1u) ? nb - 1u : (q > 0.0f ? (uint32_t)q : 0u);
    }
    const uint32_t leaf = b[0] + nb * (b[1] + nb * b[2]);
    key[t] = leaf;
    atomicAdd(&count[leaf], 1u);
    const double u = (double)f.vs * (double)f.vs;
    for (int a = 0; a < 3; ++a) {
        const uint32_t k0 = ord(v[0][a]), k1 = ord(v[1][a]), k2 = ord(v[2][a]);     // min and max in the integer order: -0 < +0
        atomicMax(&box[6 * (size_t)leaf + a], ~min(min(k0, k1), k2));
        atomicMax(&box[6 * (size_t)leaf + 3 + a], max(max(k0, k1), k2));
        atomicAdd(&sum[3 * (size_t)leaf + a], (unsigned long long)quantise_area(nrm[a], u));
    }
}

__global__ void __launch_bounds__(1024)
wn_scan(const uint32_t* __restrict__ count, uint32_t nleaves, uint32_t* __restrict__ leaf_off)
{
    __shared__ uint32_t part[1024];
    const uint32_t total = wg_scan_1024(part, nleaves, [&](uint32_t i) { return count[i]; }, [&](uint32_t i, uint32_t before) { leaf_off[i] = before; });
    if (threadIdx.x == 1023) leaf_off[nleaves] = total;
}

__global__ void __launch_bounds__(256)
wn_write(const float* __restrict__ xyz, const uint32_t* __restrict__ tri, size_t ntris, const uint32_t* __restrict__ key,
         const uint32_t* __restrict__ leaf_off, uint32_t* __restrict__ cur, float4* __restrict__ rec)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    const uint32_t leaf = key[t];
    if (leaf == kNoLeaf) return;
    const size_t slot = (size_t)leaf_off[leaf] + atomicAdd(&cur[leaf], 1u);
    const float* a = xyz + 3 * (size_t)tri[3 * t];
    const float* b = xyz + 3 * (size_t)tri[3 * t + 1];
    const float* c = xyz + 3 * (size_t)tri[3 * t + 2];
    rec[slot * kRecU4] = make_float4(a[0], a[1], a[2], b[0]);
    rec[slot * kRecU4 + 1] = make_float4(b[1], b[2], c[0], c[1]);
    rec[slot * kRecU4 + 2] = make_float4(c[2], 0.0f, 0.0f, 0.0f);
}

// level k + 1 from level k: one thread per node of the upper level
__global__ void __launch_bounds__(256)
wn_reduce(uint32_t dim_lo, uint32_t dim_up, uint32_t off_lo, uint32_t off_up, uint32_t* __restrict__ count, uint32_t* __restrict__ box,
          unsigned long long* __restrict__ sum)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= dim_up * dim_up * dim_up) return;
    const uint32_t x = i % dim_up, y = (i / dim_up) % dim_up, z = i / (dim_up * dim_up);
    uint32_t cnt = 0u, bx[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    unsigned long long s[3] = {0ull, 0ull, 0ull};
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t cx = 2u * x + (j & 1u), cy = 2u * y + ((j >> 1) & 1u), cz = 2u * z + (j >> 2);
        if (cx >= dim_lo || cy >= dim_lo || cz >= dim_lo) continue;
        const size_t c = (size_t)off_lo + cx + dim_lo * (cy + (size_t)dim_lo * cz);
        cnt += count[c];
        for (int a = 0; a < 6; ++a) bx[a] = max(bx[a], box[6 * c + a]);
        for (int a = 0; a < 3; ++a) s[a] += sum[3 * c + a];
    }
    const size_t me = (size_t)off_up + i;
    count[me] = cnt;
    for (int a = 0; a < 6; ++a) box[6 * me + a] = bx[a];
    for (int a = 0; a < 3; ++a) sum[3 * me + a] = s[a];
}

__global__ void __launch_bounds__(256)
wn_nodes(float vs, Pyr py, const uint32_t* __restrict__ count, const uint32_t* __restrict__ box, const unsigned long long* __restrict__ sum,
         WNode* __restrict__ nodes)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= py.off[py.levels]) return;
    WNode nd = {};
    if (count[i]) {
        nd.mask = 0x100u;
        int k = 0;
        while (i >= py.off[k + 1]) ++k;
        if (k > 0) {                                               // the non-empty children, inside the side of the level below
            const uint32_t d = level_dim(py.nb, k), dl = level_dim(py.nb, k - 1), at = i - py.off[k];
            const uint32_t x = at % d, y = (at / d) % d, z = at / (d * d);
            for (uint32_t j = 0; j < 8u; ++j) {
                const uint32_t cx = 2u * x + (j & 1u), cy = 2u * y + ((j >> 1) & 1u), cz = 2u * z + (j >> 2);
                if (cx < dl && cy < dl && cz < dl && count[py.off[k - 1] + cx + dl * (cy + dl * cz)]) nd.mask |= 1u << j;
            }
        }
        const double unit = ((double)vs * (double)vs) * (1.0 / 16777216.0);
        float h[3];
        for (int a = 0; a < 3; ++a) {
            const float lo = unord(~box[6 * (size_t)i + a]), hi = unord(box[6 * (size_t)i + 3 + a]);
            h[a] = (hi - lo) / 2.0f;
            nd.c[a] = lo + h[a];
            nd.nv[a] = (float)((double)(long long)sum[3 * (size_t)i + a] * unit);
        }
        nd.r = sqrtf(dot3(h, h));
    }
    nodes[i] = nd;
}

// ---- NAIVE ------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
wn_naive(Frame f, Pyr py, float beta, float level, const WNode* __restrict__ nodes, const uint32_t* __restrict__ leaf_off,
         const float4* __restrict__ rec, float* __restrict__ w, uint32_t* __restrict__ inside)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;       // n^3 is a multiple of 256
    const uint32_t n = f.n;
    const int x = (int)(i % n), y = (int)((i / n) % n), z = (int)(i / ((size_t)n * n));
    const float p[3] = {centre(f.ox, x, f.vs), centre(f.oy, y, f.vs), centre(f.oz, z, f.vs)};
    const float blo[3] = {centre(f.ox, x & ~7, f.vs), centre(f.oy, y & ~7, f.vs), centre(f.oz, z & ~7, f.vs)};
    const float bhi[3] = {centre(f.ox, x | 7, f.vs), centre(f.oy, y | 7, f.vs), centre(f.oz, z | 7, f.vs)};
    unsigned long long acc = 0;
    int k = (int)py.levels - 1;
    uint32_t nx = 0u, ny = 0u, nz = 0u;
    unsigned long long pending = 0ull;
    for (;;) {
        const uint32_t dim = level_dim(py.nb, k);
        const uint32_t at = nx + dim * (ny + dim * nz);
        const WNode nd = nodes[py.off[k] + at];
        bool down = false;
        if (nd.mask) {
            if (node_far(blo, bhi, nd, beta)) acc += far_term(p, nd);
            else if (k == 0) {
                for (uint32_t j = leaf_off[at]; j < leaf_off[at + 1]; ++j) {
                    const float4 r0 = rec[(size_t)j * kRecU4], r1 = rec[(size_t)j * kRecU4 + 1], r2 = rec[(size_t)j * kRecU4 + 2];
                    const float A[3] = {r0.x, r0.y, r0.z}, B[3] = {r0.w, r1.x, r1.y}, C[3] = {r1.z, r1.w, r2.x};
                    acc += exact_term(p, A, B, C);
                }
            } else down = true;
        }
        if (down) walk_down(nd.mask & 0xFFu, k, nx, ny, nz, pending);
        else if (!walk_next(py, k, nx, ny, nz, pending)) break;
    }
    const float wv = final_w(acc);
    w[i] = wv;
    const unsigned long long bits = __ballot(wv >= level);         // 64 consecutive voxels: two words
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0u) inside[i >> 5] = (uint32_t)bits;
    if (lane == 32u) inside[i >> 5] = (uint32_t)(bits >> 32);
}

// ---- TILED ------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
wn_brick(Frame f, Pyr py, float beta, float level, const WNode* __restrict__ nodes, const uint32_t* __restrict__ leaf_off,
         const uint4* __restrict__ rec, float* __restrict__ w, uint8_t* __restrict__ inside)
{
    __shared__ uint4 srec[kBatch * kRecU4];
    const uint32_t brick = blockIdx.x, nb = py.nb;
    const int t = (int)threadIdx.x;
    const int bx = (int)(brick % nb) * 8, by = (int)((brick / nb) % nb) * 8, bz = (int)(brick / (nb * nb)) * 8;
    const int x = bx + (t & 7), y = by + ((t >> 3) & 7), z = bz + (t >> 6);
    const float p0[3] = {centre(f.ox, x, f.vs), centre(f.oy, y, f.vs), centre(f.oz, z, f.vs)};
    const float p1[3] = {p0[0], p0[1], centre(f.oz, z + 4, f.vs)};
    const float blo[3] = {centre(f.ox, bx, f.vs), centre(f.oy, by, f.vs), centre(f.oz, bz, f.vs)};
    const float bhi[3] = {centre(f.ox, bx + 7, f.vs), centre(f.oy, by + 7, f.vs), centre(f.oz, bz + 7, f.vs)};
    unsigned long long acc0 = 0, acc1 = 0;
    int k = (int)py.levels - 1;                                    // the walk is the same in every lane: it depends on the brick alone
    uint32_t nx = 0u, ny = 0u, nz = 0u;
    unsigned long long pending = 0ull;
    for (;;) {
        const uint32_t dim = level_dim(nb, k);
        const uint32_t at = nx + dim * (ny + dim * nz);
        const WNode nd = nodes[py.off[k] + at];                    // one address for the workgroup: a broadcast
        bool down = false;
        if (nd.mask) {
            if (node_far(blo, bhi, nd, beta)) {
                acc0 += far_term(p0, nd);
                acc1 += far_term(p1, nd);
            } else if (k == 0) {
                const uint32_t first = leaf_off[at], m = leaf_off[at + 1] - first;
                for (uint32_t b = 0; b < m; b += kBatch) {
                    const uint32_t nrec = min((uint32_t)kBatch, m - b);
                    __syncthreads();                               // the previous batch has been read
                    for (uint32_t j = (uint32_t)t; j < nrec * kRecU4; j += 256) srec[j] = rec[(size_t)(first + b) * kRecU4 + j];
                    __syncthreads();
                    for (uint32_t j = 0; j < nrec; ++j) {
                        const float* r = reinterpret_cast<const float*>(&srec[j * kRecU4]);
                        acc0 += exact_term(p0, r, r + 3, r + 6);
                        acc1 += exact_term(p1, r, r + 3, r + 6);
                    }
                }
            } else down = true;
        }
        if (down) walk_down(nd.mask & 0xFFu, k, nx, ny, nz, pending);
        else if (!walk_next(py, k, nx, ny, nz, pending)) break;
    }
    const uint32_t n = f.n;
    const size_t v0 = (size_t)x + (size_t)n * ((size_t)y + (size_t)n * (size_t)z), v1 = v0 + (size_t)4 * n * n;
    const float w0 = final_w(acc0), w1 = final_w(acc1);
    w[v0] = w0;
    w[v1] = w1;
    // a wave holds one z plane of the brick: eight x rows of eight voxels, one byte of the grid each
    const unsigned long long m0 = __ballot(w0 >= level), m1 = __ballot(w1 >= level);
    const uint32_t lane = (uint32_t)t & 63u;
    if ((lane & 7u) == 0u) {
        inside[v0 >> 3] = (uint8_t)(m0 >> lane);
        inside[v1 >> 3] = (uint8_t)(m1 >> lane);
    }
}

// the number of inside voxels, only when the caller asks for it: one add per workgroup
__global__ void __launch_bounds__(256)
wn_count(const uint32_t* __restrict__ inside, size_t nwords, unsigned long long* __restrict__ counter)
{
    __shared__ unsigned long long smem[4];
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256) s += (unsigned long long)__popc(inside[i]);
    s = wg_sum_256(s, smem);
    if (threadIdx.x == 0 && s) atomicAdd(counter, s);
}

Pyr make_pyramid(uint32_t n)
{
    Pyr py = {};
    py.nb = n / 8;
    uint32_t off = 0;
    for (int k = 0;; ++k) {
        const uint32_t d = level_dim(py.nb, k);
        py.off[k] = off;
        off += d * d * d;
        if (d == 1) { py.levels = (uint32_t)k + 1; py.off[k + 1] = off; break; }
    }
    return py;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

// The caller has validated everything.  Enqueues only once the buffers have grown, unless h_inside_count asks for the count.
int launch_winding(vp_ctx* ctx, const Frame& f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris, float beta, float level,
                   int algo, uint64_t* h_inside_count)
{
    hipStream_t st = ctx->stream;
    const Pyr py = make_pyramid(f.n);
    const size_t voxels = (size_t)f.n * f.n * f.n;
    const uint32_t nleaves = py.off[1], total = py.off[py.levels];
    ctx->wn.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->wn.w, voxels * 4, false));
    VP_TRY(reserve(ctx, ctx->wn.inside, voxels / 8, false));
    VP_TRY(reserve(ctx, ctx->wn.rec, std::max<size_t>(ntris, 1) * kRecU4 * 16));
    // the tree: [counter | sums | boxes | counts | cursors] are zeroed, [nodes | leaf offsets | keys] are written in full
    const size_t o_sum = 16, o_box = o_sum + (size_t)total * 24, o_cnt = o_box + (size_t)total * 24, o_cur = o_cnt + (size_t)total * 4;
    const size_t zeroed = align16(o_cur + (size_t)nleaves * 4);
    const size_t o_nodes = zeroed, o_off = o_nodes + (size_t)total * sizeof(WNode), o_key = align16(o_off + ((size_t)nleaves + 1) * 4);
    VP_TRY(reserve(ctx, ctx->wn.tree, o_key + std::max<size_t>(ntris, 1) * 4));
    if (h_inside_count) VP_TRY(ctx->wn.host.need(1));
    char* base = (char*)ctx->wn.tree.ptr;
    unsigned long long* counter = (unsigned long long*)base;
    unsigned long long* sum = (unsigned long long*)(base + o_sum);
    uint32_t* box = (uint32_t*)(base + o_box);
    uint32_t* cnt = (uint32_t*)(base + o_cnt);
    uint32_t* cur = (uint32_t*)(base + o_cur);
    WNode* nodes = (WNode*)(base + o_nodes);
    uint32_t* leaf_off = (uint32_t*)(base + o_off);
    uint32_t* key = (uint32_t*)(base + o_key);
    const unsigned tblocks = (unsigned)((ntris + 255) / 256);

    VP_HIP(hipMemsetAsync(base, 0, zeroed, st));
    if (ntris) {
        ProfScope p(ctx, VP_K_MD_SETUP);
        hipLaunchKernelGGL(wn_setup, dim3(tblocks), dim3(256), 0, st, f, py.nb, d_xyz, nverts, d_tri, ntris, key, cnt, box, sum);
    }
    {
        ProfScope p(ctx, VP_K_MD_SCAN);
        hipLaunchKernelGGL(wn_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)cnt, nleaves, leaf_off);
    }
    if (ntris) {
        ProfScope p(ctx, VP_K_MD_WRITE);
        hipLaunchKernelGGL(wn_write, dim3(tblocks), dim3(256), 0, st, d_xyz, d_tri, ntris, (const uint32_t*)key, (const uint32_t*)leaf_off, cur,
                           (float4*)ctx->wn.rec.ptr);
    }
    {
        ProfScope p(ctx, VP_K_MD_COUNT);
        for (uint32_t k = 0; k + 1 < py.levels; ++k) {
            const uint32_t dl = level_dim(py.nb, (int)k), du = level_dim(py.nb, (int)k + 1);
            hipLaunchKernelGGL(wn_reduce, dim3((du * du * du + 255u) / 256u), dim3(256), 0, st, dl, du, py.off[k], py.off[k + 1], cnt, box, sum);
        }
        hipLaunchKernelGGL(wn_nodes, dim3((total + 255u) / 256u), dim3(256), 0, st, f.vs, py, (const uint32_t*)cnt, (const uint32_t*)box,
                           (const unsigned long long*)sum, nodes);
    }
    if (algo == VP_ALGO_NAIVE) {
        ProfScope p(ctx, VP_K_MD_NAIVE);
        hipLaunchKernelGGL(wn_naive, dim3((unsigned)(voxels / 256)), dim3(256), 0, st, f, py, beta, level, (const WNode*)nodes,
                           (const uint32_t*)leaf_off, (const float4*)ctx->wn.rec.ptr, (float*)ctx->wn.w.ptr, (uint32_t*)ctx->wn.inside.ptr);
    } else {
        ProfScope p(ctx, VP_K_MD_BRICK);
        hipLaunchKernelGGL(wn_brick, dim3(nleaves), dim3(256), 0, st, f, py, beta, level, (const WNode*)nodes, (const uint32_t*)leaf_off,
                           (const uint4*)ctx->wn.rec.ptr, (float*)ctx->wn.w.ptr, (uint8_t*)ctx->wn.inside.ptr);
    }
    if (h_inside_count) {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(wn_count, dim3((unsigned)std::min<size_t>((voxels / 32 + 255) / 256, (size_t)ctx->cus * 4)), dim3(256), 0, st,
                           (const uint32_t*)ctx->wn.inside.ptr, voxels / 32, counter);
    }
    VP_HIP(hipGetLastError());
    if (h_inside_count) {
        VP_HIP(hipMemcpyAsync(ctx->wn.host, counter, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VP_HIP(hipStreamSynchronize(st));
        *h_inside_count = *ctx->wn.host;
    }
    ctx->wn.n = f.n;
    return 0;
}

}  // namespace vp
