// cvox.hip -- conservative surface voxelization for gfx950 (MI355X).
//
// A voxel is set iff its CLOSED box overlaps the CLOSED triangle: the 26-separating test of Schwarz & Seidel 2010, section 3.1
// (bounding box, triangle plane, three edge-function projections).  The float32 expressions, their association and the
// absence of FMA contraction are the contract (include/vphip.h, vp_voxelize_conservative): this file,
// the host restatement (vplib/src/cvox.cpp) and the tests' numpy restatement agree bit for bit.
//
// Candidate ranges never decide a bit, they only bound which voxels get the predicate:
//   - per axis, the EXACT index range whose voxels pass the bounding-box test (the corner expression is monotone in the index, so a
//     floor() guess corrected by stepping is exact for any frame) -- inside it the box test is not repeated;
//   - per (y, z) row, an x interval solved from the plane in double, widened by a bound of the float rounding of the predicate
//     (row_plane_range below) -- a superset of the voxels whose plane test passes.
//
// TILED:
//   cvox_setup   one thread per triangle.  SMALL triangles (at most kSmallTests candidate voxels -- every triangle of a fine mesh)
//                are rasterised right here: each (row, word) mask is built in registers and written with ONE atomicOr.  LARGE
//                triangles append a record to a compact list (grow-only, sized from what earlier calls counted; a large triangle
//                that finds it full is walked in place -- slow for that call, correct for any input).
//   cvox_scan    exclusive scan of the rows of the listed triangles (one workgroup, 64-bit).
//   cvox_rows    grid-stride over the rows of ALL listed triangles: one lane per (triangle, row), found by a binary search of the
//                scan; the lane walks its plane interval word by word, one atomicOr per touched word.  A triangle that covers
//                10^6 voxels is 10^5+ rows spread over every CU; no lane walks more than one row of n voxels.
// NAIVE: one thread per triangle over its candidate rows, one atomicOr per set voxel (the simple form TILED is tested against).
// accumulate = 0 zero-fills the words first; 1 ORs into them (a union).  Both forms are order-free: OR commutes.
#include "vp_internal.h"
#include "wg_scan.h"

#include <algorithm>
#include <cstdlib>

#pragma clang fp contract(off)

namespace vp {

namespace {

constexpr int kRecU4 = 11;             // record: 38 floats of CTri + boxes + rows = 42 dwords, padded to 11 x 16 B

struct CTri {
    float mn[3], mx[3];                // vertex bounding box
    float nrm[3];                      // Cross(e0, e1)
    float d1, d2;                      // plane offsets of the critical corner and its opposite
    float ne[3][3][3];                 // [projection xy / yz / zx][edge][ne.u, ne.v, de]
};
static_assert(sizeof(CTri) == 38 * 4, "record layout");

struct CRec {
    CTri c;
    uint32_t xb, yb, zb;               // candidate index ranges: lo | hi << 16 (inclusive)
    uint32_t rows;                     // (yhi - ylo + 1) * (zhi - zlo + 1)
    uint32_t pad[2];
};
static_assert(sizeof(CRec) == kRecU4 * 16, "record layout");

__device__ __forceinline__ float corner(float o, int i, float vs) { return o + ((float)i * vs); }
__device__ __forceinline__ float pos(float x) { return x > 0.0f ? x : 0.0f; }     // max(0, x); NaN -> 0 in all three implementations

// Triangle setup of the contract.  false: the triangle contributes nothing (index out of range, non-finite vertex, zero normal).
__device__ __forceinline__ bool ctri_setup(const Frame& f, const float* __restrict__ xyz, size_t nverts, const uint32_t* __restrict__ tri,
                                           size_t t, CTri& c)
{
    const uint32_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (id[0] >= nverts || id[1] >= nverts || id[2] >= nverts) return false;
    float v[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            v[k][a] = xyz[3 * (size_t)id[k] + a];
            if (!__builtin_isfinite(v[k][a])) return false;
        }
    float e[3][3];
    for (int a = 0; a < 3; ++a) { e[0][a] = v[1][a] - v[0][a]; e[1][a] = v[2][a] - v[1][a]; e[2][a] = v[0][a] - v[2][a]; }
    c.nrm[0] = (e[0][1] * e[1][2]) - (e[0][2] * e[1][1]);
    c.nrm[1] = (e[0][2] * e[1][0]) - (e[0][0] * e[1][2]);
    c.nrm[2] = (e[0][0] * e[1][1]) - (e[0][1] * e[1][0]);
    if (c.nrm[0] == 0.0f && c.nrm[1] == 0.0f && c.nrm[2] == 0.0f) return false;
    const float vs = f.vs;
    float cc[3], co[3];
    for (int a = 0; a < 3; ++a) {
        c.mn[a] = fminf(fminf(v[0][a], v[1][a]), v[2][a]);
        c.mx[a] = fmaxf(fmaxf(v[0][a], v[1][a]), v[2][a]);
        cc[a] = c.nrm[a] > 0.0f ? vs : 0.0f;
        co[a] = vs - cc[a];
    }
    c.d1 = ((c.nrm[0] * (cc[0] - v[0][0])) + (c.nrm[1] * (cc[1] - v[0][1]))) + (c.nrm[2] * (cc[2] - v[0][2]));
    c.d2 = ((c.nrm[0] * (co[0] - v[0][0])) + (c.nrm[1] * (co[1] - v[0][1]))) + (c.nrm[2] * (co[2] - v[0][2]));
    // projections q: (u, v) = (x, y), (y, z), (z, x); orientation from nrm.z, nrm.x, nrm.y
    for (int q = 0; q < 3; ++q) {
        const int U = q, V = (q + 1) % 3, S = (q + 2) % 3;
        const float sg = c.nrm[S] >= 0.0f ? 1.0f : -1.0f;
        for (int i = 0; i < 3; ++i) {
            const float nu = (-e[i][V]) * sg, nv = e[i][U] * sg;
            c.ne[q][i][0] = nu;
            c.ne[q][i][1] = nv;
            c.ne[q][i][2] = ((-((nu * v[i][U]) + (nv * v[i][V]))) + pos(vs * nu)) + pos(vs * nv);
        }
    }
    return true;
}

// The exact range [lo, hi] of indices in [L, H] whose voxel passes the box test on this axis: corner(i) <= mx and corner(i) + vs >= mn.
// Both sides are monotone in i (rounding is monotone), so the floor() guess only has to be corrected by stepping.
__device__ __forceinline__ bool axis_range(float mn, float mx, float o, float vs, int L, int H, int& lo, int& hi)
{
    lo = (int)fminf(fmaxf(floorf((mn - o) / vs), (float)L), (float)(H + 1));
    while (lo > L && corner(o, lo - 1, vs) + vs >= mn) --lo;
    while (lo <= H && !(corner(o, lo, vs) + vs >= mn)) ++lo;
    hi = (int)fminf(fmaxf(floorf((mx - o) / vs), (float)(L - 1)), (float)H);
    while (hi < H && corner(o, hi + 1, vs) <= mx) ++hi;
    while (hi >= L && !(corner(o, hi, vs) <= mx)) --hi;
    return lo <= hi;
}

__device__ __forceinline__ bool ctri_box(const Frame& f, const CTri& c, int& xl, int& xh, int& yl, int& yh, int& zl, int& zh)
{
    return axis_range(c.mn[0], c.mx[0], f.ox, f.vs, 0, (int)f.n - 1, xl, xh) &&
           axis_range(c.mn[1], c.mx[1], f.oy, f.vs, 0, (int)f.n - 1, yl, yh) &&
           axis_range(c.mn[2], c.mx[2], f.oz, f.vs, (int)f.z0, (int)f.z1 - 1, zl, zh);
}

// Narrows [xl, xh] of one row to the voxels whose plane test can pass.  The float plane sums s = ((nx px + A) + B) + d carry a
// rounding error below 4 u (|nx px| + |A| + |B| + |d|), u = 2^-24; E below is 1e-6 times that sum (> 16 u), and the index slack m
// covers the rounding of the corner px itself.  Anything not finite keeps the whole range.
__device__ __forceinline__ void row_plane_range(const Frame& f, const CTri& c, float A, float B, int& xl, int& xh)
{
    const double nx = c.nrm[0], ox = f.ox, vs = f.vs;
    const double P = fmax(fabs(ox + (double)xl * vs), fabs(ox + (double)(xh + 1) * vs));
    const double E = 1e-6 * (fabs(nx) * P + fabs((double)A) + fabs((double)B) + fabs((double)c.d1) + fabs((double)c.d2));
    const double base = -(double)A - (double)B;
    const double tlo = base - fmax((double)c.d1, (double)c.d2) - E, thi = base - fmin((double)c.d1, (double)c.d2) + E;
    double plo = tlo / nx, phi = thi / nx;
    if (nx < 0.0) { const double s = plo; plo = phi; phi = s; }
    const double m = 1.0 + 3e-7 * (fabs(ox) + (double)f.n * vs) / vs;
    const double ilo = floor((plo - ox) / vs - m), ihi = ceil((phi - ox) / vs + m);
    if (!(ilo == ilo) || !(ihi == ihi) || !__builtin_isfinite(ilo) || !__builtin_isfinite(ihi)) return;
    if (ilo > (double)xl) xl = ilo > (double)xh ? xh + 1 : (int)ilo;
    if (ihi < (double)xh) xh = ihi < (double)xl ? xl - 1 : (int)ihi;
}

// Tests the voxels [xl, xh] of row (y, z) and ORs the passing ones into the words: one atomicOr per touched word (TILED) or per
// set voxel (PER_BIT, NAIVE).  NARROW: solve the plane interval first (large triangles).
template <bool NARROW, bool PER_BIT>
__device__ __forceinline__ void walk_row(const Frame& f, const CTri& c, int y, int z, int xl, int xh, uint32_t* __restrict__ words)
{
    const float vs = f.vs;
    const float py = corner(f.oy, y, vs), pz = corner(f.oz, z, vs);
    for (int i = 0; i < 3; ++i)                                    // the yz projection is constant along the row
        if (!(((c.ne[1][i][0] * py) + (c.ne[1][i][1] * pz)) + c.ne[1][i][2] >= 0.0f)) return;
    const float A = c.nrm[1] * py, B = c.nrm[2] * pz;
    float kxy[3], kzx[3];
    for (int i = 0; i < 3; ++i) { kxy[i] = c.ne[0][i][1] * py; kzx[i] = c.ne[2][i][0] * pz; }
    if (c.nrm[0] == 0.0f) {                                        // the plane test is constant along the row too
        const float t = ((c.nrm[0] * corner(f.ox, xl, vs)) + A) + B;
        const float s1 = t + c.d1, s2 = t + c.d2;
        if ((s1 > 0.0f && s2 > 0.0f) || (s1 < 0.0f && s2 < 0.0f)) return;
    } else if (NARROW) {
        row_plane_range(f, c, A, B, xl, xh);
    }
    if (xl > xh) return;
    uint32_t* row = words + ((size_t)(z - (int)f.z0) * f.n + (size_t)y) * f.w;
    for (int w = xl >> 5; w <= (xh >> 5); ++w) {
        const int b = max(xl, w * 32), e = min(xh, w * 32 + 31);
        uint32_t m = 0;
        for (int x = b; x <= e; ++x) {
            const float px = corner(f.ox, x, vs);
            const float t = ((c.nrm[0] * px) + A) + B;
            const float s1 = t + c.d1, s2 = t + c.d2;
            if ((s1 > 0.0f && s2 > 0.0f) || (s1 < 0.0f && s2 < 0.0f)) continue;
            bool ok = true;
            for (int i = 0; i < 3; ++i) {
                ok = ok && ((c.ne[0][i][0] * px) + kxy[i]) + c.ne[0][i][2] >= 0.0f;
                ok = ok && (kzx[i] + (c.ne[2][i][1] * px)) + c.ne[2][i][2] >= 0.0f;
            }
            if (!ok) continue;
            if (PER_BIT) atomicOr(&row[w], 1u << (x & 31));
            else m |= 1u << (x & 31);
        }
        if (!PER_BIT && m) atomicOr(&row[w], m);
    }
}

#ifndef VP_CVOX_SMALL_TESTS
#define VP_CVOX_SMALL_TESTS 256
#endif
constexpr uint64_t kSmallTests = VP_CVOX_SMALL_TESTS;     // candidate voxels up to which a triangle is walked by its setup thread

__global__ void __launch_bounds__(256)
cvox_setup(Frame f, const float* __restrict__ xyz, size_t nverts, const uint32_t* __restrict__ tri, size_t ntris,
           CRec* __restrict__ rec, uint32_t rec_cap, uint32_t* __restrict__ nbig, uint32_t* __restrict__ words)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    CTri c;
    if (!ctri_setup(f, xyz, nverts, tri, t, c)) return;
    int xl, xh, yl, yh, zl, zh;
    if (!ctri_box(f, c, xl, xh, yl, yh, zl, zh)) return;
    const uint32_t rows = (uint32_t)((yh - yl + 1) * (zh - zl + 1));
    if ((uint64_t)rows * (uint64_t)(xh - xl + 1) > kSmallTests) {
        const uint32_t slot = atomicAdd(nbig, 1u);                 // counts every large triangle, listed or not
        if (slot < rec_cap) {
            CRec r;
            r.c = c;
            r.xb = (uint32_t)xl | ((uint32_t)xh << 16);
            r.yb = (uint32_t)yl | ((uint32_t)yh << 16);
            r.zb = (uint32_t)zl | ((uint32_t)zh << 16);
            r.rows = rows; r.pad[0] = r.pad[1] = 0;
            rec[slot] = r;
            return;
        }
        for (int z = zl; z <= zh; ++z)                             // list full: walked here (this call only; the next one has room)
            for (int y = yl; y <= yh; ++y) walk_row<true, false>(f, c, y, z, xl, xh, words);
        return;
    }
    for (int z = zl; z <= zh; ++z)
        for (int y = yl; y <= yh; ++y) walk_row<false, false>(f, c, y, z, xl, xh, words);
}

// One workgroup: base[i] = rows of the listed records before i (64-bit), base[nrec] = all of them.
__global__ void __launch_bounds__(1024)
cvox_scan(const CRec* __restrict__ rec, const uint32_t* __restrict__ nbig, uint32_t rec_cap, unsigned long long* __restrict__ base)
{
    __shared__ unsigned long long part[1024];
    const uint32_t m = min(*nbig, rec_cap);
    const unsigned long long total = wg_scan_1024(part, m, [&](uint32_t i) { return (unsigned long long)rec[i].rows; },
                                                  [&](uint32_t i, unsigned long long before) { base[i] = before; });
    if (threadIdx.x == 1023) base[m] = total;
}

// One lane per (listed triangle, candidate row), grid-stride over all of them.
__global__ void __launch_bounds__(256)
cvox_rows(Frame f, const CRec* __restrict__ rec, const uint32_t* __restrict__ nbig, uint32_t rec_cap,
          const unsigned long long* __restrict__ base, uint32_t* __restrict__ words)
{
    const uint32_t m = min(*nbig, rec_cap);
    const unsigned long long total = base[m];
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += stride) {
        uint32_t lo = 0, hi = m - 1;                               // the last record whose base is <= r (records have rows > 0)
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (base[mid] <= r) lo = mid; else hi = mid - 1;
        }
        const CRec& q = rec[lo];
        const uint32_t k = (uint32_t)(r - base[lo]);
        const int yl = (int)(q.yb & 0xFFFF), yh = (int)(q.yb >> 16), zl = (int)(q.zb & 0xFFFF);
        const int ny = yh - yl + 1;
        const CTri c = q.c;
        walk_row<true, false>(f, c, yl + (int)(k % (uint32_t)ny), zl + (int)(k / (uint32_t)ny), (int)(q.xb & 0xFFFF), (int)(q.xb >> 16), words);
    }
}

__global__ void __launch_bounds__(256)
cvox_naive(Frame f, const float* __restrict__ xyz, size_t nverts, const uint32_t* __restrict__ tri, size_t ntris, uint32_t* __restrict__ words)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntris) return;
    CTri c;
    if (!ctri_setup(f, xyz, nverts, tri, t, c)) return;
    int xl, xh, yl, yh, zl, zh;
    if (!ctri_box(f, c, xl, xh, yl, yh, zl, zh)) return;
    for (int z = zl; z <= zh; ++z)
        for (int y = yl; y <= yh; ++y) walk_row<true, true>(f, c, y, z, xl, xh, words);
}

// zero-fill of the grid (overwrite; nvec = 0 when accumulating) and of the large-triangle counter
__global__ void __launch_bounds__(256)
cvox_zero(uint4* __restrict__ grid, size_t nvec, uint32_t* __restrict__ cnt)
{
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = t0; i < nvec; i += stride) grid[i] = make_uint4(0u, 0u, 0u, 0u);
    if (t0 == 0 && cnt) *cnt = 0u;
}

}  // namespace

int launch_voxelize_conservative(vp_ctx* ctx, const Frame& f, uint32_t* d_words, const float* d_xyz, size_t nverts,
                                 const uint32_t* d_tri, size_t ntris, int algo, int accumulate)
{
    hipStream_t st = ctx->stream;
    const size_t nwords = (size_t)f.n * f.n * (f.z1 - f.z0) / 32;
    const unsigned tblocks = (unsigned)((ntris + 255) / 256);
    const bool tiled = algo == VP_ALGO_TILED && ntris > 0;
    VP_TRY(reserve(ctx, ctx->cvox.cnt, 16));
    uint32_t* d_nbig = (uint32_t*)ctx->cvox.cnt.ptr;
    {
        // nwords is a multiple of 8 n (n % 32 == 0): whole uint4s; d_words is 16-byte aligned (checked at the ABI)
        const size_t nvec = accumulate ? 0 : nwords / 4;
        if (nvec || tiled) {
            const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, 256 * 16));
            ProfScope p(ctx, VP_K_CVOX_ZERO);
            hipLaunchKernelGGL(cvox_zero, dim3(blocks), dim3(256), 0, st, (uint4*)d_words, nvec, tiled ? d_nbig : nullptr);
        }
    }
    if (!ntris) { VP_HIP(hipGetLastError()); return 0; }

    if (algo == VP_ALGO_NAIVE) {
        ProfScope p(ctx, VP_K_CVOX_NAIVE);
        hipLaunchKernelGGL(cvox_naive, dim3(tblocks), dim3(256), 0, st, f, d_xyz, nverts, d_tri, ntris, d_words);
        VP_HIP(hipGetLastError());
        return 0;
    }

    // ---- TILED ----
    // Large-triangle count of an earlier call, if its copy has landed (never waited for): sizes the record list, grow-only.  This is the
    // conservative path's own state; the solid voxelizer's job cache is neither read nor written.
    if (ctx->cvox.event && ctx->cvox.pending && hipEventQuery(ctx->cvox.event) == hipSuccess) {
        ctx->cvox.pending = false;
        ctx->cvox.nbig_seen = std::max<uint64_t>(ctx->cvox.nbig_seen, ctx->cvox.host[0]);
    }
    const size_t wantRec = std::min<size_t>(ntris, std::max<size_t>((size_t)1 << 16, (size_t)ctx->cvox.nbig_seen + ctx->cvox.nbig_seen / 4));
    VP_TRY(reserve(ctx, ctx->cvox.rec, wantRec * sizeof(CRec)));
    uint32_t rcap = (uint32_t)std::min<size_t>(ctx->cvox.rec.bytes / sizeof(CRec), ntris);
#ifdef VP_TEST_HOOKS   // test builds only (libvphip_hooks.so): force the walk-in-place path of a full record list
    if (const char* e = getenv("VP_CVOX_REC_CAP")) rcap = std::min<uint32_t>(rcap, (uint32_t)strtoul(e, nullptr, 10));
#endif
    VP_TRY(reserve(ctx, ctx->cvox.base, ((size_t)rcap + 1) * 8));
    CRec* rec = (CRec*)ctx->cvox.rec.ptr;
    unsigned long long* base = (unsigned long long*)ctx->cvox.base.ptr;
    {
        ProfScope p(ctx, VP_K_CVOX_SETUP);
        hipLaunchKernelGGL(cvox_setup, dim3(tblocks), dim3(256), 0, st, f, d_xyz, nverts, d_tri, ntris, rec, rcap, d_nbig, d_words);
    }
    VP_TRY(ctx->cvox.host.need(1, true));
    if (!ctx->cvox.event) VP_HIP(hipEventCreateWithFlags(&ctx->cvox.event, hipEventDisableTiming));
    if (!ctx->cvox.pending) {
        VP_HIP(hipMemcpyAsync(ctx->cvox.host, d_nbig, 4, hipMemcpyDeviceToHost, st));
        VP_HIP(hipEventRecord(ctx->cvox.event, st));
        ctx->cvox.pending = true;
    }
    {
        ProfScope p(ctx, VP_K_CVOX_SCAN);
        hipLaunchKernelGGL(cvox_scan, dim3(1), dim3(1024), 0, st, rec, d_nbig, rcap, base);
    }
    {
        ProfScope p(ctx, VP_K_CVOX_ROWS);
        hipLaunchKernelGGL(cvox_rows, dim3((unsigned)ctx->cus * 8u), dim3(256), 0, st, f, rec, d_nbig, rcap, base, d_words);
    }
    VP_HIP(hipGetLastError());
    return 0;
}

}  // namespace vp
