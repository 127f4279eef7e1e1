// thickness.hip -- local thickness of a whole-grid bit grid for gfx950 (MI355X): vp_thickness (include/vphip.h).
//
// D(c) = min(E(c), W(c), rmax^2) on the set voxels c -- E the exact squared distance to the nearest unset voxel (edt.hip), W the squared
// distance to the first voxel outside the grid -- is the capped squared radius of the largest open ball around c that holds set voxels only.
// T2(p) = max { D(c) : |p - c|^2 < D(c) } is the largest such ball that covers p.  Integers and a maximum over a set: both algos, the host
// restatement and numpy agree bit for bit whatever any of them skips.
//   NAIVE  th_paint        one thread per set voxel c scatters D(c) over its ball with atomicMax; no culling, no LDS.  The check.
//          th_thin_naive   T2 -> the thin grid, 64 voxels per ballot.
//   TILED  th_cap          one workgroup per 8 x 8 x 8 brick: D as uint16 (rmax^2 <= 1024), the grid of the saturated centres {D = rmax^2}
//                          and the brick's largest UNSATURATED D (what th_brick culls with).
//          (edt.hip)       the saturated region {T2 = rmax^2} is the set of voxels closer than rmax to a saturated centre: one more
//                          separable transform (seeds = the saturated centres) and a threshold.  No ball is painted for it.
//          th_brick        one workgroup per brick, two voxels per lane.  A brick without a set, unsaturated voxel leaves at once (th_fill
//                          writes it).  Otherwise the neighbour bricks within rmax - 1 voxels are walked; one whose largest unsaturated D
//                          is not above the squared gap between the two boxes is skipped by the whole workgroup.  In a visited brick
//                          every lane tests two candidates c: 0 < D(c) < rmax^2 and squared gap from c to the target box < D(c); the
//                          survivors are ballot-compacted into an LDS batch (3 x 7 bits of region-relative coordinates + 10 bits of D)
//                          and all lanes loop over the batch with broadcast reads.  One store of T2 per voxel, the thin bits by ballot
//                          (a wave holds whole z planes of the brick).  No atomics on the field.
//          th_fill         the bricks no workgroup owned: 0 on unset voxels, rmax^2 on saturated ones, no thin bit.
//   th_count               the number of thin voxels, when the caller asks for it.
#include <algorithm>

#include "vp_internal.h"
#include "wg_scan.h"

namespace vp {

namespace {

constexpr int kBatch = 2048;                                      // entries of th_brick's LDS batch (8 KiB)

// D of voxel (x, y, z) from its E; 0 on an unset voxel (E = 0: the voxel is its own seed)
__device__ __forceinline__ uint32_t capped(uint32_t e, int x, int y, int z, int n, uint32_t rmax2)
{
    if (e == 0u) return 0u;
    const int m = min(min(min(x, n - 1 - x), min(y, n - 1 - y)), min(z, n - 1 - z)) + 1;
    return min(min(e, (uint32_t)(m * m)), rmax2);
}

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
th_paint(const uint32_t* __restrict__ E, uint32_t* __restrict__ T2, int n, uint32_t rmax2, size_t nvox)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nvox) return;
    const int x = (int)(idx % (size_t)n), y = (int)((idx / (size_t)n) % (size_t)n), z = (int)(idx / ((size_t)n * n));
    const uint32_t D = capped(E[idx], x, y, z, n, rmax2);
    if (D == 0u) return;
    int r = 0;                                                     // the largest r with r^2 < D; r < W's root, so the ball stays in the grid
    while ((uint32_t)((r + 1) * (r + 1)) < D) ++r;
    for (int dz = -r; dz <= r; ++dz)
        for (int dy = -r; dy <= r; ++dy) {
            const uint32_t qzy = (uint32_t)(dz * dz + dy * dy);
            if (qzy >= D) continue;
            uint32_t* row = T2 + ((ptrdiff_t)idx + (ptrdiff_t)dy * n + (ptrdiff_t)dz * n * n);
            for (int dx = -r; dx <= r; ++dx)
                if (qzy + (uint32_t)(dx * dx) < D) atomicMax(row + dx, D);
        }
}

// bit = set (T2 != 0) and T2 < thin2; the voxel count is a multiple of 256, so every wave is whole
__global__ void __launch_bounds__(256)
th_thin_naive(const uint32_t* __restrict__ T2, uint32_t* __restrict__ thin, uint32_t thin2)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = T2[idx];
    const unsigned long long m = __ballot(v != 0u && v < thin2);
    if ((threadIdx.x & 63u) == 0u) reinterpret_cast<uint2*>(thin)[idx >> 6] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

// lane t of the workgroup of brick b holds the voxels (8 bx + (t & 7), 8 by + ((t >> 3) & 7), 8 bz + (t >> 6)) and the one four planes above
struct BrickLane { int x0, y0, z0, lx, ly, lz; size_t v0, v1; };

__device__ __forceinline__ BrickLane brick_lane(uint32_t brick, uint32_t nb, uint32_t n)
{
    BrickLane b;
    const int t = (int)threadIdx.x;
    b.x0 = (int)(brick % nb) * 8; b.y0 = (int)((brick / nb) % nb) * 8; b.z0 = (int)(brick / (nb * nb)) * 8;
    b.lx = t & 7; b.ly = (t >> 3) & 7; b.lz = t >> 6;
    b.v0 = (size_t)(b.x0 + b.lx) + (size_t)n * ((size_t)(b.y0 + b.ly) + (size_t)n * (size_t)(b.z0 + b.lz));
    b.v1 = b.v0 + (size_t)4 * n * n;
    return b;
}

__global__ void __launch_bounds__(256)
th_cap(const uint32_t* __restrict__ E, uint32_t n, uint32_t rmax2, uint16_t* __restrict__ D16, uint8_t* __restrict__ satc,
       uint32_t* __restrict__ umax)
{
    __shared__ uint32_t s_max[4];
    const BrickLane b = brick_lane(blockIdx.x, n / 8, n);
    const uint32_t d0 = capped(E[b.v0], b.x0 + b.lx, b.y0 + b.ly, b.z0 + b.lz, (int)n, rmax2);
    const uint32_t d1 = capped(E[b.v1], b.x0 + b.lx, b.y0 + b.ly, b.z0 + b.lz + 4, (int)n, rmax2);
    D16[b.v0] = (uint16_t)d0;
    D16[b.v1] = (uint16_t)d1;
    // a wave holds one z plane of the brick: eight x rows of eight voxels, one byte of the grid each
    const unsigned long long m0 = __ballot(d0 == rmax2), m1 = __ballot(d1 == rmax2);
    const uint32_t lane = threadIdx.x & 63u;
    if ((lane & 7u) == 0u) {
        satc[b.v0 >> 3] = (uint8_t)(m0 >> lane);
        satc[b.v1 >> 3] = (uint8_t)(m1 >> lane);
    }
    uint32_t u = max(d0 < rmax2 ? d0 : 0u, d1 < rmax2 ? d1 : 0u);
    for (int d = 32; d >= 1; d >>= 1) u = max(u, (uint32_t)__shfl_xor((int)u, d));
    if (lane == 0u) s_max[threadIdx.x >> 6] = u;
    __syncthreads();
    if (threadIdx.x == 0) umax[blockIdx.x] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
}

__device__ __forceinline__ int axis_gap(int c, int lo) { return max(0, max(lo - c, c - (lo + 7))); }      // from c to the voxels lo .. lo + 7

__global__ void __launch_bounds__(256)
th_brick(const uint16_t* __restrict__ D16, const uint32_t* __restrict__ umax, const uint8_t* __restrict__ sat, uint32_t n, uint32_t rmax,
         uint32_t thin2, uint32_t* __restrict__ T2, uint8_t* __restrict__ thin, uint32_t* __restrict__ own)
{
    __shared__ uint32_t s_batch[kBatch];
    __shared__ uint32_t s_count;
    const uint32_t nb = n / 8, rmax2 = rmax * rmax;
    const BrickLane b = brick_lane(blockIdx.x, nb, n);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d0 = D16[b.v0], d1 = D16[b.v1];
    const bool s0 = (sat[b.v0 >> 3] >> b.lx) & 1u, s1 = (sat[b.v1 >> 3] >> b.lx) & 1u;
    const int mine = __syncthreads_or((d0 != 0u && !s0) || (d1 != 0u && !s1));
    if (threadIdx.x == 0) { own[blockIdx.x] = mine ? 1u : 0u; s_count = 0u; }
    if (!mine) return;                                             // the whole workgroup: th_fill writes this brick
    __syncthreads();

    // coordinates relative to (x0 - 32, y0 - 32, z0 - 32): every candidate lies in 0 .. 71
    const int px = b.lx + 32, py = b.ly + 32, pz0 = b.lz + 32, pz1 = b.lz + 36;
    uint32_t t0 = 0u, t1 = 0u, total = 0u;
    auto drain = [&](uint32_t m) {
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t e = s_batch[j];                         // one address for the workgroup: a broadcast
            const int dx = (int)(e & 127u) - px, dy = (int)((e >> 7) & 127u) - py, ez = (int)((e >> 14) & 127u);
            const uint32_t D = e >> 21, qxy = (uint32_t)(dx * dx + dy * dy);
            const int dz0 = ez - pz0, dz1 = ez - pz1;
            if (qxy + (uint32_t)(dz0 * dz0) < D) t0 = max(t0, D);
            if (qxy + (uint32_t)(dz1 * dz1) < D) t1 = max(t1, D);
        }
    };
    auto append = [&](bool ok, uint32_t e) {
        const unsigned long long m = __ballot(ok);
        uint32_t base = 0u;
        if (lane == 0u && m) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0);
        if (ok) s_batch[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = e;
    };

    const int R = (int)rmax - 1, bx = b.x0 >> 3, by = b.y0 >> 3, bz = b.z0 >> 3, last = (int)nb - 1;
    const int lox = max(0, (b.x0 - R) >> 3), hix = min(last, (b.x0 + 7 + R) >> 3);
    const int loy = max(0, (b.y0 - R) >> 3), hiy = min(last, (b.y0 + 7 + R) >> 3);
    const int loz = max(0, (b.z0 - R) >> 3), hiz = min(last, (b.z0 + 7 + R) >> 3);
    for (int nz = loz; nz <= hiz; ++nz)
        for (int ny = loy; ny <= hiy; ++ny)
            for (int nx = lox; nx <= hix; ++nx) {
                // the gap between the closest voxels of two bricks k apart along an axis is 8 k - 7
                const int kx = abs(nx - bx), ky = abs(ny - by), kz = abs(nz - bz);
                const int gx = kx ? 8 * kx - 7 : 0, gy = ky ? 8 * ky - 7 : 0, gz = kz ? 8 * kz - 7 : 0;
                const uint32_t nbrick = (uint32_t)nx + nb * ((uint32_t)ny + nb * (uint32_t)nz);
                if (umax[nbrick] <= (uint32_t)(gx * gx + gy * gy + gz * gz)) continue;      // wave-uniform: no ball of it reaches this brick
                const int cx = nx * 8 + b.lx, cy = ny * 8 + b.ly, cz = nz * 8 + b.lz;
                const size_t c = (size_t)cx + (size_t)n * ((size_t)cy + (size_t)n * (size_t)cz);
                const uint32_t c0 = D16[c], c1 = D16[c + (size_t)4 * n * n];
                const int ax = axis_gap(cx, b.x0), ay = axis_gap(cy, b.y0), az0 = axis_gap(cz, b.z0), az1 = axis_gap(cz + 4, b.z0);
                const uint32_t qxy = (uint32_t)(ax * ax + ay * ay);
                const bool ok0 = c0 != 0u && c0 < rmax2 && qxy + (uint32_t)(az0 * az0) < c0;
                const bool ok1 = c1 != 0u && c1 < rmax2 && qxy + (uint32_t)(az1 * az1) < c1;
                const uint32_t exy = (uint32_t)(cx - b.x0 + 32) | ((uint32_t)(cy - b.y0 + 32) << 7);
                append(ok0, exy | ((uint32_t)(cz - b.z0 + 32) << 14) | (c0 << 21));
                append(ok1, exy | ((uint32_t)(cz - b.z0 + 36) << 14) | (c1 << 21));
                total += (uint32_t)__syncthreads_count(ok0);
                total += (uint32_t)__syncthreads_count(ok1);
                if (total > (uint32_t)kBatch - 512u) {             // the next brick may not fit: 512 candidates at most
                    drain(total);
                    __syncthreads();
                    if (threadIdx.x == 0) s_count = 0u;
                    total = 0u;
                    __syncthreads();
                }
            }
    drain(total);
    const uint32_t r0 = d0 == 0u ? 0u : (s0 ? rmax2 : t0), r1 = d1 == 0u ? 0u : (s1 ? rmax2 : t1);
    T2[b.v0] = r0;
    T2[b.v1] = r1;
    const unsigned long long m0 = __ballot(d0 != 0u && r0 < thin2), m1 = __ballot(d1 != 0u && r1 < thin2);
    if ((lane & 7u) == 0u) {
        thin[b.v0 >> 3] = (uint8_t)(m0 >> lane);
        thin[b.v1 >> 3] = (uint8_t)(m1 >> lane);
    }
}

// one lane per x row of eight voxels of a brick that th_brick left: a set voxel there is saturated
__global__ void __launch_bounds__(256)
th_fill(const uint32_t* __restrict__ own, const uint8_t* __restrict__ sat, uint32_t n, uint32_t rmax2, uint32_t* __restrict__ T2,
        uint8_t* __restrict__ thin, size_t rows)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint32_t nb = n / 8;
    const uint32_t x8 = (uint32_t)(r % nb), y = (uint32_t)((r / nb) % n), z = (uint32_t)(r / ((size_t)nb * n));
    if (own[x8 + nb * ((y >> 3) + nb * (z >> 3))]) return;
    const uint32_t s = sat[r];
    uint4* out = reinterpret_cast<uint4*>(T2 + r * 8);
    out[0] = make_uint4((s & 1u) ? rmax2 : 0u, (s & 2u) ? rmax2 : 0u, (s & 4u) ? rmax2 : 0u, (s & 8u) ? rmax2 : 0u);
    out[1] = make_uint4((s & 16u) ? rmax2 : 0u, (s & 32u) ? rmax2 : 0u, (s & 64u) ? rmax2 : 0u, (s & 128u) ? rmax2 : 0u);
    thin[r] = 0;
}

// the number of thin voxels, only when the caller asks for it: one add per workgroup
__global__ void __launch_bounds__(256)
th_count(const uint32_t* __restrict__ thin, size_t nwords, unsigned long long* __restrict__ counter)
{
    __shared__ unsigned long long smem[4];
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256) s += (unsigned long long)__popc(thin[i]);
    s = wg_sum_256(s, smem);
    if (threadIdx.x == 0 && s) atomicAdd(counter, s);
}

}  // namespace

// The caller has validated everything.  Enqueues only once the buffers have grown, unless h_thin_count asks for the count.
int launch_thickness(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, uint32_t rmax, uint32_t thin2, int algo, uint64_t* h_thin_count)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n, nb = n / 8, nbricks = nb * nb * nb, rmax2 = rmax * rmax;
    const size_t nvox = (size_t)n * n * n;
    ctx->th.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->th.t2, nvox * 4, false));
    VP_TRY(reserve(ctx, ctx->th.thin, nvox / 8, false));
    VP_TRY(reserve(ctx, ctx->edt.vol, nvox * 4, false));
    if (algo == VP_ALGO_NAIVE) VP_TRY(reserve(ctx, ctx->edt.vol2, nvox * 4, false));
    else {
        VP_TRY(reserve(ctx, ctx->th.d16, nvox * 2, false));
        VP_TRY(reserve(ctx, ctx->th.sat, nvox / 4, false));          // the saturated centres, then the saturated region
    }
    VP_TRY(reserve(ctx, ctx->th.sum, 16 + (size_t)nbricks * 8, false));  // the thin count | per brick: the largest unsaturated D | owned
    if (h_thin_count) VP_TRY(ctx->th.host.need(1));
    uint32_t* E = (uint32_t*)ctx->edt.vol.ptr;
    uint32_t* T2 = (uint32_t*)ctx->th.t2.ptr;
    uint32_t* thin = (uint32_t*)ctx->th.thin.ptr;
    unsigned long long* counter = (unsigned long long*)ctx->th.sum.ptr;
    uint32_t* umax = (uint32_t*)((char*)ctx->th.sum.ptr + 16);
    uint32_t* own = umax + nbricks;

    if (algo == VP_ALGO_NAIVE) {
        VP_HIP(hipMemsetAsync(T2, 0, nvox * 4, st));
        VP_TRY(launch_edt(ctx, f, d_words, VP_EDT_SEEDS_UNSET, E, algo));
        {
            ProfScope p(ctx, VP_K_MD_NAIVE);
            hipLaunchKernelGGL(th_paint, dim3((unsigned)(nvox / 256)), dim3(256), 0, st, (const uint32_t*)E, T2, (int)n, rmax2, nvox);
        }
        ProfScope p(ctx, VP_K_EDT_THRESH);
        hipLaunchKernelGGL(th_thin_naive, dim3((unsigned)(nvox / 256)), dim3(256), 0, st, (const uint32_t*)T2, thin, thin2);
    } else {
        uint16_t* D16 = (uint16_t*)ctx->th.d16.ptr;
        uint32_t* satc = (uint32_t*)ctx->th.sat.ptr;
        uint32_t* sat = satc + nvox / 32;
        VP_TRY(launch_edt(ctx, f, d_words, VP_EDT_SEEDS_UNSET, E, algo));
        {
            ProfScope p(ctx, VP_K_EDT_THRESH);
            hipLaunchKernelGGL(th_cap, dim3(nbricks), dim3(256), 0, st, (const uint32_t*)E, n, rmax2, D16, (uint8_t*)satc, umax);
        }
        VP_HIP(hipGetLastError());
        // E is spent (D16 holds what is needed of it): the same volume takes the distance to the saturated centres
        VP_TRY(launch_edt(ctx, f, satc, VP_EDT_SEEDS_SET, E, algo));
        VP_TRY(launch_edt_thresh(ctx, n, E, sat, rmax2 - 1u, 0));
        {
            ProfScope p(ctx, VP_K_MD_BRICK);
            hipLaunchKernelGGL(th_brick, dim3(nbricks), dim3(256), 0, st, (const uint16_t*)D16, (const uint32_t*)umax, (const uint8_t*)sat, n, rmax,
                               thin2, T2, (uint8_t*)thin, own);
        }
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(th_fill, dim3((unsigned)((nvox / 8 + 255) / 256)), dim3(256), 0, st, (const uint32_t*)own, (const uint8_t*)sat, n, rmax2,
                           T2, (uint8_t*)thin, nvox / 8);
    }
    VP_HIP(hipGetLastError());
    if (h_thin_count) {
        VP_HIP(hipMemsetAsync(counter, 0, 16, st));
        {
            ProfScope p(ctx, VP_K_MD_SPLIT);
            hipLaunchKernelGGL(th_count, dim3((unsigned)std::min<size_t>((nvox / 32 + 255) / 256, (size_t)ctx->cus * 4)), dim3(256), 0, st,
                               (const uint32_t*)thin, nvox / 32, counter);
        }
        VP_HIP(hipGetLastError());
        VP_HIP(hipMemcpyAsync(ctx->th.host, counter, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VP_HIP(hipStreamSynchronize(st));
        *h_thin_count = *ctx->th.host;
    }
    ctx->th.n = n;
    return 0;
}

}  // namespace vp
