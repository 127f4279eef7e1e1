// geodesic.hip -- geodesic distance inside a mask from seed voxels, whole-grid bit grids, for gfx950 (MI355X): vp_geodesic (include/vphip.h;
// DESIGN.md section 21).
//
// D holds one uint32 per voxel: 0 at the used seeds (S & M), VP_GEO_NONE elsewhere, then lowered by pulls D[p] = min(D[p], D[q] + w) over
// the allowed neighbours q of p in M, the add saturating at VP_GEO_MAX, until nothing changes.
//   both   gd_init    one lane per four voxels: D from the two bit grids (16 B per lane), the seed count, TILED's first block flags
//          gd_final   one lane per voxel: the reach grid (one ballot = 64 bits = two words), the reached count and the key
//                     (D << 32 | ~index) of the farthest voxel, reduced over the workgroup and then with one atomicMax: the larger D wins,
//                     among equal D the lower index, whichever workgroup comes first
//   NAIVE  gd_naive   one lane per voxel of M, global memory only, in place.  Whole-grid launches repeat until one changes nothing, kGeoBatch
//                     rounds per read-back of their flags (round_ring.h).
//   TILED  gd_relax   one workgroup per ACTIVE block of 32 x 16 x 16 voxels, 256 lanes = one per x row.  The block's D and a one-voxel halo
//                     are staged in LDS (the tile of block_list.h: 45,360 B, three workgroups per CU), the lane's mask row is a register.  One
//                     sweep: the lane walks along its row with a sliding window of column minima over the eight rows around it (9 LDS
//                     reads per voxel), then relaxes forward and backward along its own row in registers (exact for the face weight) and
//                     stores what it lowered.  Sweeps repeat until one lowers nothing in the block or kGeoSweeps have run; then the
//                     values that changed are written back, by the lanes along x.
//          block_list (block_list.h)  the list of active blocks from the block flags.  A block whose face, edge or corner voxel changed
//                     raises the flags of exactly the neighbour blocks whose halo holds that voxel (face neighbours only for VP_GEO_6);
//                     a block that was still changing at the sweep cap raises its own.  The first list is the blocks whose tile holds a
//                     used seed, in its interior OR in its halo (gd_init raises them by the same rule: a seed reads 0 from the start and
//                     is never "changed"); the host loop ends with the first empty list.
// Order-free, for both: (1) every voxel of D has one writer in any launch -- its own lane (NAIVE), the workgroup of its block, which the
// list names once (TILED).  (2) Values only decrease: a value is stored only where it is smaller than the one read.  (3) Every value ever
// stored is 0 at a used seed or D[q] + w for a stored D[q] and an allowed step, so by induction it is the cost of a real path from a seed
// and >= the true distance.  (4) Aligned 32-bit loads and stores do not tear: a read of a neighbour's voxel during the neighbour's write
// sees the old or the new value, both upper bounds of that kind; inside a workgroup the same holds for LDS between two barriers.  (5) A
// block is run after every event that puts a finite value into its tile (interior or halo): the initial D does so only at the used seeds,
// and gd_init lists every block whose tile holds one; every later store is a lowering, whose flags are raised in the launch that makes
// it and read after the kernel boundary; a block that stops at the cap re-lists itself.  A block that is never listed therefore has a tile
// that holds VP_GEO_NONE only, from start to end, and the pull of each of its voxels gives VP_GEO_NONE, which is what it reads.  NAIVE
// reruns everything.  (6) Hence when a launch changes nothing (NAIVE) or the list is empty (TILED) -- no store happened since every voxel
// of a block that was ever listed last evaluated its pull, and the others have nothing to pull -- D[p] = min(D[q] + w) holds at every
// voxel of M but the seeds, and with (3) D is the shortest distance: the unique fixed point, whatever the order of execution.  Saturation
// is monotone and changes none of it.
// Kernel boundaries are the only synchronisation between workgroups; every device loop has a compile-time bound.
#include "block_list.h"
#include "round_ring.h"
#include "vp_internal.h"

#include <algorithm>

namespace vp {

namespace {

constexpr uint32_t kGeoSweeps = 64;  // TILED: sweeps over a block per launch at most (tests/test_geodesic_gpu.py reads this line)
constexpr uint32_t kGeoBatch = 8;    // NAIVE: rounds enqueued between two read-backs of their flags
constexpr uint32_t kNone = VP_GEO_NONE, kMax = VP_GEO_MAX;
// the counters in front of the flags: kAuxHead bytes, of which seeds used (u64) | voxels reached (u64) | key of the farthest voxel (u64) |
// active blocks (u32) are in use; kCnt* = where each starts, in 32-bit words
constexpr uint32_t kCntSeeds = 0, kCntReached = 2, kCntKey = 4, kCntActive = 6;

template <int METRIC> struct Weights;
template <> struct Weights<VP_GEO_6> { static constexpr uint32_t w1 = 1, w2 = 0, w3 = 0; static constexpr bool diagonal = false; };
template <> struct Weights<VP_GEO_26> { static constexpr uint32_t w1 = 1, w2 = 1, w3 = 1; static constexpr bool diagonal = true; };
template <> struct Weights<VP_GEO_CHAMFER> { static constexpr uint32_t w1 = 3, w2 = 4, w3 = 5; static constexpr bool diagonal = true; };

// min(d + w, VP_GEO_MAX); VP_GEO_NONE stays
__device__ __forceinline__ uint32_t gd_add(uint32_t d, uint32_t w) { return d == kNone ? kNone : (d > kMax - w ? kMax : d + w); }

// ---- both --------------------------------------------------------------------------------------------------------------------------

// lane i serves voxels 4 i .. 4 i + 3.  n^3 / 4 is a multiple of 256: every workgroup is whole.  flags != nullptr (TILED): the first list --
// a used seed reads 0 from the start and is never "lowered", so every block whose tile holds one, in its interior or in its halo, is
// raised here
__global__ void __launch_bounds__(256)
gd_init(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ seeds, uint4* __restrict__ D, uint32_t n, uint32_t* __restrict__ flags,
        int diagonal, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, word = i >> 3;
    const uint32_t used = mask[word] & seeds[word], s = used >> ((uint32_t)(i & 7u) * 4u);
    D[i] = make_uint4((s & 1u) ? 0u : kNone, (s & 2u) ? 0u : kNone, (s & 4u) ? 0u : kNone, (s & 8u) ? 0u : kNone);
    if ((i & 7u) == 0 && used != 0u && flags) {
        const uint32_t w = n / 32, y = (uint32_t)((word / w) % n), z = (uint32_t)(word / ((size_t)w * n));
        const BlockAt at{(uint32_t)(word % w), y / kBlockY, z / kBlockZ, w, n / kBlockY};
        const uint32_t see = block_seen_by(used, y % kBlockY, z % kBlockZ, diagonal != 0);
        for (uint32_t k = 0; k < 27u; ++k) block_raise(flags, see, at, k);
    }
    const unsigned long long sum = wg_sum_256((unsigned long long)__popc(s & 15u), smem);
    if (threadIdx.x == 0 && sum) atomicAdd(&counters[kCntSeeds / 2], sum);
}

__global__ void __launch_bounds__(256)
gd_final(const uint32_t* __restrict__ D, uint32_t* __restrict__ reach, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4], kmem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t d = D[i];
    store_ballot(reach, i, d != kNone);
    unsigned long long key = d != kNone ? ((unsigned long long)d << 32) | (0xFFFFFFFFu - (uint32_t)i) : 0ull;   // i < 2^30
    for (int s = 32; s >= 1; s >>= 1) key = max(key, (unsigned long long)__shfl_xor(key, s));
    if ((threadIdx.x & 63u) == 0) kmem[threadIdx.x >> 6] = key;
    const unsigned long long sum = wg_sum_256((unsigned long long)(d != kNone), smem);   // its barrier also publishes kmem[]
    if (threadIdx.x == 0 && sum) {
        atomicAdd(&counters[kCntReached / 2], sum);
        atomicMax(&counters[kCntKey / 2], max(max(kmem[0], kmem[1]), max(kmem[2], kmem[3])));
    }
}

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

template <int METRIC>
__global__ void __launch_bounds__(256)
gd_naive(const uint32_t* __restrict__ mask, uint32_t* D, uint32_t n, const uint32_t* prev, uint32_t* cur)
{
    if (round_skip(prev)) return;
    using W = Weights<METRIC>;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool changed = false;
    if ((mask[i >> 5] >> (i & 31u)) & 1u) {
        const uint32_t x = (uint32_t)(i % n), y = (uint32_t)((i / n) % n), z = (uint32_t)(i / ((size_t)n * n));
        const uint32_t old = D[i];
        uint32_t best = old;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1, steps = (dx != 0) + (dy != 0) + (dz != 0);
            if (steps == 0 || (steps > 1 && !W::diagonal)) continue;
            const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
            if (qx >= n || qy >= n || qz >= n) continue;             // outside the grid is outside M; a voxel outside M reads NONE
            best = min(best, gd_add(D[qx + (size_t)n * (qy + (size_t)n * qz)], steps == 1 ? W::w1 : steps == 2 ? W::w2 : W::w3));
        }
        if (best < old) {
            D[i] = best;
            changed = true;
        }
    }
    round_mark(changed, cur);
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

// column c of the window around the row at `row` (word offset of its column 0): own = the row's value, same = the minimum that reaches a
// voxel of the row at the same x (through the eight rows around it), side = the one that reaches the voxels at x - 1 and x + 1
template <int METRIC>
__device__ __forceinline__ void gd_column(const uint32_t* row, uint32_t c, uint32_t& own, uint32_t& same, uint32_t& side)
{
    using W = Weights<METRIC>;
    constexpr int P = (int)kRowPitch, Z = (int)(kHalo * kRowPitch);
    own = row[c];
    const uint32_t face = min(min(row[(int)c - P], row[(int)c + P]), min(row[(int)c - Z], row[(int)c + Z]));
    if constexpr (W::diagonal) {
        const uint32_t edge = min(min(row[(int)c - P - Z], row[(int)c + P - Z]), min(row[(int)c - P + Z], row[(int)c + P + Z]));
        same = min(gd_add(face, W::w1), gd_add(edge, W::w2));
        side = min(gd_add(own, W::w1), min(gd_add(face, W::w2), gd_add(edge, W::w3)));
    } else {
        same = gd_add(face, W::w1);
        side = gd_add(own, W::w1);
    }
}

template <int METRIC>
__global__ void __launch_bounds__(256)
gd_relax(const uint32_t* __restrict__ mask, uint32_t* D, const uint32_t* __restrict__ list, uint32_t* __restrict__ flags, uint32_t n)
{
    using W = Weights<METRIC>;
    __shared__ uint32_t tile[kHalo * kHalo * kRowPitch];
    __shared__ uint32_t lowered[256];                              // per row: the voxels that changed in this launch
    __shared__ uint32_t seen;                                      // the neighbour blocks whose halo holds a changed voxel
    const uint32_t t = threadIdx.x;
    const BlockAt at = block_at(list[blockIdx.x], n);
    stage_halo(tile, at, n, [&](uint32_t x, uint32_t y, uint32_t z, bool inside, uint32_t, uint32_t, uint32_t) {
        return inside ? D[x + (size_t)n * (y + (size_t)n * z)] : kNone;
    });
    if (t == 0) seen = 0u;
    const uint32_t ly = t & 15u, lz = t >> 4;
    const uint32_t m = mask[at.word(n, ly, lz)];
    uint32_t* row = tile_row(tile, ly, lz);
    __syncthreads();

    uint32_t chg = 0u;
    int still = 0;
#pragma unroll 1
    for (uint32_t sweep = 0; sweep < kGeoSweeps; ++sweep) {
        uint32_t now = 0u;
        if (m != 0u) {
            uint32_t v[32];
            uint32_t own, same, side, left, nown, nsame, nside;
            gd_column<METRIC>(row, 0u, own, same, left);
            gd_column<METRIC>(row, 1u, own, same, side);
#pragma unroll
            for (uint32_t x = 0; x < 32u; ++x) {
                gd_column<METRIC>(row, x + 2u, nown, nsame, nside);
                const uint32_t best = min(min(own, same), min(left, nside));
                const bool in = (m >> x) & 1u;
                v[x] = in ? best : kNone;
                now |= (in && best < own) ? 1u << x : 0u;
                left = side; own = nown; same = nsame; side = nside;
            }
#pragma unroll
            for (uint32_t x = 1; x < 32u; ++x) {                   // along the row: toward higher x, then toward lower x
                const uint32_t c = gd_add(v[x - 1u], W::w1);
                if (((m >> x) & 1u) && c < v[x]) { v[x] = c; now |= 1u << x; }
            }
#pragma unroll
            for (uint32_t k = 0; k < 31u; ++k) {
                const uint32_t x = 30u - k;
                const uint32_t c = gd_add(v[x + 1u], W::w1);
                if (((m >> x) & 1u) && c < v[x]) { v[x] = c; now |= 1u << x; }
            }
#pragma unroll
            for (uint32_t x = 0; x < 32u; ++x)
                if ((now >> x) & 1u) row[x + 1u] = v[x];
        }
        chg |= now;
        still = __syncthreads_or(now != 0u);
        if (!still) break;
    }

    lowered[t] = chg;
    const uint32_t see = block_seen_by(chg, ly, lz, W::diagonal) & ~(1u << 13);   // the neighbour blocks that see a changed voxel
    if (see) atomicOr(&seen, see);
    __syncthreads();
    store_lowered(lowered, at, n, [&](uint32_t, uint32_t, size_t i, uint32_t in_tile) { D[i] = tile[in_tile]; });
    if (t < 27u) block_raise(flags, seen | (still ? 1u << 13 : 0u), at, t);   // still changing at the cap: this block again
}

}  // namespace

// The caller has validated everything.  Blocks: the round flags (NAIVE) or the list length (TILED) are read back.
int launch_geodesic(vp_ctx* ctx, const Frame& f, const uint32_t* d_mask, const uint32_t* d_seeds, int metric, int algo, uint64_t* h_stats)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n, nblocks = block_count(n);
    const size_t voxels = (size_t)n * n * n;
    const unsigned wgs = (unsigned)(voxels / 256);
    ctx->gd.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->gd.dist, voxels * 4, false));
    VP_TRY(reserve(ctx, ctx->gd.reach, voxels / 8, false));
    VP_TRY(reserve(ctx, ctx->gd.aux, kAuxHead + (size_t)std::max(nblocks * 2u, 2u * kGeoBatch) * 4, false));
    VP_TRY(ctx->gd.host.need(kAuxHead / 8));
    uint32_t* D = (uint32_t*)ctx->gd.dist.ptr;
    uint32_t* counters = (uint32_t*)ctx->gd.aux.ptr;
    uint32_t* flags = block_flags(ctx->gd.aux.ptr);                      // TILED: block flags, then the list; NAIVE: the ring of round flags
    uint32_t* list = flags + nblocks;
    volatile uint32_t* host = (volatile uint32_t*)ctx->gd.host.p;

    VP_HIP(hipMemsetAsync(ctx->gd.aux.ptr, 0, kAuxHead + (size_t)(algo == VP_ALGO_TILED ? nblocks : 0u) * 4, st));
    {
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(gd_init, dim3(wgs / 4), dim3(256), 0, st, d_mask, d_seeds, (uint4*)D, n, algo == VP_ALGO_TILED ? flags : nullptr,
                           metric == VP_GEO_6 ? 0 : 1, (unsigned long long*)counters);
    }
    const auto relax = metric == VP_GEO_6 ? gd_relax<VP_GEO_6> : metric == VP_GEO_26 ? gd_relax<VP_GEO_26> : gd_relax<VP_GEO_CHAMFER>;
    const auto naive = metric == VP_GEO_6 ? gd_naive<VP_GEO_6> : metric == VP_GEO_26 ? gd_naive<VP_GEO_26> : gd_naive<VP_GEO_CHAMFER>;
    if (algo == VP_ALGO_TILED) {
        for (;;) {
            uint32_t active = 0;
            VP_TRY(list_active(ctx, flags, nblocks, list, counters + kCntActive, host, 4, &active));
            if (active == 0) break;                                // no block's halo or interior changed since it last ran: the fixed point
            ProfScope p(ctx, VP_K_MD_BRICK);
            hipLaunchKernelGGL(relax, dim3(active), dim3(256), 0, st, d_mask, D, (const uint32_t*)list, flags, n);
        }
    } else {
        // rounds until one lowers nothing: the fixed point
        VP_TRY(run_rounds(st, RoundRing{flags, kGeoBatch, host}, nullptr, nullptr, [&](uint32_t, const uint32_t* prev, uint32_t* cur) {
            ProfScope p(ctx, VP_K_MD_NAIVE);
            hipLaunchKernelGGL(naive, dim3(wgs), dim3(256), 0, st, d_mask, D, n, prev, cur);
        }));
    }
    {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(gd_final, dim3(wgs), dim3(256), 0, st, (const uint32_t*)D, (uint32_t*)ctx->gd.reach.ptr, (unsigned long long*)counters);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->gd.host, counters, 24, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint64_t* h64 = ctx->gd.host;
    const uint64_t reached = h64[kCntReached / 2], key = h64[kCntKey / 2];
    ctx->gd.stats[0] = reached ? h64[kCntSeeds / 2] : 0;
    ctx->gd.stats[1] = reached;
    ctx->gd.stats[2] = reached ? key >> 32 : 0;
    ctx->gd.stats[3] = reached ? 0xFFFFFFFFull - (key & 0xFFFFFFFFull) : 0;
    if (h_stats) std::copy(ctx->gd.stats, ctx->gd.stats + 4, h_stats);
    ctx->gd.n = n;
    return 0;
}

}  // namespace vp
