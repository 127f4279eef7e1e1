// reconstruct.hip -- grayscale geodesic reconstruction and h-extrema on whole grids, for gfx950 (MI355X): vp_reconstruct, vp_extrema
// (include/vphip.h).
//
// The kernels know one operator, reconstruction by dilation on WORK values: u(v) = v for VP_REC_DILATION, ~v for VP_REC_EROSION, 0 for both
// fields off the domain M.  R holds one uint32 per voxel: R0 = min(u(F), u(G)), then raised by pulls R[p] = min(g[p], max(R[p], R[q])) over
// the neighbours q of p, g = u(G), until nothing changes.  A work value g = 0 is a wall: R <= g keeps the voxel at 0, and 0 raises nobody --
// which is all that "not in M" means, so only the launches that read F and G look at the domain.
//   both   rc_init    one lane per four voxels (16 B per field): R0 from F, G and M, |M|, TILED's first block flags -- the blocks that hold
//                     a voxel with R0 < g: only such a voxel can ever change
//          rc_final   one lane per voxel: R back from work values (R ^ flip: the off-domain 0 becomes 0 or 0xFFFFFFFF by itself), the sum
//                     of R over M, the voxels with R != R0, the largest work value, reduced with wg_scan.h sums and one atomic per workgroup
//   NAIVE  rc_naive   one lane per voxel with room (R < g), global memory only, in place.  Whole-grid launches repeat until one changes
//                     nothing, kRecBatch rounds per read-back of their flags (round_ring.h).
//   TILED  rc_relax   one workgroup per ACTIVE block of 32 x 16 x 16 voxels, 256 lanes = one per x row.  The block's R and a one-voxel halo
//                     are staged in LDS (the tile of block_list.h: 45,360 B, three workgroups per CU), the lane's g row is 32 registers.
//                     One sweep: the lane walks along its row with a sliding window of column maxima over the eight rows around it (four
//                     for VP_CONN_6), r = min(g, max(r, left, columns)), then raises forward and backward along its own row in registers
//                     and stores what rose.  Sweeps repeat until one raises nothing in the block or kRecSweeps have run; then the values
//                     that changed are written back, by the lanes along x.
//          block_list (block_list.h)  a block whose face, edge or corner voxel rose raises the flags of exactly the neighbour blocks whose
//                     halo holds that voxel (face neighbours only for VP_CONN_6); a block still rising at the sweep cap raises its own; the
//                     host loop ends with the first empty list.
//   extrema ex_shift  one lane per four voxels: V = the scaled values (VP_EXT_SQRT16: floor(sqrt(256 v)), twenty compare-and-set steps in
//                     64-bit integers), and V -+ h saturating -- the marker of the reconstruction that gives H; again with h = 1 on H
//          ex_ballot  one lane per voxel: E = { H differs from the reconstruction of H -+ 1 under H }, one ballot per 64 voxels, |E| and the
//                     voxels of M with H != V
// Order-free, for both: (1) every voxel of R has one writer in any launch -- its own lane (NAIVE), the workgroup of its block, which the
// list names once (TILED).  (2) Values only rise: a value is stored only where it is larger than the one read.  (3) Every value ever stored
// is R0[p] or min(g[p], R[q]) for a stored R[q] and an allowed step, so by induction it is min(R0(q0), min of g along a real path q0 .. p)
// and <= the fixed point, which is the maximum of that over all paths.  (4) Aligned 32-bit loads and stores do not tear: a read of a
// neighbour's voxel during the neighbour's write sees the old or the new value, both lower bounds of that kind; inside a workgroup the same
// holds for LDS between two barriers.  (5) A block is run after every event that can raise a voxel of its interior: a voxel rises only if
// it has room (R < g) and a neighbour in its tile is larger; rc_init lists every block that holds a voxel with room, every later store
// is a raise, whose flags are set in the launch that makes it and read after the kernel boundary, and a block that stops at the cap
// re-lists itself.  A block that is never listed has no voxel with room from start to end.  NAIVE reruns everything.  (6) Hence when a launch
// changes nothing (NAIVE) or the list is empty (TILED) -- no store happened since every voxel of a block that was ever listed last evaluated
// its pull -- R[p] = min(g[p], max(R[p], max R[q])) holds at every voxel, and with (3) R is the least such field above R0: the unique fixed
// point, whatever the order of execution.
// No atomics on R.  Kernel boundaries are the only synchronisation between workgroups; every device loop has a compile-time bound.
#include "block_list.h"
#include "round_ring.h"
#include "vp_internal.h"

#include <algorithm>

namespace vp {

namespace {

constexpr uint32_t kRecSweeps = 64;  // TILED: sweeps over a block per launch at most (tests/test_reconstruct_gpu.py reads this line)
constexpr uint32_t kRecBatch = 8;    // NAIVE: rounds enqueued between two read-backs of their flags
// the counters in front of the flags, as 64-bit words: |M|, voxels with R != R0, the sum of R over M, the largest work value, |E|, voxels of M
// with H != V; then the 32-bit count of active blocks
constexpr uint32_t kCntDomain = 0, kCntChanged = 1, kCntSum = 2, kCntTop = 3, kCntExtrema = 4, kCntFlat = 5, kCntActive32 = 12;

// bits k .. k + 3 of the domain word that holds voxel 4 i: all ones without a domain
__device__ __forceinline__ uint32_t domain_nibble(const uint32_t* __restrict__ domain, size_t i)
{
    return domain ? (domain[i >> 3] >> ((uint32_t)(i & 7u) * 4u)) & 15u : 15u;
}
__device__ __forceinline__ uint32_t work(uint32_t v, uint32_t flip, uint32_t in) { return in ? v ^ flip : 0u; }

// ---- both --------------------------------------------------------------------------------------------------------------------------

// lane i serves voxels 4 i .. 4 i + 3.  n^3 / 4 is a multiple of 256: every workgroup is whole.  F may be R itself (vp_extrema builds its
// markers in place): each lane reads its four values before it writes them.
__global__ void __launch_bounds__(256)
rc_init(const uint32_t* __restrict__ domain, const uint4* F, const uint4* __restrict__ G, uint4* R, uint32_t n, uint32_t flip,
        uint32_t* __restrict__ flags, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t m = domain_nibble(domain, i);
    const uint4 f = F[i], g = G[i];
    const uint32_t g0 = work(g.x, flip, m & 1u), g1 = work(g.y, flip, m & 2u), g2 = work(g.z, flip, m & 4u), g3 = work(g.w, flip, m & 8u);
    const uint4 r = make_uint4(min(work(f.x, flip, m & 1u), g0), min(work(f.y, flip, m & 2u), g1), min(work(f.z, flip, m & 4u), g2),
                               min(work(f.w, flip, m & 8u), g3));
    R[i] = r;
    if (flags && (r.x < g0 || r.y < g1 || r.z < g2 || r.w < g3)) {
        const size_t v = i * 4;
        const uint32_t x = (uint32_t)(v % n), y = (uint32_t)((v / n) % n), z = (uint32_t)(v / ((size_t)n * n));
        flags[x / 32u + (n / 32u) * (y / kBlockY + (n / kBlockY) * (z / kBlockZ))] = 1u;
    }
    const unsigned long long sum = wg_sum_256((unsigned long long)__popc(m), smem);
    if (threadIdx.x == 0 && sum) atomicAdd(&counters[kCntDomain], sum);
}

// F == nullptr: the voxels with R != R0 are not counted (the marker was overwritten in place)
__global__ void __launch_bounds__(256)
rc_final(const uint32_t* __restrict__ domain, const uint32_t* __restrict__ F, const uint32_t* __restrict__ G, uint32_t* __restrict__ R,
         uint32_t flip, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4], cmem[4], tmem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t in = domain ? (domain[i >> 5] >> (i & 31u)) & 1u : 1u;
    const uint32_t w = R[i], real = w ^ flip;                     // off the domain w = 0: 0 or 0xFFFFFFFF
    R[i] = real;
    uint32_t changed = 0u;
    if (F && in) changed = w != min(F[i] ^ flip, G[i] ^ flip) ? 1u : 0u;
    unsigned long long top = w;
    for (int s = 32; s >= 1; s >>= 1) top = max(top, (unsigned long long)__shfl_xor(top, s));
    if ((threadIdx.x & 63u) == 0) tmem[threadIdx.x >> 6] = top;
    const unsigned long long sum = wg_sum_256((unsigned long long)(in ? real : 0u), smem);   // its barrier also publishes tmem[]
    const unsigned long long chg = wg_sum_256((unsigned long long)changed, cmem);
    if (threadIdx.x == 0) {
        if (sum) atomicAdd(&counters[kCntSum], sum);
        if (chg) atomicAdd(&counters[kCntChanged], chg);
        const unsigned long long t = max(max(tmem[0], tmem[1]), max(tmem[2], tmem[3]));
        if (t) atomicMax(&counters[kCntTop], t);
    }
}

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

template <int CONN>
__global__ void __launch_bounds__(256)
rc_naive(const uint32_t* __restrict__ domain, const uint32_t* __restrict__ G, uint32_t* R, uint32_t n, uint32_t flip, const uint32_t* prev,
         uint32_t* cur)
{
    if (round_skip(prev)) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t in = domain ? (domain[i >> 5] >> (i & 31u)) & 1u : 1u;
    const uint32_t g = work(G[i], flip, in), old = R[i];
    bool changed = false;
    if (old < g) {
        const uint32_t x = (uint32_t)(i % n), y = (uint32_t)((i / n) % n), z = (uint32_t)(i / ((size_t)n * n));
        uint32_t best = old;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1, steps = (dx != 0) + (dy != 0) + (dz != 0);
            if (steps == 0 || (steps > 1 && CONN == VP_CONN_6)) continue;
            const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
            if (qx >= n || qy >= n || qz >= n) continue;             // outside the grid is outside M: a work value of 0
            best = max(best, R[qx + (size_t)n * (qy + (size_t)n * qz)]);
        }
        best = min(best, g);
        if (best > old) {
            R[i] = best;
            changed = true;
        }
    }
    round_mark(changed, cur);
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

// column c of the window around the row at `row` (word offset of its column 0): own = the row's value, same = the maximum that reaches a
// voxel of the row at the same x (through the rows around it), side = the one that reaches the voxels at x - 1 and x + 1
template <int CONN>
__device__ __forceinline__ void rc_column(const uint32_t* row, uint32_t c, uint32_t& own, uint32_t& same, uint32_t& side)
{
    constexpr int P = (int)kRowPitch, Z = (int)(kHalo * kRowPitch);
    own = row[c];
    const uint32_t face = max(max(row[(int)c - P], row[(int)c + P]), max(row[(int)c - Z], row[(int)c + Z]));
    if constexpr (CONN == VP_CONN_26) {
        const uint32_t edge = max(max(row[(int)c - P - Z], row[(int)c + P - Z]), max(row[(int)c - P + Z], row[(int)c + P + Z]));
        same = max(face, edge);
        side = max(own, same);
    } else {
        same = face;
        side = own;
    }
}

template <int CONN>
__global__ void __launch_bounds__(256)
rc_relax(const uint32_t* __restrict__ domain, const uint32_t* __restrict__ G, uint32_t* R, const uint32_t* __restrict__ list,
         uint32_t* __restrict__ flags, uint32_t n, uint32_t flip)
{
    __shared__ uint32_t tile[kHalo * kHalo * kRowPitch];
    __shared__ uint32_t raised[256];                               // per row: the voxels that changed in this launch
    __shared__ uint32_t seen;                                      // the neighbour blocks whose halo holds a changed voxel
    const uint32_t t = threadIdx.x;
    const BlockAt at = block_at(list[blockIdx.x], n);
    stage_halo(tile, at, n, [&](uint32_t x, uint32_t y, uint32_t z, bool inside, uint32_t, uint32_t, uint32_t) {
        return inside ? R[x + (size_t)n * (y + (size_t)n * z)] : 0u;
    });
    if (t == 0) seen = 0u;
    const uint32_t ly = t & 15u, lz = t >> 4;
    const uint32_t m = domain ? domain[at.word(n, ly, lz)] : 0xFFFFFFFFu;
    uint32_t g[32];                                                // the lane's row of work G: 128 contiguous bytes
    {
        const uint4* grow = reinterpret_cast<const uint4*>(G + at.voxel(n, 0u, ly, lz));
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint4 q = grow[k];
            g[4u * k] = work(q.x, flip, (m >> (4u * k)) & 1u);
            g[4u * k + 1u] = work(q.y, flip, (m >> (4u * k + 1u)) & 1u);
            g[4u * k + 2u] = work(q.z, flip, (m >> (4u * k + 2u)) & 1u);
            g[4u * k + 3u] = work(q.w, flip, (m >> (4u * k + 3u)) & 1u);
        }
    }
    uint32_t* row = tile_row(tile, ly, lz);
    __syncthreads();

    uint32_t chg = 0u, room = m;                                   // room: the voxels of the row that may still rise (all of M until looked at)
    int still = 0;
#pragma unroll 1
    for (uint32_t sweep = 0; sweep < kRecSweeps; ++sweep) {
        uint32_t now = 0u;
        if (room != 0u) {
            uint32_t v[32];
            uint32_t own, same, side, left, nown, nsame, nside;
            rc_column<CONN>(row, 0u, own, same, left);
            rc_column<CONN>(row, 1u, own, same, side);
#pragma unroll
            for (uint32_t x = 0; x < 32u; ++x) {
                rc_column<CONN>(row, x + 2u, nown, nsame, nside);
                const uint32_t best = min(g[x], max(max(own, same), max(left, nside)));
                const bool up = best > own;                        // own <= g always: best < own cannot happen
                v[x] = up ? best : own;
                now |= up ? 1u << x : 0u;
                left = side; own = nown; same = nsame; side = nside;
            }
#pragma unroll
            for (uint32_t x = 1; x < 32u; ++x) {                   // along the row: toward higher x, then toward lower x
                const uint32_t c = min(g[x], v[x - 1u]);
                if (c > v[x]) { v[x] = c; now |= 1u << x; }
            }
#pragma unroll
            for (uint32_t k = 0; k < 31u; ++k) {
                const uint32_t x = 30u - k;
                const uint32_t c = min(g[x], v[x + 1u]);
                if (c > v[x]) { v[x] = c; now |= 1u << x; }
            }
            room = 0u;
#pragma unroll
            for (uint32_t x = 0; x < 32u; ++x) {
                if ((now >> x) & 1u) row[x + 1u] = v[x];
                room |= v[x] < g[x] ? 1u << x : 0u;
            }
        }
        chg |= now;
        still = __syncthreads_or(now != 0u);
        if (!still) break;
    }

    raised[t] = chg;
    const uint32_t see = block_seen_by(chg, ly, lz, CONN == VP_CONN_26) & ~(1u << 13);   // the neighbour blocks that see a changed voxel
    if (see) atomicOr(&seen, see);
    __syncthreads();
    store_lowered(raised, at, n, [&](uint32_t, uint32_t, size_t i, uint32_t in_tile) { R[i] = tile[in_tile]; });
    if (t < 27u) block_raise(flags, seen | (still ? 1u << 13 : 0u), at, t);   // still rising at the cap: this block again
}

// ---- extrema -------------------------------------------------------------------------------------------------------------------------

// floor(sqrt(256 v)) for every uint32: the result is below 2^20, built bit by bit in 64-bit integers
__device__ __forceinline__ uint32_t isqrt16(uint32_t v)
{
    const unsigned long long x = (unsigned long long)v << 8;
    uint32_t r = 0u;
#pragma unroll
    for (int b = 19; b >= 0; --b) {
        const uint32_t c = r | (1u << b);
        if ((unsigned long long)c * c <= x) r = c;
    }
    return r;
}

__device__ __forceinline__ uint32_t ex_shift1(uint32_t v, uint32_t h, int up) { return up ? (v > ~h ? 0xFFFFFFFFu : v + h) : (v < h ? 0u : v - h); }

// lane i serves voxels 4 i .. 4 i + 3: scaled (if asked for) = the scaled values, shifted = scaled - h (up == 0) or + h, saturating
__global__ void __launch_bounds__(256)
ex_shift(const uint4* __restrict__ values, uint4* __restrict__ scaled, uint4* __restrict__ shifted, int sqrt16, uint32_t h, int up)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint4 v = values[i];
    if (sqrt16) v = make_uint4(isqrt16(v.x), isqrt16(v.y), isqrt16(v.z), isqrt16(v.w));
    if (scaled) scaled[i] = v;
    shifted[i] = make_uint4(ex_shift1(v.x, h, up), ex_shift1(v.y, h, up), ex_shift1(v.z, h, up), ex_shift1(v.w, h, up));
}

// S = the reconstruction of H -+ 1 under H: bit = H above S (maxima) or below it (minima); off the domain both read the same
__global__ void __launch_bounds__(256)
ex_ballot(const uint32_t* __restrict__ domain, const uint32_t* __restrict__ V, const uint32_t* __restrict__ H, const uint32_t* __restrict__ S,
          uint32_t* __restrict__ E, int minima, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4], fmem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t in = domain ? (domain[i >> 5] >> (i & 31u)) & 1u : 1u;
    const uint32_t h = H[i], s = S[i];
    const bool bit = minima ? h < s : h > s;
    store_ballot(E, i, bit);
    const unsigned long long sum = wg_sum_256((unsigned long long)bit, smem);
    const unsigned long long flat = wg_sum_256((unsigned long long)(in && h != V[i]), fmem);
    if (threadIdx.x == 0) {
        if (sum) atomicAdd(&counters[kCntExtrema], sum);
        if (flat) atomicAdd(&counters[kCntFlat], flat);
    }
}

// One reconstruction: R from F under G on `domain` (null: every voxel), in work values while it runs.  F may be R (then the voxels with
// R != R0 are not counted).  aux: kAuxHead bytes of counters, then the block flags and the list (TILED) or the ring of round flags (NAIVE).
// Blocks: the round flags or the list length are read back, and the four counters at the end.
struct RecJob {
    uint32_t n;
    const uint32_t *domain, *F, *G;
    uint32_t* R;
    int mode, conn, algo;
};
size_t rec_aux_bytes(uint32_t n) { return kAuxHead + (size_t)std::max(block_count(n) * 2u, 2u * kRecBatch) * 4; }

int run_reconstruct(vp_ctx* ctx, const RecJob& j, void* aux, uint64_t* host, uint64_t* stats)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = j.n, nblocks = block_count(n), flip = j.mode == VP_REC_EROSION ? 0xFFFFFFFFu : 0u;
    const unsigned wgs = (unsigned)((size_t)n * n * n / 256);
    unsigned long long* counters = (unsigned long long*)aux;
    uint32_t* flags = block_flags(aux);
    uint32_t* list = flags + nblocks;
    const bool tiled = j.algo == VP_ALGO_TILED, in_place = j.F == j.R;

    VP_HIP(hipMemsetAsync(aux, 0, kAuxHead + (size_t)(tiled ? nblocks : 0u) * 4, st));
    {
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(rc_init, dim3(wgs / 4), dim3(256), 0, st, j.domain, (const uint4*)j.F, (const uint4*)j.G, (uint4*)j.R, n, flip,
                           tiled ? flags : nullptr, counters);
    }
    if (tiled) {
        const auto relax = j.conn == VP_CONN_6 ? rc_relax<VP_CONN_6> : rc_relax<VP_CONN_26>;
        for (;;) {
            uint32_t active = 0;
            VP_TRY(list_active(ctx, flags, nblocks, list, (uint32_t*)aux + kCntActive32, (volatile uint32_t*)host, 4, &active));
            if (active == 0) break;                                // no block holds a voxel that rose or could rise since it last ran: the fixed point
            ProfScope p(ctx, VP_K_MD_BRICK);
            hipLaunchKernelGGL(relax, dim3(active), dim3(256), 0, st, j.domain, j.G, j.R, (const uint32_t*)list, flags, n, flip);
        }
    } else {
        const auto naive = j.conn == VP_CONN_6 ? rc_naive<VP_CONN_6> : rc_naive<VP_CONN_26>;
        // rounds until one raises nothing: the fixed point
        VP_TRY(run_rounds(st, RoundRing{flags, kRecBatch, (volatile uint32_t*)host}, nullptr, nullptr,
                          [&](uint32_t, const uint32_t* prev, uint32_t* cur) {
                              ProfScope p(ctx, VP_K_MD_NAIVE);
                              hipLaunchKernelGGL(naive, dim3(wgs), dim3(256), 0, st, j.domain, j.G, j.R, n, flip, prev, cur);
                          }));
    }
    {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(rc_final, dim3(wgs), dim3(256), 0, st, j.domain, in_place ? nullptr : j.F, j.G, j.R, flip, counters);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(host, counters, 32, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint64_t domain = host[kCntDomain];
    stats[0] = domain;
    stats[1] = host[kCntChanged];
    stats[2] = host[kCntSum];
    stats[3] = domain ? (uint32_t)host[kCntTop] ^ flip : 0;       // erosion: the smallest R
    return 0;
}

}  // namespace

// The caller has validated everything.
int launch_reconstruct(vp_ctx* ctx, const Frame& f, const uint32_t* d_domain, const uint32_t* d_marker, const uint32_t* d_mask, int mode, int conn,
                       int algo, uint64_t* h_stats)
{
    const uint32_t n = f.n;
    ctx->rc.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->rc.field, (size_t)n * n * n * 4, false));
    VP_TRY(reserve(ctx, ctx->rc.aux, rec_aux_bytes(n), false));
    VP_TRY(ctx->rc.host.need(kAuxHead / 8));
    VP_TRY(run_reconstruct(ctx, RecJob{n, d_domain, d_marker, d_mask, (uint32_t*)ctx->rc.field.ptr, mode, conn, algo}, ctx->rc.aux.ptr,
                           ctx->rc.host, ctx->rc.stats));
    if (h_stats) std::copy(ctx->rc.stats, ctx->rc.stats + 4, h_stats);
    ctx->rc.n = n;
    return 0;
}

int launch_extrema(vp_ctx* ctx, const Frame& f, const uint32_t* d_domain, const uint32_t* d_values, int kind, int scale, uint32_t h, int conn,
                   int algo, uint64_t* h_stats)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n;
    const size_t voxels = (size_t)n * n * n;
    const unsigned wgs = (unsigned)(voxels / 256);
    const int minima = kind == VP_EXT_MINIMA ? 1 : 0, mode = minima ? VP_REC_EROSION : VP_REC_DILATION;
    ctx->ex.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->ex.scaled, voxels * 4, false));
    VP_TRY(reserve(ctx, ctx->ex.flat, voxels * 4, false));
    VP_TRY(reserve(ctx, ctx->ex.extrema, voxels / 8, false));
    VP_TRY(reserve(ctx, ctx->ex.tmp, voxels * 4, false));
    VP_TRY(reserve(ctx, ctx->ex.aux, rec_aux_bytes(n), false));
    VP_TRY(ctx->ex.host.need(kAuxHead / 8));
    uint32_t *V = (uint32_t*)ctx->ex.scaled.ptr, *H = (uint32_t*)ctx->ex.flat.ptr, *S = (uint32_t*)ctx->ex.tmp.ptr;
    unsigned long long* counters = (unsigned long long*)ctx->ex.aux.ptr;
    uint64_t first[4], second[4];

    {
        ProfScope p(ctx, VP_K_MD_FILL);                            // V and the marker V -+ h, in H's own buffer
        hipLaunchKernelGGL(ex_shift, dim3(wgs / 4), dim3(256), 0, st, (const uint4*)d_values, (uint4*)V, (uint4*)H, scale == VP_EXT_SQRT16 ? 1 : 0, h, minima);
    }
    VP_TRY(run_reconstruct(ctx, RecJob{n, d_domain, H, V, H, mode, conn, algo}, ctx->ex.aux.ptr, ctx->ex.host, first));
    {
        ProfScope p(ctx, VP_K_MD_FILL);                            // the marker H -+ 1 of the second reconstruction, in scratch
        hipLaunchKernelGGL(ex_shift, dim3(wgs / 4), dim3(256), 0, st, (const uint4*)H, (uint4*)nullptr, (uint4*)S, 0, 1u, minima);
    }
    VP_TRY(run_reconstruct(ctx, RecJob{n, d_domain, S, H, S, mode, conn, algo}, ctx->ex.aux.ptr, ctx->ex.host, second));
    VP_HIP(hipMemsetAsync(counters + kCntExtrema, 0, 16, st));
    {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(ex_ballot, dim3(wgs), dim3(256), 0, st, d_domain, (const uint32_t*)V, (const uint32_t*)H, (const uint32_t*)S,
                           (uint32_t*)ctx->ex.extrema.ptr, minima, counters);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->ex.host, counters + kCntExtrema, 16, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint64_t* h64 = ctx->ex.host;
    ctx->ex.stats[0] = first[0];
    ctx->ex.stats[1] = h64[0];
    ctx->ex.stats[2] = first[3];
    ctx->ex.stats[3] = h64[1];
    if (h_stats) std::copy(ctx->ex.stats, ctx->ex.stats + 4, h_stats);
    ctx->ex.n = n;
    return 0;
}

}  // namespace vp
