// watershed.hip -- seeded watershed and geodesic influence zones of a mask, whole-grid bit grids, for gfx950 (MI355X): vp_watershed
// (include/vphip.h).
//
// K holds one aligned 64-bit key per voxel, [T : 30 | source rank : 14 | label : 20]; 0 = "no label" (labels start at 1, so W is the low
// 20 bits).  T is a cumulative arrival time: 0 at the markers, base + hops for a voxel labelled in a level that started with
// base = the largest T stored before it.  Inside a level a neighbour u with T(u) <= base is a frozen source and CONTRIBUTES
// (base + 1, rank(u) from P, label(u)); any other labelled u contributes its stored key with T + 1; a voxel of the level's set A takes the
// minimum contribution of its neighbours whenever that is smaller than what it holds.  rank = the level in flood order, 0 .. 16383.
//   both   ws_pre     one workgroup per block of 32 x 16 x 16 voxels, BEFORE anything of the result is written: K from M and L0, min / max
//                     of P over M and the largest marker label in M (workgroup reductions, one atomic each), the markers used, the
//                     presence bitmap of the levels (bit (P / q) mod 16384: injective while the span is served; 2 KiB, gathered in LDS)
//                     and per block the lowest and highest P of its voxels of M.  The host reads head and bitmap back once, decides the
//                     refusals and walks the present levels only.
//          ws_final   one lane per voxel: W, the cut grid (one ballot = 64 bits = two words) and the two counts (wg_scan.h)
//   NAIVE  ws_naive   one lane per voxel, global memory only, in place; per level whole-grid launches repeat until one changes nothing
//                     (the flag ring of round_ring.h, restarted per level).
//   TILED  ws_relax   one workgroup per ACTIVE block (block_list.h), 256 lanes = one per x row.  The CONTRIBUTIONS of the block and a
//                     one-voxel halo are staged in LDS (the tile of block_list.h with values of 8 bytes = 90,720 B: one workgroup per
//                     CU of the 160 KiB).  A sweep: every lane walks its row with column minima over the eight (four) rows around
//                     it, left to right with the value it just made, then right to left in registers; barrier; the lanes store what
//                     they lowered; barrier.  Sweeps repeat until one lowers nothing or kWsSweeps ran; the changed keys are written back.
//          ws_first   the first list of a level: the blocks whose recorded [lo, hi] of P meets the level's range (a superset: a voxel that
//                     becomes labelled in level h lies behind a voxel of level h on its path, since level h - 1 ended at its fixed point).
//          block_list / block_seen_by (block_list.h) as in geodesic.hip; a block that stops at the cap re-lists itself.
// Levels are separated by kernel boundaries: level h + 1 starts after level h's list came back empty (its round changed nothing).  Inside a
// level the sources are frozen and (k, s, l) -> (k + 1, s, l) is isotone, so section 21's points hold word for word: (1) one writer per
// voxel; (2) keys only decrease (0 counts as +infinity); (3) every stored key is the key of a real path; (4) no torn key: K is read and
// written across workgroups with relaxed 64-bit atomic loads and stores (single 8-byte vector accesses, no read-modify-write; profiles/
// r21/resource_usage.txt), LDS only between barriers; (5) a block is rerun after every change in its tile or halo; (6) the smallest wrong
// key leads to a contradiction, so the fixed point of a level is unique whatever the order of execution.  T < 2^30: the hops of all
// levels together are at most the voxels labelled.  Every device loop has a compile-time bound.
#include "block_list.h"
#include "round_ring.h"
#include "vp_internal.h"

#include <algorithm>

namespace vp {

namespace {

constexpr uint32_t kWsSweeps = 64;   // TILED: sweeps over a block per launch at most (the tests read this line: their comb must outlast it)
constexpr uint32_t kWsBatch = 8;     // NAIVE: rounds enqueued between two read-backs of their flags
constexpr uint32_t kLabelBits = 20, kRankBits = 14, kTShift = kLabelBits + kRankBits;
constexpr uint32_t kLabelMask = VP_WS_LABEL_MAX, kBitmapWords = VP_WS_MAX_SPAN / 32;
constexpr unsigned long long kHop = 1ull << kTShift, kInf = ~0ull;
// the aux buffer: kAuxHead bytes of counters, the presence bitmap, then per block lo | hi | flag | list (or NAIVE's ring in place of the last two)
// counters, in 32-bit words: min P | max P | largest label | active blocks | largest T | - | markers used (u64) | labelled (u64) | |C| (u64)
constexpr uint32_t kCntMin = 0, kCntMax = 1, kCntLabel = 2, kCntActive = 3, kCntT = 4, kCntMarkers = 6, kCntLabelled = 8, kCntCut = 10;

struct Levels { uint32_t q, flip, edge; };                       // rank(p) = flip ? edge - p / q : p / q - edge  (edge = the last / first level)

__device__ __forceinline__ uint32_t ws_rank(const uint32_t* __restrict__ P, size_t i, Levels lv)
{
    if (!P) return 0u;
    const uint32_t l = P[i] / lv.q;
    return lv.flip ? lv.edge - l : l - lv.edge;
}

__device__ __forceinline__ unsigned long long ws_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ws_store(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// what the labelled or unlabelled voxel i with key k offers its neighbours in a level with base `base`
__device__ __forceinline__ unsigned long long ws_contribution(unsigned long long k, const uint32_t* __restrict__ P, size_t i, Levels lv, uint32_t base)
{
    if (k == 0ull) return kInf;
    if ((uint32_t)(k >> kTShift) > base) return k + kHop;
    return ((unsigned long long)(base + 1u) << kTShift) | ((unsigned long long)ws_rank(P, i, lv) << kLabelBits) | (k & kLabelMask);
}

// ---- both --------------------------------------------------------------------------------------------------------------------------

// one workgroup per block; lanes along x: element e = k * 256 + t is voxel x = e & 31 of row e >> 5 of the block
__global__ void __launch_bounds__(256)
ws_pre(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ markers, const uint32_t* __restrict__ P, unsigned long long* __restrict__ K,
       uint32_t n, uint32_t q, uint32_t* __restrict__ counters, uint32_t* __restrict__ bitmap, uint32_t* __restrict__ lohi)
{
    __shared__ uint32_t present[kBitmapWords];
    __shared__ uint32_t red[4][4];
    __shared__ unsigned long long smem[4];
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    const BlockAt at = block_at(b, n);
    present[t] = 0u;
    present[t + 256u] = 0u;
    __syncthreads();
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, top = 0u, used = 0u;
#pragma unroll 4
    for (uint32_t k = 0; k < 32u; ++k) {
        const uint32_t e = k * 256u + t, x = e & 31u, r = e >> 5;
        const size_t i = at.voxel(n, x, r & 15u, r >> 4);
        const bool in = (mask[i >> 5] >> x) & 1u;
        const uint32_t l = in ? markers[i] : 0u;
        K[i] = l <= kLabelMask ? l : 0ull;                           // a label above the bound is refused by the host: nothing is flooded then
        if (in) {
            const uint32_t p = P ? P[i] : 0u;
            lo = min(lo, p); hi = max(hi, p); top = max(top, l); used += l != 0u;
            const uint32_t level = (p / q) & (VP_WS_MAX_SPAN - 1u);
            atomicOr(&present[level >> 5], 1u << (level & 31u));
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor(lo, s)); hi = max(hi, (uint32_t)__shfl_xor(hi, s)); top = max(top, (uint32_t)__shfl_xor(top, s));
    }
    if ((t & 63u) == 0) { red[t >> 6][0] = lo; red[t >> 6][1] = hi; red[t >> 6][2] = top; }
    const unsigned long long sum = wg_sum_256((unsigned long long)used, smem);   // its barrier also publishes red[] and present[]
    if (t == 0) {
        lo = min(min(red[0][0], red[1][0]), min(red[2][0], red[3][0]));
        hi = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
        top = max(max(red[0][2], red[1][2]), max(red[2][2], red[3][2]));
        lohi[2u * b] = lo;
        lohi[2u * b + 1u] = hi;
        if (lo <= hi) { atomicMin(&counters[kCntMin], lo); atomicMax(&counters[kCntMax], hi); }
        if (top) atomicMax(&counters[kCntLabel], top);
        if (sum) atomicAdd((unsigned long long*)(counters + kCntMarkers), sum);
    }
    if (present[t]) atomicOr(&bitmap[t], present[t]);
    if (present[t + 256u]) atomicOr(&bitmap[t + 256u], present[t + 256u]);
}

template <int CONN>
__global__ void __launch_bounds__(256)
ws_final(const unsigned long long* __restrict__ K, uint32_t* __restrict__ W, uint32_t* __restrict__ cut, uint32_t n, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4], cmem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t x = (uint32_t)(i % n), y = (uint32_t)((i / n) % n), z = (uint32_t)(i / ((size_t)n * n));
    const uint32_t l = (uint32_t)K[i] & kLabelMask;
    W[i] = l;
    bool keep = l != 0u;
    if (keep) {
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1, steps = (dx != 0) + (dy != 0) + (dz != 0);
            if (steps == 0 || (steps > 1 && CONN == 6)) continue;
            const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
            if (qx >= n || qy >= n || qz >= n) continue;
            keep = keep && ((uint32_t)K[qx + (size_t)n * (qy + (size_t)n * qz)] & kLabelMask) <= l;
        }
    }
    store_ballot(cut, i, keep);
    const unsigned long long labelled = wg_sum_256((unsigned long long)(l != 0u), smem);
    const unsigned long long kept = wg_sum_256((unsigned long long)keep, cmem);
    if (threadIdx.x == 0) {
        if (labelled) atomicAdd(&counters[kCntLabelled / 2], labelled);
        if (kept) atomicAdd(&counters[kCntCut / 2], kept);
    }
}

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

template <int CONN>
__global__ void __launch_bounds__(256)
ws_naive(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ P, unsigned long long* K, uint32_t n, Levels lv, uint32_t rank, uint32_t base,
         const uint32_t* prev, uint32_t* cur, uint32_t* tmax)
{
    if (round_skip(prev)) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t stamp = 0u;                                           // T of the key stored, 0: none
    if ((mask[i >> 5] >> (i & 31u)) & 1u) {
        const unsigned long long old = ws_load(K + i);
        if ((old == 0ull || (uint32_t)(old >> kTShift) > base) && ws_rank(P, i, lv) <= rank) {
            const uint32_t x = (uint32_t)(i % n), y = (uint32_t)((i / n) % n), z = (uint32_t)(i / ((size_t)n * n));
            unsigned long long best = kInf;
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1, steps = (dx != 0) + (dy != 0) + (dz != 0);
                if (steps == 0 || (steps > 1 && CONN == 6)) continue;
                const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
                if (qx >= n || qy >= n || qz >= n) continue;         // outside the grid is outside M; a voxel outside M holds no label
                const size_t j = qx + (size_t)n * (qy + (size_t)n * qz);
                best = min(best, ws_contribution(ws_load(K + j), P, j, lv, base));
            }
            if (best != kInf && (old == 0ull || best < old)) {
                ws_store(K + i, best);
                stamp = (uint32_t)(best >> kTShift);
            }
        }
    }
    for (int s = 32; s >= 1; s >>= 1) stamp = max(stamp, (uint32_t)__shfl_xor(stamp, s));
    round_mark(stamp != 0u, cur);
    if (stamp && (threadIdx.x & 63u) == 0) atomicMax(tmax, stamp);
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
ws_first(const uint32_t* __restrict__ lohi, uint32_t nblocks, uint32_t plo, uint32_t phi, uint32_t* __restrict__ flags)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < nblocks && lohi[2u * b] <= phi && lohi[2u * b + 1u] >= plo) flags[b] = 1u;   // a block without a voxel of M holds lo > hi: never listed
}

// column c of the window around the row at `row`: own = the row's contribution, other = the minimum over the rows around it that are its
// neighbours (eight, or the four face rows)
template <int CONN>
__device__ __forceinline__ void ws_column(const unsigned long long* row, uint32_t c, unsigned long long& own, unsigned long long& other)
{
    constexpr int P = (int)kRowPitch, Z = (int)(kHalo * kRowPitch);
    own = row[c];
    other = min(min(row[(int)c - P], row[(int)c + P]), min(row[(int)c - Z], row[(int)c + Z]));
    if constexpr (CONN == 26)
        other = min(other, min(min(row[(int)c - P - Z], row[(int)c + P - Z]), min(row[(int)c - P + Z], row[(int)c + P + Z])));
}

template <int CONN>
__global__ void __launch_bounds__(256)
ws_relax(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ P, unsigned long long* K, const uint32_t* __restrict__ list,
         uint32_t* __restrict__ flags, uint32_t n, Levels lv, uint32_t rank, uint32_t base, uint32_t* tmax)
{
    __shared__ unsigned long long tile[kHalo * kHalo * kRowPitch];
    __shared__ uint32_t open[256];                                 // per row: the voxels of M whose level has come (the level's set A, once unlabelled)
    __shared__ uint32_t lowered[256];                              // per row: the voxels that changed in this launch
    __shared__ uint32_t seen, newest;                              // neighbour blocks whose halo holds a changed voxel; the largest T stored
    const uint32_t t = threadIdx.x;
    const BlockAt at = block_at(list[blockIdx.x], n);
    stage_halo(tile, at, n, [&](uint32_t x, uint32_t y, uint32_t z, bool inside, uint32_t, uint32_t, uint32_t) {
        if (!inside) return kInf;
        const size_t i = x + (size_t)n * (y + (size_t)n * z);
        return ws_contribution(ws_load(K + i), P, i, lv, base);
    });
#pragma unroll 4
    for (uint32_t k = 0; k < 32u; ++k) {                           // lanes along x: a wave makes the words of two rows by one ballot
        const uint32_t e = k * 256u + t, x = e & 31u, r = e >> 5;
        const size_t i = at.voxel(n, x, r & 15u, r >> 4);
        const bool in = ((mask[i >> 5] >> x) & 1u) && ws_rank(P, i, lv) <= rank;
        store_ballot(open, e, in);
    }
    if (t == 0) { seen = 0u; newest = 0u; }
    const uint32_t ly = t & 15u, lz = t >> 4;
    unsigned long long* row = tile_row(tile, ly, lz);
    __syncthreads();
    const uint32_t m = open[t];
    const unsigned long long frozen = (unsigned long long)(base + 1u);   // T of a frozen source's contribution, and of nothing else

    uint32_t chg = 0u;
    int still = 0;
#pragma unroll 1
    for (uint32_t sweep = 0; sweep < kWsSweeps; ++sweep) {
        uint32_t now = 0u;
        unsigned long long v[32];
        if (m != 0u) {
            unsigned long long own, other, left, nown, nother;
            ws_column<CONN>(row, 0u, own, other);
            left = CONN == 26 ? min(own, other) : own;
            ws_column<CONN>(row, 1u, own, other);
#pragma unroll
            for (uint32_t x = 0; x < 32u; ++x) {                   // toward higher x, with the value just made
                ws_column<CONN>(row, x + 2u, nown, nother);
                const unsigned long long best = min(other, min(left, CONN == 26 ? min(nown, nother) : nown));
                const bool can = ((m >> x) & 1u) && (own >> kTShift) != frozen;
                unsigned long long c = own;
                if (can && best != kInf && best + kHop < c) { c = best + kHop; now |= 1u << x; }
                v[x] = c;
                left = CONN == 26 ? min(c, other) : c;
                own = nown; other = nother;
            }
#pragma unroll
            for (uint32_t k = 0; k < 31u; ++k) {                   // toward lower x, in registers
                const uint32_t x = 30u - k;
                const bool can = ((m >> x) & 1u) && (v[x] >> kTShift) != frozen;
                if (can && v[x + 1u] != kInf && v[x + 1u] + kHop < v[x]) { v[x] = v[x + 1u] + kHop; now |= 1u << x; }
            }
        }
        __syncthreads();                                           // every read of this sweep is done
        if (now != 0u) {
#pragma unroll
            for (uint32_t x = 0; x < 32u; ++x)
                if ((now >> x) & 1u) row[x + 1u] = v[x];
        }
        chg |= now;
        still = __syncthreads_or(now != 0u);
        if (!still) break;
    }

    lowered[t] = chg;
    const uint32_t see = block_seen_by(chg, ly, lz, CONN == 26) & ~(1u << 13);   // the neighbour blocks that see a changed voxel
    if (see) atomicOr(&seen, see);
    __syncthreads();
    uint32_t stamp = 0u;
    store_lowered(lowered, at, n, [&](uint32_t, uint32_t, size_t i, uint32_t in_tile) {
        const unsigned long long key = tile[in_tile] - kHop;
        ws_store(K + i, key);
        stamp = max(stamp, (uint32_t)(key >> kTShift));
    });
    if (stamp) atomicMax(&newest, stamp);
    __syncthreads();
    if (t == 0 && newest) atomicMax(tmax, newest);
    if (t < 27u) block_raise(flags, seen | (still ? 1u << 13 : 0u), at, t);   // still changing at the cap: this block again
}

// the smallest quantum >= q whose levels of [lo, hi] span less than VP_WS_MAX_SPAN
uint32_t fitting_quantum(uint32_t lo, uint32_t hi, uint32_t q)
{
    uint32_t s = std::max(q, (hi - lo) / VP_WS_MAX_SPAN);
    if (s == 0) s = 1;
    while (hi / s - lo / s >= VP_WS_MAX_SPAN) ++s;
    return s;
}

}  // namespace

// The caller has validated everything but what only the data show.  Blocks: head and bitmap once, then the round flags (NAIVE) or the list
// length (TILED) with the largest T.
int launch_watershed(vp_ctx* ctx, const Frame& f, const uint32_t* d_mask, const uint32_t* d_markers, const uint32_t* d_priority, int order,
                     uint32_t quantum, int conn, int algo, uint64_t* h_stats)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n, nblocks = block_count(n);
    const size_t voxels = (size_t)n * n * n;
    const unsigned wgs = (unsigned)(voxels / 256);
    const uint32_t q = d_priority ? quantum : 1u;
    const size_t head = kAuxHead + kBitmapWords * 4;
    // the pre-pass writes scratch only: a refusal below leaves W, C and the statistics of the previous result as they were
    VP_TRY(reserve(ctx, ctx->wsd.keys, voxels * 8, false));
    VP_TRY(reserve(ctx, ctx->wsd.aux, head + (size_t)std::max(nblocks * 4u, nblocks * 2u + 2u * kWsBatch) * 4, false));
    VP_TRY(ctx->wsd.host.need((head + 2u * kWsBatch * 4) / 4));
    unsigned long long* K = (unsigned long long*)ctx->wsd.keys.ptr;
    uint32_t* counters = (uint32_t*)ctx->wsd.aux.ptr;
    uint32_t* bitmap = counters + kAuxHead / 4;
    uint32_t* lohi = bitmap + kBitmapWords;
    uint32_t* flags = lohi + 2u * nblocks;                         // TILED: block flags, then the list; NAIVE: the ring of round flags
    uint32_t* list = flags + nblocks;
    volatile uint32_t* host = (volatile uint32_t*)ctx->wsd.host.p;

    VP_HIP(hipMemsetAsync(counters, 0, head, st));
    VP_HIP(hipMemsetAsync(counters + kCntMin, 0xFF, 4, st));
    if (algo == VP_ALGO_TILED) VP_HIP(hipMemsetAsync(flags, 0, (size_t)nblocks * 4, st));
    {
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(ws_pre, dim3(nblocks), dim3(256), 0, st, d_mask, d_markers, d_priority, K, n, q, counters, bitmap, lohi);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->wsd.host, counters, head, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint32_t pmin = host[kCntMin], pmax = host[kCntMax], top = host[kCntLabel];
    const uint64_t used = ((const uint64_t*)ctx->wsd.host.p)[kCntMarkers / 2];
    const bool empty = pmin > pmax;
    if (top > VP_WS_LABEL_MAX) return set_error(VP_ERR_INVALID, "vp_watershed: marker label %u above VP_WS_LABEL_MAX = %u", top, (uint32_t)VP_WS_LABEL_MAX);
    const uint32_t first = empty ? 0u : pmin / q, last = empty ? 0u : pmax / q;
    if (last - first >= VP_WS_MAX_SPAN)
        return set_error(VP_ERR_INVALID, "vp_watershed: the levels span %llu, VP_WS_MAX_SPAN = %u: the smallest quantum that fits is %u",
                         (unsigned long long)(last - first) + 1ull, (uint32_t)VP_WS_MAX_SPAN, fitting_quantum(pmin, pmax, q));   // 2^32 levels at most
    std::vector<uint32_t> levels;                                  // the present levels in flood order
    if (!empty)
        for (uint32_t l = first;; ++l) {
            const uint32_t bit = l & (VP_WS_MAX_SPAN - 1u);
            if ((host[kAuxHead / 4 + (bit >> 5)] >> (bit & 31u)) & 1u) levels.push_back(l);
            if (l == last) break;
        }
    const bool flip = d_priority && order == VP_WS_DESCENDING;
    if (flip) std::reverse(levels.begin(), levels.end());
    const Levels lv{q, flip ? 1u : 0u, flip ? last : first};

    ctx->wsd.n = 0;                                                // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->wsd.labels, voxels * 4, false));
    VP_TRY(reserve(ctx, ctx->wsd.cut, voxels / 8, false));
    uint32_t base = 0;                                             // the largest T stored so far
    const auto naive = conn == VP_CONN_6 ? ws_naive<6> : ws_naive<26>;
    const auto relax = conn == VP_CONN_6 ? ws_relax<6> : ws_relax<26>;
    for (size_t at = 0; used != 0 && at < levels.size(); ++at) {
        const uint32_t level = levels[at], rank = flip ? last - level : level - first;
        if (algo == VP_ALGO_TILED) {
            {
                ProfScope p(ctx, VP_K_MD_SCAN);
                const uint64_t plo = (uint64_t)level * q, phi = std::min<uint64_t>(plo + q - 1u, 0xFFFFFFFFull);
                hipLaunchKernelGGL(ws_first, dim3((nblocks + 255u) / 256u), dim3(256), 0, st, lohi, nblocks, (uint32_t)plo, (uint32_t)phi, flags);
            }
            for (;;) {
                uint32_t active = 0;
                VP_TRY(list_active(ctx, flags, nblocks, list, counters + kCntActive, host, 8, &active));   // active blocks | largest T
                if (active == 0) { base = host[1]; break; }         // the level's fixed point: what it stored is frozen from now on
                ProfScope p(ctx, VP_K_MD_BRICK);
                hipLaunchKernelGGL(relax, dim3(active), dim3(256), 0, st, d_mask, d_priority, K, (const uint32_t*)list, flags, n, lv, rank, base, counters + kCntT);
            }
        } else {
            // rounds until one changes nothing: the level's fixed point; the largest T comes back with every batch of flags
            VP_TRY(run_rounds(st, RoundRing{flags, kWsBatch, host}, nullptr, counters + kCntT, [&](uint32_t, const uint32_t* prev, uint32_t* cur) {
                ProfScope p(ctx, VP_K_MD_NAIVE);
                hipLaunchKernelGGL(naive, dim3(wgs), dim3(256), 0, st, d_mask, d_priority, K, n, lv, rank, base, prev, cur, counters + kCntT);
            }));
            base = host[kWsBatch];
        }
    }
    {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(conn == VP_CONN_6 ? ws_final<6> : ws_final<26>, dim3(wgs), dim3(256), 0, st, (const unsigned long long*)K, (uint32_t*)ctx->wsd.labels.ptr,
                           (uint32_t*)ctx->wsd.cut.ptr, n, (unsigned long long*)counters);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->wsd.host, counters, kAuxHead, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint64_t* h64 = (const uint64_t*)ctx->wsd.host.p;
    ctx->wsd.stats[0] = used;
    ctx->wsd.stats[1] = h64[kCntLabelled / 2];
    ctx->wsd.stats[2] = levels.size();
    ctx->wsd.stats[3] = h64[kCntLabelled / 2] - h64[kCntCut / 2];
    if (h_stats) std::copy(ctx->wsd.stats, ctx->wsd.stats + 4, h_stats);
    ctx->wsd.n = n;
    return 0;
}

}  // namespace vp
