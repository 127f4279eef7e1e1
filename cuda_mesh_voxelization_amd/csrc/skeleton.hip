// skeleton.hip -- topological thinning of a whole-grid bit grid for gfx950 (MI355X): vp_skeleton and the table of simple neighbourhoods
// (include/vphip.h).
//
// One iteration = one border-mark launch and eight sub-iteration launches, s = 0 .. 7 = (x & 1) | (y & 1) << 1 | (z & 1) << 2.  Two voxels
// of one subfield are never 26-neighbours, so the deletions of one launch are independent of each other and of the order of execution.
//   NAIVE  sk_border_naive  one lane per word: B = S & ~anchor & ~(all six face neighbours set), taken from the grid at the iteration's start
//          sk_sub_naive     one lane per word of 32 voxels, global memory only: the words of the wrong y / z parity are copied, the others
//                           examine their candidate bits one by one with the plain simple() and write the word into the OTHER grid (eight
//                           launches: the result is back in the first).  The deleted count is read back after every iteration.
//   TILED  sk_mark_nonempty / block_list (block_list.h)   the list of active blocks: a block of 32 x 16 x 16 voxels is active when it or a
//                           26-neighbour block lost a voxel in the previous iteration (every non-empty block in the first).  A block
//                           that lost a voxel raises the flags of its 27 blocks.  The list length comes back with the deleted count, so
//                           every launch has exactly one workgroup per active block.
//          sk_border_tiled  the border words of the active blocks
//          sk_sub_tiled     one workgroup per active block, 256 lanes = one per word.  The block's rows and a one-voxel halo are staged
//                           in LDS as 34-bit rows (bit 0 = x - 1 from the word before, bit 33 = x + 32 from the word after: the fetch
//                           across word boundaries happens once, here).  The candidates -- at most 16 per word, in a quarter of the
//                           rows -- are ranked over the workgroup (wg_exclusive_256) and written to an LDS list; then every lane takes
//                           one candidate per round (four rounds at most), assembles the 27-bit mask from nine three-bit row windows
//                           and runs the shift form of simple(); deletions are ORed into a per-word LDS mask and the owner of the word
//                           writes it back.
// In-place update (TILED): in sub-iteration s a word is written only by the lane that owns it, and only its subfield-s bits change.  A
// reader uses a neighbour's bits only as the 26 neighbours of a subfield-s voxel, none of which is of subfield s; a staged halo may
// therefore hold either the old or the new value of a neighbour's subfield-s bit without any effect.  Aligned 32-bit stores do not tear.
// Every device loop has a compile-time bound; the host loop runs one iteration per round and ends with the first that deletes nothing.
#include <algorithm>
#include <thread>
#include <vector>

#include "block_list.h"
#include "skeleton_simple.h"
#include "vp_internal.h"

namespace vp {

namespace {

// the counters in front of the block flags (kAuxHead bytes): active blocks | deleted | - | - | voxels left (u64); kCnt* = where each starts,
// in 32-bit words.  The rows of a block and its halo are staged as kHalo x kHalo 34-bit rows (block_list.h: one lane per word).
constexpr uint32_t kCntActive = 0, kCntDeleted = 1, kCntLeft = 4;

// the row of word xw at (y, z) with its two x neighbours: bit 0 = voxel 32 xw - 1, bits 1 .. 32 the word, bit 33 = voxel 32 xw + 32;
// rows and voxels outside the grid are unset
__device__ __forceinline__ uint64_t sk_row(const uint32_t* __restrict__ g, uint32_t n, uint32_t w, uint32_t xw, int y, int z)
{
    if ((uint32_t)y >= n || (uint32_t)z >= n) return 0ull;
    const size_t i = xw + (size_t)w * ((size_t)y + (size_t)n * (size_t)z);
    const uint32_t cur = g[i];
    const uint32_t lo = xw ? g[i - 1] >> 31 : 0u;
    const uint32_t hi = xw + 1u < w ? g[i + 1] & 1u : 0u;
    return (uint64_t)lo | ((uint64_t)cur << 1) | ((uint64_t)hi << 33);
}

__device__ __forceinline__ uint32_t sk_border_word(const uint32_t* __restrict__ g, const uint32_t* __restrict__ anchor, uint32_t n, uint32_t w,
                                                   uint32_t xw, uint32_t y, uint32_t z)
{
    const size_t i = xw + (size_t)w * ((size_t)y + (size_t)n * (size_t)z), dz = (size_t)w * n;
    const uint32_t cur = g[i];
    if (cur == 0u) return 0u;
    const uint32_t xm = (cur << 1) | (xw ? g[i - 1] >> 31 : 0u), xp = (cur >> 1) | (xw + 1u < w ? g[i + 1] << 31 : 0u);
    const uint32_t ym = y ? g[i - w] : 0u, yp = y + 1u < n ? g[i + w] : 0u;
    const uint32_t zm = z ? g[i - dz] : 0u, zp = z + 1u < n ? g[i + dz] : 0u;
    return cur & ~(xm & xp & ym & yp & zm & zp) & ~(anchor ? anchor[i] : 0u);
}

// the neighbourhood of voxel x of the centre row from nine rows, r[dy + 3 dz]
__device__ __forceinline__ uint32_t sk_mask_at(const uint64_t (&r)[9], uint32_t x)
{
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < 9; ++k) m |= ((uint32_t)(r[k] >> x) & 7u) << (3 * k);
    return m;
}

__device__ __forceinline__ uint32_t sk_xmask(uint32_t s) { return (s & 1u) ? 0xAAAAAAAAu : 0x55555555u; }

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

// nwords is a multiple of 256 (n >= 32): every workgroup is whole
__global__ void __launch_bounds__(256)
sk_border_naive(const uint32_t* __restrict__ g, const uint32_t* __restrict__ anchor, uint32_t* __restrict__ border, uint32_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = n / 32, xw = (uint32_t)(i % w), y = (uint32_t)((i / w) % n), z = (uint32_t)(i / ((size_t)w * n));
    border[i] = sk_border_word(g, anchor, n, w, xw, y, z);
}

__global__ void __launch_bounds__(256)
sk_sub_naive(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint32_t* __restrict__ border, uint32_t n, uint32_t s, int mode,
             uint32_t* __restrict__ deleted)
{
    __shared__ uint32_t smem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = n / 32, xw = (uint32_t)(i % w), y = (uint32_t)((i / w) % n), z = (uint32_t)(i / ((size_t)w * n));
    const uint32_t cur = src[i];
    uint32_t cand = 0u, del = 0u;
    if ((y & 1u) == ((s >> 1) & 1u) && (z & 1u) == (s >> 2) && cur != 0u) cand = cur & border[i] & sk_xmask(s);
    if (cand) {
        uint64_t r[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = sk_row(src, n, w, xw, (int)y + k % 3 - 1, (int)z + k / 3 - 1);
        for (int k = 0; k < 16 && cand != 0u; ++k) {
            const uint32_t x = (uint32_t)__builtin_ctz(cand);
            cand &= cand - 1u;
            if (sk_deletable<false>(sk_mask_at(r, x), mode)) del |= 1u << x;
        }
    }
    dst[i] = cur & ~del;
    const uint32_t sum = wg_sum_256((uint32_t)__popc(del), smem);
    if (threadIdx.x == 0 && sum) atomicAdd(deleted, sum);
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

// one lane per word: the block of a non-empty word is active in the first iteration (plain stores of the same value)
__global__ void __launch_bounds__(256)
sk_mark_nonempty(const uint32_t* __restrict__ g, uint32_t n, uint32_t* __restrict__ flags)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g[i] == 0u) return;
    const uint32_t w = n / 32, nb = n / kBlockY, xw = (uint32_t)(i % w), y = (uint32_t)((i / w) % n), z = (uint32_t)(i / ((size_t)w * n));
    flags[xw + w * (y / kBlockY + nb * (z / kBlockZ))] = 1u;
}

__global__ void __launch_bounds__(256)
sk_border_tiled(const uint32_t* __restrict__ g, const uint32_t* __restrict__ anchor, uint32_t* __restrict__ border, const uint32_t* __restrict__ list,
                uint32_t n)
{
    const BlockAt at = block_at(list[blockIdx.x], n);
    const uint32_t ly = threadIdx.x & 15u, lz = threadIdx.x >> 4;
    border[at.word(n, ly, lz)] = sk_border_word(g, anchor, n, at.w, at.bx, at.y0() + ly, at.z0() + lz);
}

__global__ void __launch_bounds__(256)
sk_sub_tiled(uint32_t* __restrict__ g, const uint32_t* __restrict__ border, const uint32_t* __restrict__ list, uint32_t* __restrict__ flags,
             uint32_t n, uint32_t s, int mode, uint32_t* __restrict__ deleted)
{
    __shared__ uint64_t rows[kHalo * kHalo];
    __shared__ uint32_t del[256];
    __shared__ uint16_t cands[1024];                               // (lane << 5) | x of every candidate: 64 rows of the parity x 16 bits
    __shared__ uint32_t smem[4];
    const uint32_t t = threadIdx.x;
    const BlockAt at = block_at(list[blockIdx.x], n);
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {
        const uint32_t j = t + 256u * r;
        if (j < kHalo * kHalo) rows[j] = sk_row(g, n, at.w, at.bx, (int)(at.y0() + j % kHalo) - 1, (int)(at.z0() + j / kHalo) - 1);
    }
    del[t] = 0u;
    const uint32_t ly = t & 15u, lz = t >> 4, y = at.y0() + ly, z = at.z0() + lz;
    const size_t i = at.word(n, ly, lz);
    __syncthreads();
    const uint32_t own = (uint32_t)(rows[(lz + 1u) * kHalo + ly + 1u] >> 1);
    uint32_t cand = 0u;
    if ((y & 1u) == ((s >> 1) & 1u) && (z & 1u) == (s >> 2) && own != 0u) cand = own & border[i] & sk_xmask(s);
    uint32_t total = 0u;
    uint32_t put = wg_exclusive_256((uint32_t)__popc(cand), smem, &total);
    for (int k = 0; k < 16 && cand != 0u; ++k) {
        cands[put++] = (uint16_t)((t << 5) | (uint32_t)__builtin_ctz(cand));
        cand &= cand - 1u;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t j = r * 256u + t;
        if (j < total) {
            const uint32_t e = cands[j], x = e & 31u, lane = e >> 5, cy = lane & 15u, cz = lane >> 4;
            uint64_t r9[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) r9[k] = rows[(cz + k / 3) * kHalo + cy + k % 3];
            if (sk_deletable<true>(sk_mask_at(r9, x), mode)) atomicOr(&del[lane], 1u << x);
        }
    }
    __syncthreads();
    const uint32_t d = del[t];
    if (d) g[i] = own & ~d;
    const uint32_t sum = wg_sum_256((uint32_t)__popc(d), smem);
    if (sum == 0u) return;
    if (t == 0) atomicAdd(deleted, sum);
    if (t < 27u) block_raise(flags, ~0u, at, t);                   // this block and its 26 neighbours are active in the next iteration
}

// ---- both --------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
sk_count(const uint32_t* __restrict__ g, unsigned long long* __restrict__ counter)
{
    __shared__ unsigned long long smem[4];
    const unsigned long long s = wg_sum_256((unsigned long long)__popc(g[(size_t)blockIdx.x * 256 + threadIdx.x]), smem);
    if (threadIdx.x == 0 && s) atomicAdd(counter, s);
}

// one lane per word of the table: bit c = simple(sk_mask_of_index(c))
template <bool SHIFT>
__global__ void __launch_bounds__(256)
sk_table(uint32_t* __restrict__ table)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t bits = 0u;
    for (uint32_t k = 0; k < 32u; ++k) {
        const uint32_t m = sk_mask_of_index(i * 32u + k);
        bits |= ((SHIFT ? sk_simple_shift(m) : sk_simple_plain(m)) ? 1u : 0u) << k;
    }
    table[i] = bits;
}

}  // namespace

// The caller has validated everything.  Blocks: the deleted count of every iteration is read back.
int launch_skeleton(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, const uint32_t* d_anchor, int mode, uint32_t max_iters, int algo,
                    uint64_t* h_stats)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n, nblocks = block_count(n);
    const size_t nwords = (size_t)n * n * n / 32;
    const unsigned wgs = (unsigned)(nwords / 256);
    ctx->sk.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(reserve(ctx, ctx->sk.grid, nwords * 4, false));
    VP_TRY(reserve(ctx, ctx->sk.border, nwords * 4, false));
    VP_TRY(reserve(ctx, ctx->sk.aux, block_aux_bytes(nblocks), false));
    if (algo == VP_ALGO_NAIVE) VP_TRY(reserve(ctx, ctx->sk.tmp, nwords * 4, false));
    VP_TRY(ctx->sk.host.need(kAuxHead / 8));
    uint32_t* grid = (uint32_t*)ctx->sk.grid.ptr;
    uint32_t* other = (uint32_t*)ctx->sk.tmp.ptr;
    uint32_t* border = (uint32_t*)ctx->sk.border.ptr;
    uint32_t* counters = (uint32_t*)ctx->sk.aux.ptr;
    uint32_t* flags = block_flags(ctx->sk.aux.ptr);
    uint32_t* list = flags + nblocks;
    volatile uint32_t* host = (volatile uint32_t*)ctx->sk.host.p;

    VP_HIP(hipMemsetAsync(ctx->sk.aux.ptr, 0, kAuxHead + (size_t)nblocks * 4, st));
    {
        ProfScope p(ctx, VP_K_SURFACE);
        VP_TRY(launch_stream_copy(ctx, grid, d_words, nwords * 4));
    }
    uint32_t active = 0;
    if (algo == VP_ALGO_TILED) {
        VP_TRY(list_active(ctx, flags, nblocks, list, counters + kCntActive, host, 4, &active,
                           [&] { hipLaunchKernelGGL(sk_mark_nonempty, dim3(wgs), dim3(256), 0, st, (const uint32_t*)grid, n, flags); }));
    }
    uint64_t iterations = 0, deleted = 0;
    while (max_iters == 0 || iterations < max_iters) {
        uint32_t lost = 0;
        if (algo == VP_ALGO_NAIVE) {
            VP_HIP(hipMemsetAsync(counters + kCntDeleted, 0, 4, st));
            {
                ProfScope p(ctx, VP_K_SURFACE);
                hipLaunchKernelGGL(sk_border_naive, dim3(wgs), dim3(256), 0, st, (const uint32_t*)grid, d_anchor, border, n);
            }
            for (uint32_t s = 0; s < 8; ++s) {
                ProfScope p(ctx, VP_K_MORPH_NAIVE);
                hipLaunchKernelGGL(sk_sub_naive, dim3(wgs), dim3(256), 0, st, (const uint32_t*)((s & 1u) ? other : grid), (s & 1u) ? grid : other,
                                   (const uint32_t*)border, n, s, mode, counters + kCntDeleted);
            }
            VP_HIP(hipGetLastError());
            VP_HIP(hipMemcpyAsync(ctx->sk.host, counters + kCntDeleted, 4, hipMemcpyDeviceToHost, st));
            VP_HIP(hipStreamSynchronize(st));
            lost = host[0];
        } else if (active) {
            VP_HIP(hipMemsetAsync(counters + kCntDeleted, 0, 4, st));
            {
                ProfScope p(ctx, VP_K_SURFACE);
                hipLaunchKernelGGL(sk_border_tiled, dim3(active), dim3(256), 0, st, (const uint32_t*)grid, d_anchor, border, (const uint32_t*)list, n);
            }
            for (uint32_t s = 0; s < 8; ++s) {
                ProfScope p(ctx, VP_K_MORPH);
                hipLaunchKernelGGL(sk_sub_tiled, dim3(active), dim3(256), 0, st, grid, (const uint32_t*)border, (const uint32_t*)list, flags, n, s,
                                   mode, counters + kCntDeleted);
            }
            VP_TRY(list_active(ctx, flags, nblocks, list, counters + kCntActive, host, 8, &active));   // active blocks | deleted
            lost = host[kCntDeleted];
        }
        ++iterations;
        deleted += lost;
        if (lost == 0) break;                                      // the state is a fixed point: every further iteration would delete nothing
    }
    VP_HIP(hipMemsetAsync(counters + kCntLeft, 0, 8, st));
    {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(sk_count, dim3(wgs), dim3(256), 0, st, (const uint32_t*)grid, (unsigned long long*)(counters + kCntLeft));
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->sk.host + 2, counters + kCntLeft, 8, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    ctx->sk.stats[0] = ctx->sk.host[2];
    ctx->sk.stats[1] = iterations;
    ctx->sk.stats[2] = deleted;
    if (h_stats) std::copy(ctx->sk.stats, ctx->sk.stats + 3, h_stats);
    ctx->sk.n = n;
    return 0;
}

// the table of the 2^26 neighbourhoods on the device (2^21 words at d_table): NAIVE the plain form, TILED the shift form
int launch_skeleton_table(vp_ctx* ctx, int algo, uint32_t* d_table)
{
    if (algo == VP_ALGO_NAIVE) {
        ProfScope p(ctx, VP_K_MD_NAIVE);
        hipLaunchKernelGGL(sk_table<false>, dim3(1u << 13), dim3(256), 0, ctx->stream, d_table);
    } else {
        ProfScope p(ctx, VP_K_MD_BRICK);
        hipLaunchKernelGGL(sk_table<true>, dim3(1u << 13), dim3(256), 0, ctx->stream, d_table);
    }
    VP_HIP(hipGetLastError());
    return 0;
}

// the same table on the CPU, words dealt to a few threads
void skeleton_table_cpu(int algo, uint32_t* h_table)
{
    const uint32_t threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            for (uint32_t i = t; i < (1u << 21); i += threads) {
                uint32_t bits = 0u;
                for (uint32_t k = 0; k < 32u; ++k) {
                    const uint32_t m = sk_mask_of_index(i * 32u + k);
                    bits |= ((algo == VP_ALGO_NAIVE ? sk_simple_plain(m) : sk_simple_shift(m)) ? 1u : 0u) << k;
                }
                h_table[i] = bits;
            }
        });
    for (auto& th : pool) th.join();
}

}  // namespace vp
