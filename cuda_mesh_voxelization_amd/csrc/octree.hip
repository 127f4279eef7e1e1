// octree.hip -- sparse voxel octree of a whole-grid bit grid for gfx950 (MI355X): vp_octree, vp_octree_expand and the host validator
// (include/vphip.h).
//
// The tree covers the cube of side P = NextPow2(n), L = log2 P levels; a level-l cell has side P >> l and is empty, full or mixed.  A node
// is stored for the root and for every mixed cell of levels 1 .. L - 1, breadth-first, ascending Morton code within a level.  A record is
// (valid | full << 8, index of the first mixed child).  Integer logic only: both algos, the host restatement and numpy agree byte for byte.
// Cell states are kept in Morton order, so the eight children of cell m are the cells 8 m .. 8 m + 7 one level down, and the index of the
// first mixed child of a node is the exclusive count of the mixed cells in front of cell 8 m.
//   NAIVE  oc_leaf_state   one thread per side-2 cell: a state byte (0 empty, 1 mixed, 2 full) from its eight voxels
//          oc_up_state     one thread per cell of the level above: the state from the eight state bytes below
//          oc_scan_flags   per level, one workgroup: the exclusive scan of the stored flags (the rank of every cell) and the level's count
//          oc_offsets      level_offset from the counts
//          oc_write_level  one thread per cell: a stored cell writes its record at level_offset[l] + rank
//   TILED  oc_block<0>     one workgroup per 32^3 block of bits (1024 words staged in LDS), blocks in Morton order.  Thread t owns the side-2
//                          cells 16 t .. 16 t + 15 of the block (Morton codes), i.e. the side-4 cells 2 t and 2 t + 1; the any / all bits of
//                          the sides 2, 4, 8, 16 and 32 are reduced in registers, LDS and two ballots.  Writes the five mixed counts, the
//                          five full-child counts and the state byte of the block.
//          oc_upper        one workgroup: the levels above the blocks from the block states, the ranks of their cells, the scans of the
//                          per-block counts of the five in-block levels, level_offset and full_leaves.
//          oc_block<1>     the same reduction; every stored cell writes its record at level_offset[l] + block offset + rank in the block,
//                          the child index from the same ranks one level down.  No atomics.
//          oc_write_level  the levels above the blocks (at most 4681 cells).
//   expand NAIVE           one thread per voxel descends from the root; 64 bits per ballot.
//          TILED           one lane per output word: the walk to the side-32 cell is the same for the 32 bits, then at most 31 node
//                          visits resolve them along x.
// A descent reads a child only if its index is below the node count and runs L levels at most, whatever the bytes are.
#include <algorithm>
#include <vector>

#include "vp_internal.h"
#include "wg_scan.h"

namespace vp {

namespace {

constexpr int kSlots = 11;                                        // level_offset / full_leaves entries
constexpr int kSumWords = 3 * kSlots;                             // device summary: level_offset | full_leaves | nodes per level

// every third bit of a Morton code, from bit 0
__host__ __device__ __forceinline__ uint32_t compact3(uint32_t m)
{
    uint32_t x = m & 0x09249249u;
    x = (x ^ (x >> 2)) & 0x030C30C3u;
    x = (x ^ (x >> 4)) & 0x0300F00Fu;
    x = (x ^ (x >> 8)) & 0x030000FFu;
    x = (x ^ (x >> 16)) & 0x000003FFu;
    return x;
}

inline size_t level_start(uint32_t l) { return (((size_t)1 << (3 * l)) - 1) / 7; }          // cells of the levels above l

// the eight voxels of the side-2 cell (cx, cy, cz) of the grid, bit c = x + 2 y + 4 z; voxels outside the grid are unset
__device__ __forceinline__ uint32_t grid_cell_bits(const uint32_t* __restrict__ words, uint32_t n, uint32_t cx, uint32_t cy, uint32_t cz)
{
    const uint32_t x = 2 * cx, y = 2 * cy, z = 2 * cz;
    if (x >= n || y >= n || z >= n) return 0u;                     // n is even: the cell is inside or outside as a whole
    const uint32_t* row = words + (x >> 5) + (size_t)(n / 32) * ((size_t)y + (size_t)n * z);
    const size_t dy = n / 32, dz = (size_t)(n / 32) * n;
    const uint32_t sh = x & 31u;
    return ((row[0] >> sh) & 3u) | (((row[dy] >> sh) & 3u) << 2) | (((row[dz] >> sh) & 3u) << 4) | (((row[dz + dy] >> sh) & 3u) << 6);
}

__device__ __forceinline__ uint32_t state_of(uint32_t valid, uint32_t full) { return valid == 0u ? 0u : (full == 0xFFu ? 2u : 1u); }

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

// cells = 8^(L-1) is a multiple of 256: every workgroup is whole
__global__ void __launch_bounds__(256)
oc_leaf_state(const uint32_t* __restrict__ words, uint32_t n, uint8_t* __restrict__ st, uint32_t* __restrict__ full_leaves)
{
    __shared__ uint32_t smem[4];
    const size_t m = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = grid_cell_bits(words, n, compact3((uint32_t)m), compact3((uint32_t)(m >> 1)), compact3((uint32_t)(m >> 2)));
    const uint32_t s = state_of(v, v);
    st[m] = (uint8_t)s;
    const uint32_t sum = wg_sum_256(s == 1u ? (uint32_t)__popc(v) : 0u, smem);
    if (threadIdx.x == 0 && sum) atomicAdd(full_leaves, sum);
}

__device__ __forceinline__ void child_masks(const uint8_t* __restrict__ child, size_t m, uint32_t& valid, uint32_t& full)
{
    valid = full = 0u;
    for (uint32_t c = 0; c < 8; ++c) {
        const uint32_t s = child[8 * m + c];
        valid |= (s != 0u ? 1u : 0u) << c;
        full |= (s == 2u ? 1u : 0u) << c;
    }
}

__global__ void __launch_bounds__(256)
oc_up_state(const uint8_t* __restrict__ child, uint8_t* __restrict__ st, size_t cells, int root, uint32_t* __restrict__ full_leaves)
{
    __shared__ uint32_t smem[4];
    const size_t m = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t mine = 0u;
    if (m < cells) {
        uint32_t valid, full;
        child_masks(child, m, valid, full);
        const uint32_t s = state_of(valid, full);
        st[m] = (uint8_t)s;
        if (s == 1u || root) mine = (uint32_t)__popc(full);
    }
    const uint32_t sum = wg_sum_256(mine, smem);
    if (threadIdx.x == 0 && sum) atomicAdd(full_leaves, sum);
}

// rank[m] = the stored cells in front of cell m; *count = the stored cells of the level.  The root is stored whatever its state
__global__ void __launch_bounds__(1024)
oc_scan_flags(const uint8_t* __restrict__ st, size_t cells, int root, uint32_t* __restrict__ rank, uint32_t* __restrict__ count)
{
    __shared__ uint32_t part[1024];
    const uint32_t total = wg_scan_1024<uint32_t, size_t>(
        part, cells, [&](size_t i) { return (st[i] == 1 || root) ? 1u : 0u; }, [&](size_t i, uint32_t v) { rank[i] = v; });
    if (threadIdx.x == 0) *count = total;
}

__device__ __forceinline__ void write_offsets(uint32_t* __restrict__ sum, uint32_t L)
{
    uint32_t run = 0u;
    for (uint32_t l = 0; l < (uint32_t)kSlots; ++l) {
        sum[l] = run;
        if (l < L) run += sum[2 * kSlots + l];
    }
}

__global__ void oc_offsets(uint32_t* __restrict__ sum, uint32_t L)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) write_offsets(sum, L);
}

// level l < L - 1: child / child_rank are the states and ranks of level l + 1; level L - 1 (child == nullptr): the children are voxels
__global__ void __launch_bounds__(256)
oc_write_level(const uint8_t* __restrict__ st, const uint32_t* __restrict__ rank, const uint8_t* __restrict__ child,
               const uint32_t* __restrict__ child_rank, const uint32_t* __restrict__ words, uint32_t n, size_t cells, uint32_t l,
               const uint32_t* __restrict__ sum, uint2* __restrict__ nodes)
{
    const size_t m = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= cells || !(st[m] == 1 || l == 0u)) return;
    uint32_t valid, full, first = 0u;
    if (child) {
        child_masks(child, m, valid, full);
        if (valid & ~full) first = sum[l + 1] + child_rank[8 * m];
    } else {
        valid = full = grid_cell_bits(words, n, compact3((uint32_t)m), compact3((uint32_t)(m >> 1)), compact3((uint32_t)(m >> 2)));
    }
    nodes[sum[l] + rank[m]] = make_uint2(valid | (full << 8), first);
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

// the eight voxels of the side-2 cell with Morton code m (12 bits) of the staged block: s_words[32 z + y] holds the 32 bits along x
__device__ __forceinline__ uint32_t block_cell_bits(const uint32_t* s_words, uint32_t m)
{
    const uint32_t sh = 2u * compact3(m), r = 64u * compact3(m >> 2) + 2u * compact3(m >> 1);
    return ((s_words[r] >> sh) & 3u) | (((s_words[r + 1] >> sh) & 3u) << 2) | (((s_words[r + 32] >> sh) & 3u) << 4) |
           (((s_words[r + 33] >> sh) & 3u) << 6);
}

// in-block level i = 0 .. 4 holds the cells of side 2 << i, tree level L - 1 - i.  cnt / flb / off: five arrays of nb entries, block-major
// within a level (blocks in Morton order)
template <bool WRITE>
__global__ void __launch_bounds__(256)
oc_block(const uint32_t* __restrict__ words, uint32_t n, uint32_t L, uint32_t nb, uint32_t* __restrict__ cnt, uint32_t* __restrict__ flb,
         uint8_t* __restrict__ st_block, const uint32_t* __restrict__ off, const uint32_t* __restrict__ sum, uint2* __restrict__ nodes)
{
    __shared__ uint32_t s_words[1024];
    __shared__ uint32_t s_st4[256];                                 // per thread: the any bits of its two side-4 cells | the all bits << 2
    __shared__ uint32_t s_r4[256];                                  // per thread: the mixed side-4 cells in front of its own
    __shared__ unsigned long long s_top[2];                         // any / all of the 64 side-8 cells
    __shared__ uint32_t s_scan[4];
    __shared__ unsigned long long s_sum[4];
    const uint32_t t = threadIdx.x, bm = blockIdx.x;
    const uint32_t bx = compact3(bm), by = compact3(bm >> 1), bz = compact3(bm >> 2);
    if (32u * max(bx, max(by, bz)) >= n) {                          // a block outside the grid is empty (the whole workgroup leaves)
        if (!WRITE && t == 0) {
            for (uint32_t i = 0; i < 5; ++i) cnt[i * nb + bm] = flb[i * nb + bm] = 0u;
            st_block[bm] = 0;
        }
        return;
    }
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t idx = t + 256u * k;
        s_words[idx] = words[bx + (size_t)(n / 32) * ((size_t)(32u * by + (idx & 31u)) + (size_t)n * (32u * bz + (idx >> 5)))];
    }
    __syncthreads();

    // side 2: 16 cells per thread
    uint32_t any2 = 0u, all2 = 0u, fl2 = 0u;
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t v = block_cell_bits(s_words, 16u * t + j);
        any2 |= (v != 0u ? 1u : 0u) << j;
        all2 |= (v == 0xFFu ? 1u : 0u) << j;
        if (v != 0u && v != 0xFFu) fl2 += (uint32_t)__popc(v);
    }
    const uint32_t mix2 = any2 & ~all2;
    // side 4: the cells 2 t and 2 t + 1 are the two bytes of the thread's own bits
    const uint32_t a4 = ((any2 & 0xFFu) ? 1u : 0u) | ((any2 >> 8) ? 2u : 0u);
    const uint32_t l4 = ((all2 & 0xFFu) == 0xFFu ? 1u : 0u) | ((all2 >> 8) == 0xFFu ? 2u : 0u);
    const uint32_t mix4 = a4 & ~l4;
    const uint32_t fl4 = ((mix4 & 1u) ? (uint32_t)__popc(all2 & 0xFFu) : 0u) + ((mix4 & 2u) ? (uint32_t)__popc(all2 >> 8) : 0u);
    s_st4[t] = a4 | (l4 << 2);
    __syncthreads();
    // side 8: cell t of the first wave, from the threads 4 t .. 4 t + 3; its masks are the record of the side-8 node
    uint32_t m8 = 0u;
    if (t < 64) {
        const uint32_t b0 = s_st4[4 * t], b1 = s_st4[4 * t + 1], b2 = s_st4[4 * t + 2], b3 = s_st4[4 * t + 3];
        const uint32_t va = (b0 & 3u) | ((b1 & 3u) << 2) | ((b2 & 3u) << 4) | ((b3 & 3u) << 6);
        const uint32_t fa = (b0 >> 2) | ((b1 >> 2) << 2) | ((b2 >> 2) << 4) | ((b3 >> 2) << 6);
        m8 = va | (fa << 8);
        const unsigned long long a = __ballot(va != 0u), f = __ballot(fa == 0xFFu);     // the wave is whole: 64 cell states at a time
        if (t == 0) { s_top[0] = a; s_top[1] = f; }
    }
    __syncthreads();
    const unsigned long long A8 = s_top[0], L8 = s_top[1], M8 = A8 & ~L8;
    const uint32_t fl8 = (t < 64 && ((M8 >> t) & 1ull)) ? (uint32_t)__popc(m8 >> 8) : 0u;
    // sides 16 and 32: the same for every thread
    uint32_t A16 = 0u, L16 = 0u;
    for (uint32_t j = 0; j < 8; ++j) {
        A16 |= (((A8 >> (8 * j)) & 0xFFull) ? 1u : 0u) << j;
        L16 |= (((L8 >> (8 * j)) & 0xFFull) == 0xFFull ? 1u : 0u) << j;
    }
    const uint32_t M16 = A16 & ~L16;
    const bool any32 = A16 != 0u, all32 = L16 == 0xFFu;
    const bool stored32 = L == 5u || (any32 && !all32);             // P = 32: the block's own cell is the root, stored whatever it holds

    uint32_t tot;
    const uint32_t ex = wg_exclusive_256<uint32_t>((uint32_t)__popc(mix2) | ((uint32_t)__popc(mix4) << 16), s_scan, &tot);
    const uint32_t r2 = ex & 0xFFFFu, r4 = ex >> 16;

    if (!WRITE) {
        const unsigned long long fs = wg_sum_256<unsigned long long>(
            (unsigned long long)fl2 | ((unsigned long long)fl4 << 16) | ((unsigned long long)fl8 << 32), s_sum);
        if (t == 0) {
            uint32_t fl16 = 0u;
            for (uint32_t j = 0; j < 8; ++j)
                if ((M16 >> j) & 1u) fl16 += (uint32_t)__popcll((L8 >> (8 * j)) & 0xFFull);
            cnt[bm] = tot & 0xFFFFu;
            cnt[nb + bm] = tot >> 16;
            cnt[2 * nb + bm] = (uint32_t)__popcll(M8);
            cnt[3 * nb + bm] = (uint32_t)__popc(M16);
            cnt[4 * nb + bm] = stored32 ? 1u : 0u;
            flb[bm] = (uint32_t)(fs & 0xFFFFull);
            flb[nb + bm] = (uint32_t)((fs >> 16) & 0xFFFFull);
            flb[2 * nb + bm] = (uint32_t)(fs >> 32);
            flb[3 * nb + bm] = fl16;
            flb[4 * nb + bm] = stored32 ? (uint32_t)__popc(L16) : 0u;
            st_block[bm] = (uint8_t)(!any32 ? 0u : (all32 ? 2u : 1u));
        }
        return;
    }

    uint32_t base[5];
    for (uint32_t i = 0; i < 5; ++i) base[i] = sum[L - 1 - i] + off[i * nb + bm];
    for (uint32_t mm = mix2; mm; mm &= mm - 1u) {
        const uint32_t j = (uint32_t)__ffs((int)mm) - 1u;
        const uint32_t v = block_cell_bits(s_words, 16u * t + j);
        nodes[base[0] + r2 + (uint32_t)__popc(mix2 & ((1u << j) - 1u))] = make_uint2(v | (v << 8), 0u);
    }
    for (uint32_t h = 0; h < 2; ++h)
        if ((mix4 >> h) & 1u) {
            const uint32_t va = (any2 >> (8 * h)) & 0xFFu, fa = (all2 >> (8 * h)) & 0xFFu;
            const uint32_t first = (va & ~fa) ? base[0] + r2 + (h ? (uint32_t)__popc(mix2 & 0xFFu) : 0u) : 0u;
            nodes[base[1] + r4 + (h ? (mix4 & 1u) : 0u)] = make_uint2(va | (fa << 8), first);
        }
    s_r4[t] = r4;
    __syncthreads();
    if (t < 64 && ((M8 >> t) & 1ull)) {
        const uint32_t va = m8 & 0xFFu, fa = m8 >> 8;
        const uint32_t first = (va & ~fa) ? base[1] + s_r4[4 * t] : 0u;
        nodes[base[2] + (uint32_t)__popcll(M8 & ((1ull << t) - 1ull))] = make_uint2(m8, first);
    }
    if (t < 8 && ((M16 >> t) & 1u)) {
        const uint32_t va = (uint32_t)((A8 >> (8 * t)) & 0xFFull), fa = (uint32_t)((L8 >> (8 * t)) & 0xFFull);
        const uint32_t first = (va & ~fa) ? base[2] + (uint32_t)__popcll(M8 & ((1ull << (8 * t)) - 1ull)) : 0u;
        nodes[base[3] + (uint32_t)__popc(M16 & ((1u << t) - 1u))] = make_uint2(va | (fa << 8), first);
    }
    if (t == 0 && stored32) nodes[base[4]] = make_uint2(A16 | (L16 << 8), M16 ? base[3] : 0u);
}

// One workgroup.  st / rank hold the levels 0 .. U (the blocks are level U = L - 5) one after the other, level k at (8^k - 1) / 7; the
// ranks of level U are the block offsets of the side-32 cells, off + 4 nb, and are not stored a second time.
__global__ void __launch_bounds__(1024)
oc_upper(uint32_t L, uint32_t nb, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ flb, uint32_t* __restrict__ off,
         uint8_t* __restrict__ st, uint32_t* __restrict__ rank, uint32_t* __restrict__ sum)
{
    __shared__ uint32_t part[1024];
    const uint32_t U = L - 5u, tid = threadIdx.x;
    uint32_t counts[kSlots], fulls[kSlots];
    for (int l = 0; l < kSlots; ++l) counts[l] = fulls[l] = 0u;
    for (int k = (int)U - 1; k >= 0; --k) {
        const uint32_t cells = 1u << (3 * k);
        const uint8_t* child = st + ((1u << (3 * (k + 1))) - 1u) / 7u;
        uint8_t* mine = st + (cells - 1u) / 7u;
        uint32_t nf = 0u;
        for (uint32_t m = tid; m < cells; m += 1024u) {
            uint32_t valid, full;
            child_masks(child, m, valid, full);
            const uint32_t s = state_of(valid, full);
            mine[m] = (uint8_t)s;
            if (s == 1u || k == 0) nf += (uint32_t)__popc(full);
        }
        fulls[k] = wg_scan_1024<uint32_t, uint32_t>(part, 1024u, [&](uint32_t) { return nf; }, [&](uint32_t, uint32_t) {});
        __syncthreads();                                           // the states of level k are read by other threads from here on
    }
    for (uint32_t k = 0; k < U; ++k) {
        const uint32_t cells = 1u << (3 * k);
        const uint8_t* mine = st + (cells - 1u) / 7u;
        uint32_t* r = rank + (cells - 1u) / 7u;
        counts[k] = wg_scan_1024<uint32_t, uint32_t>(
            part, cells, [&](uint32_t i) { return (mine[i] == 1 || k == 0u) ? 1u : 0u; }, [&](uint32_t i, uint32_t v) { r[i] = v; });
    }
    for (uint32_t i = 0; i < 5; ++i) {
        const uint32_t* c = cnt + i * nb;
        const uint32_t* f = flb + i * nb;
        uint32_t* o = off + i * nb;
        counts[L - 1 - i] = wg_scan_1024<uint32_t, uint32_t>(part, nb, [&](uint32_t b) { return c[b]; }, [&](uint32_t b, uint32_t v) { o[b] = v; });
        fulls[L - 1 - i] = wg_scan_1024<uint32_t, uint32_t>(part, nb, [&](uint32_t b) { return f[b]; }, [&](uint32_t, uint32_t) {});
    }
    if (tid == 0) {
        for (int l = 0; l < kSlots; ++l) { sum[kSlots + l] = fulls[l]; sum[2 * kSlots + l] = counts[l]; }
        write_offsets(sum, L);
    }
}

// ---- expand ------------------------------------------------------------------------------------------------------------------------

struct Masks { uint32_t valid, full, first; };
__device__ __forceinline__ Masks masks_of(const uint2* __restrict__ nodes, uint32_t node)
{
    const uint2 r = nodes[node];
    return { r.x & 0xFFu, (r.x >> 8) & 0xFFu, r.y };
}

// the stored child c of a node, or 0 (never a child: the root) where the record points outside the buffer
__device__ __forceinline__ uint32_t stored_child(const Masks& k, uint32_t c, uint32_t count)
{
    const uint64_t next = (uint64_t)k.first + (uint32_t)__popc(k.valid & ~k.full & ((1u << c) - 1u));
    return next < count ? (uint32_t)next : 0u;
}

__global__ void __launch_bounds__(256)
oc_expand_naive(const uint2* __restrict__ nodes, uint32_t count, uint32_t n, uint32_t L, uint32_t* __restrict__ words)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;     // n^3 is a multiple of 256
    const uint32_t x = (uint32_t)(idx % n), y = (uint32_t)((idx / n) % n), z = (uint32_t)(idx / ((size_t)n * n));
    bool set = false;
    uint32_t node = 0u;
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t sh = L - 1u - l, c = ((x >> sh) & 1u) | (((y >> sh) & 1u) << 1) | (((z >> sh) & 1u) << 2);
        const Masks k = masks_of(nodes, node);
        if (!((k.valid >> c) & 1u)) break;
        if ((k.full >> c) & 1u) { set = true; break; }
        node = stored_child(k, c, count);
        if (node == 0u) break;
    }
    const unsigned long long m = __ballot(set);
    if ((threadIdx.x & 63u) == 0u) reinterpret_cast<uint2*>(words)[idx >> 6] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
}

// the 2 << SH bits along x at (y, z) of a node whose cell has side 2 << SH
template <int SH>
__device__ __forceinline__ uint32_t span_bits(const uint2* __restrict__ nodes, uint32_t count, uint32_t node, uint32_t y, uint32_t z)
{
    const Masks k = masks_of(nodes, node);
    const uint32_t cyz = (((y >> SH) & 1u) << 1) | (((z >> SH) & 1u) << 2);
    uint32_t out = 0u;
    for (uint32_t xb = 0; xb < 2; ++xb) {
        const uint32_t c = cyz | xb;
        if (!((k.valid >> c) & 1u)) continue;
        if ((k.full >> c) & 1u) { out |= (SH == 4 ? 0xFFFFu : ((1u << (1 << SH)) - 1u)) << (xb << SH); continue; }
        if constexpr (SH > 0) {
            const uint32_t next = stored_child(k, c, count);
            if (next != 0u) out |= span_bits<SH - 1>(nodes, count, next, y, z) << (xb << SH);
        }
    }
    return out;
}

__global__ void __launch_bounds__(256)
oc_expand_tiled(const uint2* __restrict__ nodes, uint32_t count, uint32_t n, uint32_t L, uint32_t* __restrict__ words, size_t nwords)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nwords) return;
    const uint32_t w = n / 32;
    const uint32_t x = (uint32_t)(idx % w) * 32u, y = (uint32_t)((idx / w) % n), z = (uint32_t)(idx / ((size_t)w * n));
    uint32_t node = 0u, out = 0u;
    bool inside = true;                                            // the walk ended on the stored side-32 cell of the word
    for (uint32_t l = 0; l + 5u < L; ++l) {
        const uint32_t sh = L - 1u - l, c = ((x >> sh) & 1u) | (((y >> sh) & 1u) << 1) | (((z >> sh) & 1u) << 2);
        const Masks k = masks_of(nodes, node);
        if (!((k.valid >> c) & 1u)) { inside = false; break; }
        if ((k.full >> c) & 1u) { inside = false; out = 0xFFFFFFFFu; break; }
        node = stored_child(k, c, count);
        if (node == 0u) { inside = false; break; }
    }
    if (inside) out = span_bits<4>(nodes, count, node, y, z);
    words[idx] = out;
}

uint32_t levels_of(uint32_t n)
{
    uint32_t L = 5;
    while ((1u << L) < n) ++L;
    return L;
}

}  // namespace

// The caller has validated everything.  Blocks once: the summary is read back to size the node buffer.
int launch_octree(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, int algo, uint64_t* h_nodes)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n, L = levels_of(n), U = L - 5u, nb = 1u << (3 * U);
    ctx->oc.n = 0;                                                 // from here on the previous result is gone
    VP_TRY(ctx->oc.host.need(kSumWords));
    VP_TRY(reserve(ctx, ctx->oc.sum, kSumWords * 4, false));
    uint32_t* sum = (uint32_t*)ctx->oc.sum.ptr;
    const uint32_t top = algo == VP_ALGO_NAIVE ? L - 1u : U;       // the levels 0 .. top have state bytes
    VP_TRY(reserve(ctx, ctx->oc.state, level_start(top + 1), false));
    VP_TRY(reserve(ctx, ctx->oc.rank, std::max<size_t>(level_start(algo == VP_ALGO_NAIVE ? L : U), 1) * 4, false));
    uint8_t* state = (uint8_t*)ctx->oc.state.ptr;
    uint32_t* rank = (uint32_t*)ctx->oc.rank.ptr;
    uint32_t *cnt = nullptr, *flb = nullptr, *off = nullptr;
    VP_HIP(hipMemsetAsync(sum, 0, kSumWords * 4, st));
    auto cells_of = [](uint32_t l) { return (size_t)1 << (3 * l); };

    if (algo == VP_ALGO_NAIVE) {
        {
            ProfScope p(ctx, VP_K_MD_PREFILL);
            hipLaunchKernelGGL(oc_leaf_state, dim3((unsigned)(cells_of(L - 1) / 256)), dim3(256), 0, st, d_words, n, state + level_start(L - 1),
                               sum + kSlots + (L - 1));
            for (int l = (int)L - 2; l >= 0; --l)
                hipLaunchKernelGGL(oc_up_state, dim3((unsigned)((cells_of(l) + 255) / 256)), dim3(256), 0, st,
                                   (const uint8_t*)(state + level_start(l + 1)), state + level_start(l), cells_of(l), l == 0 ? 1 : 0, sum + kSlots + l);
        }
        VP_HIP(hipGetLastError());
        ProfScope p(ctx, VP_K_MD_SCAN);
        for (uint32_t l = 0; l < L; ++l)
            hipLaunchKernelGGL(oc_scan_flags, dim3(1), dim3(1024), 0, st, (const uint8_t*)(state + level_start(l)), cells_of(l), l == 0 ? 1 : 0,
                               rank + level_start(l), sum + 2 * kSlots + l);
        hipLaunchKernelGGL(oc_offsets, dim3(1), dim3(64), 0, st, sum, L);
    } else {
        VP_TRY(reserve(ctx, ctx->oc.cnt, (size_t)nb * 15 * 4, false));
        cnt = (uint32_t*)ctx->oc.cnt.ptr; flb = cnt + 5 * (size_t)nb; off = flb + 5 * (size_t)nb;
        {
            ProfScope p(ctx, VP_K_MD_COUNT);
            hipLaunchKernelGGL(oc_block<false>, dim3(nb), dim3(256), 0, st, d_words, n, L, nb, cnt, flb, state + level_start(U),
                               (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint2*)nullptr);
        }
        VP_HIP(hipGetLastError());
        ProfScope p(ctx, VP_K_MD_SCAN);
        hipLaunchKernelGGL(oc_upper, dim3(1), dim3(1024), 0, st, L, nb, (const uint32_t*)cnt, (const uint32_t*)flb, off, state, rank, sum);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->oc.host, sum, kSumWords * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint64_t M = ctx->oc.host[kSlots - 1];
    VP_TRY(reserve(ctx, ctx->oc.nodes, M * 8, false));
    uint2* nodes = (uint2*)ctx->oc.nodes.ptr;

    {
        ProfScope p(ctx, algo == VP_ALGO_NAIVE ? VP_K_MD_NAIVE : VP_K_MD_WRITE);
        if (algo == VP_ALGO_TILED)
            hipLaunchKernelGGL(oc_block<true>, dim3(nb), dim3(256), 0, st, d_words, n, L, nb, (uint32_t*)nullptr, (uint32_t*)nullptr,
                               (uint8_t*)nullptr, (const uint32_t*)off, (const uint32_t*)sum, nodes);
        for (uint32_t l = 0; l < (algo == VP_ALGO_NAIVE ? L : U); ++l) {
            const bool voxels = l == L - 1u;
            const uint32_t* child_rank = voxels ? nullptr : ((algo == VP_ALGO_TILED && l + 1 == U) ? off + 4 * (size_t)nb : rank + level_start(l + 1));
            hipLaunchKernelGGL(oc_write_level, dim3((unsigned)((cells_of(l) + 255) / 256)), dim3(256), 0, st,
                               (const uint8_t*)(state + level_start(l)), (const uint32_t*)(rank + level_start(l)),
                               voxels ? (const uint8_t*)nullptr : (const uint8_t*)(state + level_start(l + 1)), (const uint32_t*)child_rank, d_words, n,
                               cells_of(l), l, (const uint32_t*)sum, nodes);
        }
    }
    VP_HIP(hipGetLastError());
    for (int l = 0; l < kSlots; ++l) { ctx->oc.level_offset[l] = ctx->oc.host[l]; ctx->oc.full_leaves[l] = ctx->oc.host[kSlots + l]; }
    ctx->oc.count = M;
    ctx->oc.n = n;
    if (h_nodes) *h_nodes = M;
    return 0;
}

int launch_octree_expand(vp_ctx* ctx, const Frame& f, const uint32_t* d_nodes, uint64_t nodes, uint32_t* d_words, int algo)
{
    const uint32_t n = f.n, L = levels_of(n);
    const size_t nvox = (size_t)n * n * n;
    ProfScope p(ctx, VP_K_MD_FILL);
    if (algo == VP_ALGO_NAIVE)
        hipLaunchKernelGGL(oc_expand_naive, dim3((unsigned)(nvox / 256)), dim3(256), 0, ctx->stream, (const uint2*)d_nodes, (uint32_t)nodes, n, L,
                           d_words);
    else
        hipLaunchKernelGGL(oc_expand_tiled, dim3((unsigned)((nvox / 32 + 255) / 256)), dim3(256), 0, ctx->stream, (const uint2*)d_nodes,
                           (uint32_t)nodes, n, L, d_words, nvox / 32);
    VP_HIP(hipGetLastError());
    return 0;
}

// Pure CPU: walks the levels once, carrying the cell coordinates of the stored nodes.  0, or VP_ERR_INVALID with the reason.
int octree_validate(const uint32_t* h, uint64_t M, uint32_t n)
{
    const char* who = "vp_octree_validate_host";
    if (!h) return set_error(VP_ERR_INVALID, "%s: null nodes", who);
    if (n < 32 || n > 1024 || n % 32) return set_error(VP_ERR_INVALID, "%s: n=%u (32 <= n <= 1024, n %% 32 == 0)", who, n);
    if (M < 1 || M >= (1ull << 28)) return set_error(VP_ERR_INVALID, "%s: %llu nodes (1 .. 2^28 - 1)", who, (unsigned long long)M);
    const uint32_t L = levels_of(n), P = 1u << L;
    struct Cell { uint16_t x, y, z; };
    std::vector<Cell> level{ Cell{0, 0, 0} }, next;
    uint64_t begin = 0, running = 1;
    for (uint32_t l = 0; l < L && !level.empty(); ++l) {
        const uint32_t side = P >> (l + 1);
        next.clear();
        for (size_t k = 0; k < level.size(); ++k) {
            const uint64_t i = begin + k;
            const uint32_t masks = h[2 * i], child = h[2 * i + 1], valid = masks & 0xFFu, full = (masks >> 8) & 0xFFu, mixed = valid & ~full;
            if (masks >> 16) return set_error(VP_ERR_INVALID, "%s: node %llu: upper mask bits set", who, (unsigned long long)i);
            if (full & ~valid) return set_error(VP_ERR_INVALID, "%s: node %llu: full is not a subset of valid", who, (unsigned long long)i);
            if (l > 0 && (valid == 0 || full == 0xFFu)) return set_error(VP_ERR_INVALID, "%s: node %llu: a stored cell that is not mixed", who, (unsigned long long)i);
            if (l == L - 1 && mixed) return set_error(VP_ERR_INVALID, "%s: node %llu: a voxel that is neither set nor unset", who, (unsigned long long)i);
            if (child != (mixed ? running : 0)) return set_error(VP_ERR_INVALID, "%s: node %llu: child %u is not the running sum", who, (unsigned long long)i, child);
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t cx = 2u * level[k].x + (c & 1u), cy = 2u * level[k].y + ((c >> 1) & 1u), cz = 2u * level[k].z + (c >> 2);
                const uint32_t far = std::max(cx, std::max(cy, cz)) * side;
                if (((full >> c) & 1u) && far + side > n) return set_error(VP_ERR_INVALID, "%s: node %llu: a full child pokes out of the grid", who, (unsigned long long)i);
                if (((valid >> c) & 1u) && far >= n) return set_error(VP_ERR_INVALID, "%s: node %llu: a child outside the grid", who, (unsigned long long)i);
                if ((mixed >> c) & 1u) next.push_back(Cell{(uint16_t)cx, (uint16_t)cy, (uint16_t)cz});
            }
            running += (uint64_t)__builtin_popcount(mixed);
            if (running > M) return set_error(VP_ERR_INVALID, "%s: node %llu: children beyond the %llu nodes", who, (unsigned long long)i, (unsigned long long)M);
        }
        begin += level.size();
        level.swap(next);
    }
    if (running != M) return set_error(VP_ERR_INVALID, "%s: the levels end at %llu, not at %llu nodes", who, (unsigned long long)running, (unsigned long long)M);
    return 0;
}

}  // namespace vp
