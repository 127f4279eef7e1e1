// components.hip -- connected-component labelling and size filters of a whole-grid bit grid for gfx950 (MI355X): vp_components_label,
// vp_components_sizes, vp_components_filter (include/vphip.h).
//
// Set voxels are the foreground, voxels outside the grid are empty, connectivity is 6 (faces) or 26 (faces, edges, corners).  Component k
// (1 .. K) is the one with the k-th lowest minimum linear voxel index v = x + n (y + n z); the label volume therefore equals
// scipy.ndimage.label(vox_zyx, structure)[0] element for element.
//
// The label volume is the PARENT ARRAY P of a union-find forest while the call runs: P[v] = 0xFFFFFFFF for an empty voxel, else the
// linear index of another voxel OF THE SAME COMPONENT with P[v] <= v.  A voxel with P[v] == v is a root.
//
//   init     NAIVE: P[v] = v, one thread per voxel.  TILED: every set voxel points at the first voxel of its x run.  Inside a word that
//            is bit arithmetic; across the words of a row the start of the run that reaches a word's bit 31 is carried by a segmented scan
//            over the lanes of a wave (an all-ones word passes the start through, as fill_x passes its flood).  A run that crosses word
//            edges is one tree from the start, with no atomics.  The 32 labels of a word are stored as 8 x 16 B by 8 lanes.
//   merge    NAIVE: one thread per set voxel unites it with each set backward neighbour (3 under 6-connectivity, 13 under 26).
//            TILED: one lane per word and backward neighbour row -- (y-1, z), (y, z-1) under 6; (y-1, z), (y-1, z-1), (y, z-1),
//            (y+1, z-1) under 26 -- and ONE union per pair of adjacent runs: under 6 at the run starts of w & nb (a run that continues
//            from the previous word is not a start: a solid row pair costs one union); under 26 at the run starts of each of
//            w & (nb << 1), w & nb, w & (nb >> 1), shifts carried across word edges ("1 0 1" over "1 1 1" touches two runs).  Inside a
//            run of w & shift(nb) consecutive pairs are joined through both rows, so the first pair stands for all of them.
//   union    lock-free: find both roots; atomicMin the larger root's slot with the smaller root; if the value returned is not the
//            slot's own index, another thread had linked that root meanwhile: go on with the returned value in its place.  A find
//            also lowers the slot it started from to the root it found (atomicMin again).  Every load of P in the merge kernels is a
//            relaxed agent-scope atomic load, every store an agent-scope atomicMin: nothing rests on what a CU's L1 still holds.
//   flatten  (after the kernel boundary) every set voxel takes its root; roots are counted per block of 8192 voxels.
//   rank     a one-workgroup exclusive scan of the block counts (the shape of extract.hip); then every root v takes
//            kRankFlag | rank(v), its rank among the roots in index order.  The total is K.
//   relabel  a voxel that holds a flagged rank becomes rank + 1; any other set voxel reads its root's slot and takes rank + 1 from it --
//            or the label itself if the root was rewritten already: flagged ranks (bit 31), labels and indices (below 2^30) cannot be
//            mistaken for one another, so one kernel rewrites roots while others still read them.
//   sizes    one atomicAdd per run of lanes of a wave that hold the same label, and the label a wave meets most is summed in a register
//            over the wave's whole grid-stride loop: one giant component costs one add per wave, not one per voxel.
//   select   MIN_VOXELS: a compare per label.  KEEP_LARGEST m: m rounds of an arg-max over the sizes with the 64-bit key
//            size << 32 | (0xFFFFFFFF - label) -- ties go to the lower label -- each skipping the earlier winners.
//   write    8 lanes assemble one output word from the keep flags of their 4 labels each; one writer per word.
//
// Order-free: the only writes of the merge kernels are atomicMin with a lower index of the same component, so P[v] <= v always, slots
// only fall, and a slot that is no root never becomes one again.  A union ends when both finds return the same root or when its
// atomicMin hit a slot that still was a root, which links the two trees; otherwise it goes on with strictly lower indices, so it ends
// after finitely many steps and never waits for another thread.  When the kernel has ended every pair it was given is in one tree, and
// the root of a tree is the lowest index in it -- the same forest ROOTS whatever the order of execution.  The ranks of the roots in
// index order are the labels, so the label volume is a function of the grid alone.  No persistent kernel, grid barrier, cooperative
// launch or inline assembly: kernel boundaries are the only synchronisation between the steps.
#include "vp_internal.h"
#include "wg_scan.h"

#include <algorithm>

namespace vp {

namespace {

constexpr uint32_t kBg = 0xFFFFFFFFu;          // P of an empty voxel
constexpr uint32_t kRankFlag = 0x80000000u;    // roots hold kRankFlag | rank between comp_rank and comp_relabel (n <= 1024: indices < 2^30)
constexpr uint32_t kChunk = 8192;              // voxels per workgroup of flatten / rank: 8 rounds x 256 lanes x 4 voxels; n^3 % 32768 == 0
constexpr uint32_t kChunkVec = kChunk / 4;

__device__ __forceinline__ uint32_t ld(const uint32_t* P, uint32_t i)
{
    return __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t lower(uint32_t* P, uint32_t i, uint32_t v)
{
    return __hip_atomic_fetch_min(P + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of set voxel i; the slot of i is lowered to it when the path was longer than one link
__device__ __forceinline__ uint32_t find_root(uint32_t* P, uint32_t i)
{
    const uint32_t i0 = i;
    uint32_t p = ld(P, i);
    const uint32_t p0 = p;
    while (p != i) { i = p; p = ld(P, i); }
    if (i < p0) (void)lower(P, i0, i);
    return i;
}

__device__ __forceinline__ void unite(uint32_t* P, uint32_t a, uint32_t b)
{
    while (true) {
        a = find_root(P, a);
        b = find_root(P, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = lower(P, a, b);     // P[a] = min(P[a], b)
        if (old == a) return;                    // a still was a root: linked
        a = old;                                 // a had been linked to old < a meanwhile: old and b are still to be joined
    }
}

// ---- NAIVE ----
__global__ void __launch_bounds__(256)
comp_init_naive(const uint32_t* __restrict__ W, uint32_t* __restrict__ P, size_t nvox)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvox) return;
    P[v] = ((W[v >> 5] >> (v & 31)) & 1u) ? (uint32_t)v : kBg;
}

template <int CONN>
__global__ void __launch_bounds__(256)
comp_merge_naive(const uint32_t* __restrict__ W, uint32_t* P, uint32_t n, size_t nvox)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvox) return;
    if (!((W[v >> 5] >> (v & 31)) & 1u)) return;
    const int N = (int)n;
    const int x = (int)(v % n), y = (int)((v / n) % n), z = (int)(v / ((size_t)n * n));
    // the neighbours with a lower linear index: dz < 0, or dz == 0 and dy < 0, or dz == dy == 0 and dx < 0
    for (int dz = -1; dz <= 0; ++dz)
        for (int dy = -1; dy <= (dz < 0 ? 1 : 0); ++dy)
            for (int dx = -1; dx <= ((dz < 0 || dy < 0) ? 1 : -1); ++dx) {
                if (CONN == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
                const int xx = x + dx, yy = y + dy, zz = z + dz;
                if (xx < 0 || xx >= N || yy < 0 || yy >= N || zz < 0) continue;
                const size_t u = ((size_t)zz * n + yy) * n + xx;
                if ((W[u >> 5] >> (u & 31)) & 1u) unite(P, (uint32_t)v, (uint32_t)u);
            }
}

// ---- TILED ----
// Each wave owns rpw whole rows (rpw w <= 64 lanes, lane = row x word); the workgroup's 4 rpw w words are consecutive in memory.
__global__ void __launch_bounds__(256)
comp_init_runs(const uint32_t* __restrict__ W, uint32_t* __restrict__ P, uint32_t n, uint32_t w, uint32_t rpw)
{
    __shared__ uint32_t s_w[256], s_c[256];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wpw = rpw * w;
    const size_t nwords = (size_t)n * n * w;
    const size_t wbase = (size_t)blockIdx.x * 4 * wpw;
    const size_t gw = wbase + (size_t)wave * wpw + lane;
    const uint32_t sub = lane % w;
    const bool valid = lane < wpw && gw < nwords;
    const uint32_t cw = valid ? W[gw] : 0u;
    // s: x of the first voxel of the run that reaches bit 31 of this word, with nothing carried in (none: kBg); t: the word passes a run through
    uint32_t t = cw == ~0u ? 1u : 0u;
    uint32_t s = kBg;
    if (cw >> 31) s = sub * 32u + (t ? 0u : 32u - (uint32_t)__clz((int)~cw));
    for (uint32_t d = 1; d < w; d <<= 1) {
        const uint32_t su = __shfl_up(s, d), tu = __shfl_up(t, d);
        if (sub >= d) {                          // lane - d is a word of the same row
            if (t && su != kBg) s = su;
            t &= tu;
        }
    }
    uint32_t cin = __shfl_up(s, 1);              // the run that arrives at bit 0 from the previous word of the row
    if (sub == 0) cin = kBg;
    if (lane < wpw) { s_w[wave * wpw + lane] = cw; s_c[wave * wpw + lane] = cin; }
    __syncthreads();
    const uint32_t parts = 4 * wpw * 8;          // 16-byte pieces of the workgroup's label rows
    for (uint32_t q = threadIdx.x; q < parts; q += 256) {
        const uint32_t j = q >> 3, part = q & 7;
        const size_t g = wbase + j;
        if (g >= nwords) break;
        const uint32_t c = s_w[j], ci = s_c[j];
        const uint32_t x0 = (uint32_t)(g % w) * 32u;
        const uint32_t rowv = (uint32_t)(g / w) * n;           // linear index of the row's voxel x = 0
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = part * 4 + k;
            if (!((c >> b) & 1u)) { o[k] = kBg; continue; }
            const uint32_t zero = ~c & ((2u << b) - 1u);       // the empty voxels at or below b (b = 31: the mask wraps to all ones)
            const uint32_t start = zero ? x0 + 32u - (uint32_t)__clz((int)zero) : (ci != kBg ? ci : x0);
            o[k] = rowv + start;
        }
        reinterpret_cast<uint4*>(P)[g * 8 + part] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// the unions of word g (voxels v0 .. v0 + 31) with word j of a backward neighbour row (voxels u0 ..), one per adjacent pair of runs
template <int CONN>
__device__ __forceinline__ void merge_row(const uint32_t* __restrict__ W, uint32_t* P, uint32_t cw, uint32_t cwp, uint32_t sub, uint32_t w,
                                          uint32_t v0, size_t j)
{
    const uint32_t nb = W[j];
    const uint32_t nbp = sub ? W[j - 1] : 0u;
    const uint32_t u0 = (uint32_t)(j * 32);
    const uint32_t top = cwp >> 31;              // the previous voxel of this row, x0 - 1
    {
        const uint32_t m = cw & nb;
        uint32_t st = m & ~((m << 1) | (top & (nbp >> 31)));
        while (st) { const uint32_t b = (uint32_t)__ffs((int)st) - 1u; st &= st - 1u; unite(P, v0 + b, u0 + b); }
    }
    if (CONN == 26) {
        const uint32_t nbn = sub + 1 < w ? W[j + 1] : 0u;
        const uint32_t lo = (nb << 1) | (nbp >> 31);           // bit i: the neighbour row's voxel x - 1
        const uint32_t ml = cw & lo;
        uint32_t st = ml & ~((ml << 1) | (top & (nbp >> 30) & 1u));
        while (st) { const uint32_t b = (uint32_t)__ffs((int)st) - 1u; st &= st - 1u; unite(P, v0 + b, u0 + b - 1u); }
        const uint32_t hi = (nb >> 1) | (nbn << 31);           // bit i: the neighbour row's voxel x + 1
        const uint32_t mh = cw & hi;
        st = mh & ~((mh << 1) | (top & nb & 1u));
        while (st) { const uint32_t b = (uint32_t)__ffs((int)st) - 1u; st &= st - 1u; unite(P, v0 + b, u0 + b + 1u); }
    }
}

template <int CONN>
__global__ void __launch_bounds__(256)
comp_merge_runs(const uint32_t* __restrict__ W, uint32_t* P, uint32_t n, uint32_t w, size_t nwords)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nwords) return;
    const uint32_t cw = W[g];
    if (!cw) return;
    const uint32_t sub = (uint32_t)(g % w);
    const size_t row = g / w;
    const uint32_t y = (uint32_t)(row % n), z = (uint32_t)(row / n);
    const uint32_t cwp = sub ? W[g - 1] : 0u;
    const uint32_t v0 = (uint32_t)(g * 32);
    const size_t rw = w, pw = (size_t)n * w;     // words per row, per plane
    if (y > 0) merge_row<CONN>(W, P, cw, cwp, sub, w, v0, g - rw);
    if (z > 0) {
        if (CONN == 26 && y > 0) merge_row<CONN>(W, P, cw, cwp, sub, w, v0, g - pw - rw);
        merge_row<CONN>(W, P, cw, cwp, sub, w, v0, g - pw);
        if (CONN == 26 && y + 1 < n) merge_row<CONN>(W, P, cw, cwp, sub, w, v0, g - pw + rw);
    }
}

// ---- the steps both forms share ----
__global__ void __launch_bounds__(256)
comp_flatten(uint32_t* P, uint32_t* __restrict__ block_roots)
{
    __shared__ uint32_t part[4];
    uint4* P4 = reinterpret_cast<uint4*>(P);
    uint32_t roots = 0;
    for (uint32_t it = 0; it < 8; ++it) {
        const size_t q = (size_t)blockIdx.x * kChunkVec + it * 256 + threadIdx.x;
        const uint4 p = P4[q];
        uint32_t o[4] = {p.x, p.y, p.z, p.w};
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (o[k] == kBg) continue;
            uint32_t r = o[k], pr = P[r];
            while (pr != r) { r = pr; pr = P[r]; }             // slots only fall and every path ends in the tree's root
            any |= r != o[k];
            o[k] = r;
            roots += r == (uint32_t)(q * 4 + k) ? 1u : 0u;
        }
        if (any) P4[q] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    const uint32_t total = wg_sum_256(roots, part);
    if (threadIdx.x == 0) block_roots[blockIdx.x] = total;
}

// one workgroup: off[i] = sum of cnt[0..i), off[m] = total (K < 2^30 fits 32 bits)
__global__ void __launch_bounds__(1024)
comp_scan(const uint32_t* __restrict__ cnt, uint32_t m, uint32_t* __restrict__ off)
{
    __shared__ uint32_t part[1024];
    const uint32_t total = wg_scan_1024(part, m, [&](uint32_t i) { return cnt[i]; }, [&](uint32_t i, uint32_t before) { off[i] = before; });
    if (threadIdx.x == 1023) off[m] = total;
}

__global__ void __launch_bounds__(256)
comp_rank(uint32_t* P, const uint32_t* __restrict__ block_off)
{
    __shared__ uint32_t wave_sum[4];
    const uint4* P4 = reinterpret_cast<const uint4*>(P);
    uint32_t base = block_off[blockIdx.x];
    for (uint32_t it = 0; it < 8; ++it) {
        const size_t q = (size_t)blockIdx.x * kChunkVec + it * 256 + threadIdx.x;
        const uint32_t v = (uint32_t)(q * 4);
        const uint4 p = P4[q];
        const uint32_t r0 = p.x == v, r1 = p.y == v + 1, r2 = p.z == v + 2, r3 = p.w == v + 3;
        const uint32_t cnt = r0 + r1 + r2 + r3;
        uint32_t total;
        const uint32_t before = base + wg_exclusive_256(cnt, wave_sum, &total);
        base += total;
        __syncthreads();                                       // wave_sum is written again in the next round
        if (r0) P[v] = kRankFlag | before;
        if (r1) P[v + 1] = kRankFlag | (before + r0);
        if (r2) P[v + 2] = kRankFlag | (before + r0 + r1);
        if (r3) P[v + 3] = kRankFlag | (before + r0 + r1 + r2);
    }
}

__global__ void __launch_bounds__(256)
comp_relabel(uint32_t* P, size_t nvec)
{
    uint4* P4 = reinterpret_cast<uint4*>(P);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nvec; q += stride) {
        const uint4 p = P4[q];
        uint32_t o[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (o[k] == kBg) { o[k] = 0u; continue; }
            if (!(o[k] & kRankFlag)) o[k] = ld(P, o[k]);       // the root's slot: its flagged rank, or its label if it was rewritten already
            if (o[k] & kRankFlag) o[k] = (o[k] & ~kRankFlag) + 1u;
        }
        P4[q] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

__global__ void __launch_bounds__(256)
comp_sizes(const uint4* __restrict__ L4, size_t nvec, uint32_t count, uint32_t* __restrict__ sizes)
{
    const uint32_t lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * 256;
    uint32_t acc_label = 0u, acc = 0u;           // wave-uniform: the label this wave sums in a register
    // nvec and the stride are multiples of 256: a wave is in or out as a whole
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nvec; q += stride) {
        const uint4 l = L4[q];
        const uint32_t a[4] = {l.x, l.y, l.z, l.w};
        uint32_t lab = 0u, c = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (a[k] == 0u || a[k] > count) continue;
            if (lab == 0u) lab = a[k];
            if (a[k] == lab) ++c;
            else atomicAdd(sizes + a[k] - 1u, 1u);             // a second label among the lane's four voxels
        }
        // runs of lanes with the same label: one sum per run, held by its last lane
        const uint32_t left = __shfl_up(lab, 1);
        const unsigned long long heads = __ballot(lane == 0 || lab != left);
        uint32_t incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += o;
        }
        const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
        const uint32_t prev = __shfl(incl, (int)(start ? start - 1u : 0u));
        const uint32_t seg = incl - (start ? prev : 0u);
        const bool tail = lab != 0u && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
        const unsigned long long tails = __ballot(tail);
        if (tails && acc_label == 0u) acc_label = __shfl(lab, __ffsll((long long)tails) - 1);
        uint32_t mine = (tail && lab == acc_label) ? seg : 0u;
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
        acc += mine;
        if (tail && lab != acc_label) atomicAdd(sizes + lab - 1u, seg);
    }
    if (lane == 0 && acc) atomicAdd(sizes + acc_label - 1u, acc);
}

__global__ void __launch_bounds__(256)
comp_keep_min(const uint32_t* __restrict__ sizes, uint32_t count, uint32_t v, uint8_t* __restrict__ keep)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < count; k += stride) keep[k] = sizes[k] >= v ? 1 : 0;
}

// round r of KEEP_LARGEST: best[r] = max over the labels that are none of best[0 .. r) of size << 32 | (0xFFFFFFFF - label)
__global__ void __launch_bounds__(256)
comp_argmax(const uint32_t* __restrict__ sizes, uint32_t count, unsigned long long* best, uint32_t r)
{
    __shared__ unsigned long long part[4];
    uint32_t won[16];
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) won[j] = j < r ? 0xFFFFFFFFu - (uint32_t)best[j] : 0u;
    unsigned long long top = 0ull;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < count; k += stride) {
        const uint32_t label = (uint32_t)k + 1u;
        bool taken = false;
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) taken |= won[j] == label;
        const unsigned long long key = ((unsigned long long)sizes[k] << 32) | (0xFFFFFFFFu - label);
        if (!taken && key > top) top = key;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(top, d);
        if (o > top) top = o;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = top;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) if (part[k] > top) top = part[k];
        if (top) atomicMax(best + r, top);
    }
}

__global__ void __launch_bounds__(64)
comp_keep_best(const unsigned long long* __restrict__ best, uint32_t rounds, uint8_t* __restrict__ keep)
{
    if (threadIdx.x < rounds && best[threadIdx.x]) keep[0xFFFFFFFFu - (uint32_t)best[threadIdx.x] - 1u] = 1;
}

__global__ void __launch_bounds__(256)
comp_write(const uint4* __restrict__ L4, size_t nvec, const uint8_t* __restrict__ keep, uint32_t* __restrict__ out, unsigned long long* kept)
{
    __shared__ uint32_t part[4];
    const uint32_t lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * 256;
    uint32_t cnt = 0;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nvec; q += stride) {
        const uint4 l = L4[q];
        uint32_t nib = 0u;
        if (l.x && keep[l.x - 1u]) nib |= 1u;
        if (l.y && keep[l.y - 1u]) nib |= 2u;
        if (l.z && keep[l.z - 1u]) nib |= 4u;
        if (l.w && keep[l.w - 1u]) nib |= 8u;
        cnt += __popc(nib);
        uint32_t word = nib << (4u * (lane & 7u));
        word |= __shfl_xor(word, 1);
        word |= __shfl_xor(word, 2);
        word |= __shfl_xor(word, 4);
        if ((lane & 7u) == 0) out[q >> 3] = word;
    }
    const uint32_t total = wg_sum_256(cnt, part);
    if (threadIdx.x == 0 && total) atomicAdd(kept, (unsigned long long)total);
}

unsigned stream_blocks(vp_ctx* ctx, size_t items)
{
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, (size_t)ctx->cus * 16));
}

// enqueues the whole labelling; K is left in comp_off[chunks]
int enqueue_label(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_labels, int conn, int algo)
{
    hipStream_t st = ctx->stream;
    const uint32_t w = n / 32;
    const size_t nvox = (size_t)n * n * n, nwords = nvox / 32, nvec = nvox / 4;
    const uint32_t chunks = (uint32_t)(nvox / kChunk);
    VP_TRY(reserve(ctx, ctx->comp.cnt, (size_t)chunks * 4));
    VP_TRY(reserve(ctx, ctx->comp.off, ((size_t)chunks + 1) * 4));
    uint32_t* cnt = (uint32_t*)ctx->comp.cnt.ptr;
    uint32_t* off = (uint32_t*)ctx->comp.off.ptr;
    if (algo == VP_ALGO_NAIVE) {
        const unsigned blocks = (unsigned)(nvox / 256);
        {
            ProfScope p(ctx, VP_K_COMP_INIT_NAIVE);
            hipLaunchKernelGGL(comp_init_naive, dim3(blocks), dim3(256), 0, st, d_words, d_labels, nvox);
        }
        ProfScope p(ctx, VP_K_COMP_MERGE_NAIVE);
        if (conn == VP_CONN_6) hipLaunchKernelGGL(comp_merge_naive<6>, dim3(blocks), dim3(256), 0, st, d_words, d_labels, n, nvox);
        else                   hipLaunchKernelGGL(comp_merge_naive<26>, dim3(blocks), dim3(256), 0, st, d_words, d_labels, n, nvox);
    } else {
        const uint32_t rpw = 64 / w;
        const size_t perBlock = (size_t)4 * rpw * w;
        {
            ProfScope p(ctx, VP_K_COMP_INIT);
            hipLaunchKernelGGL(comp_init_runs, dim3((unsigned)((nwords + perBlock - 1) / perBlock)), dim3(256), 0, st, d_words, d_labels, n, w, rpw);
        }
        const unsigned blocks = (unsigned)((nwords + 255) / 256);
        ProfScope p(ctx, VP_K_COMP_MERGE);
        if (conn == VP_CONN_6) hipLaunchKernelGGL(comp_merge_runs<6>, dim3(blocks), dim3(256), 0, st, d_words, d_labels, n, w, nwords);
        else                   hipLaunchKernelGGL(comp_merge_runs<26>, dim3(blocks), dim3(256), 0, st, d_words, d_labels, n, w, nwords);
    }
    {
        ProfScope p(ctx, VP_K_COMP_FLATTEN);
        hipLaunchKernelGGL(comp_flatten, dim3(chunks), dim3(256), 0, st, d_labels, cnt);
    }
    {
        ProfScope p(ctx, VP_K_COMP_RANK);
        hipLaunchKernelGGL(comp_scan, dim3(1), dim3(1024), 0, st, cnt, chunks, off);
        hipLaunchKernelGGL(comp_rank, dim3(chunks), dim3(256), 0, st, d_labels, off);
    }
    {
        ProfScope p(ctx, VP_K_COMP_RELABEL);
        hipLaunchKernelGGL(comp_relabel, dim3(stream_blocks(ctx, nvec)), dim3(256), 0, st, d_labels, nvec);
    }
    VP_HIP(hipGetLastError());
    return 0;
}

int enqueue_sizes(vp_ctx* ctx, uint32_t n, const uint32_t* d_labels, uint32_t count, uint32_t* d_sizes)
{
    const size_t nvec = (size_t)n * n * n / 4;
    VP_HIP(hipMemsetAsync(d_sizes, 0, (size_t)count * 4, ctx->stream));
    ProfScope p(ctx, VP_K_COMP_SIZES);
    hipLaunchKernelGGL(comp_sizes, dim3(stream_blocks(ctx, nvec)), dim3(256), 0, ctx->stream, (const uint4*)d_labels, nvec, count, d_sizes);
    VP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_components_label(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_labels, int conn, int algo, uint32_t* h_count)
{
    VP_TRY(ctx->comp.host.need(2));
    VP_TRY(enqueue_label(ctx, n, d_words, d_labels, conn, algo));
    const size_t chunks = (size_t)n * n * n / kChunk;
    VP_HIP(hipMemcpyAsync(ctx->comp.host, (const uint32_t*)ctx->comp.off.ptr + chunks, 4, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    if (h_count) *h_count = (uint32_t)ctx->comp.host[0];
    return 0;
}

int launch_components_sizes(vp_ctx* ctx, uint32_t n, const uint32_t* d_labels, uint32_t count, uint32_t* d_sizes)
{
    if (count == 0) return 0;
    VP_TRY(enqueue_sizes(ctx, n, d_labels, count, d_sizes));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int launch_components_filter(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_out, int conn, int mode, uint32_t param, int algo,
                             uint32_t* h_count, uint64_t* h_kept)
{
    hipStream_t st = ctx->stream;
    const size_t nvox = (size_t)n * n * n, nvec = nvox / 4, chunks = nvox / kChunk;
    VP_TRY(ctx->comp.host.need(2));
    VP_TRY(reserve(ctx, ctx->comp.labels, nvox * 4, false));
    VP_TRY(reserve(ctx, ctx->comp.small, 17 * sizeof(uint64_t), false));
    uint32_t* labels = (uint32_t*)ctx->comp.labels.ptr;
    unsigned long long* best = (unsigned long long*)ctx->comp.small.ptr;     // 16 winners of KEEP_LARGEST, then the kept voxels
    VP_TRY(enqueue_label(ctx, n, d_words, labels, conn, algo));
    // K sizes the size and keep arrays, so it is read back here; the kept count follows at the end
    VP_HIP(hipMemcpyAsync(ctx->comp.host, (const uint32_t*)ctx->comp.off.ptr + chunks, 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint32_t K = (uint32_t)ctx->comp.host[0];
    ctx->comp.host[1] = 0;
    if (K == 0) {
        VP_HIP(hipMemsetAsync(d_out, 0, nvox / 8, st));
    } else {
        VP_TRY(reserve(ctx, ctx->comp.sizes, (size_t)K * 4));
        VP_TRY(reserve(ctx, ctx->comp.keep, (size_t)K));
        uint32_t* sizes = (uint32_t*)ctx->comp.sizes.ptr;
        uint8_t* keep = (uint8_t*)ctx->comp.keep.ptr;
        VP_TRY(enqueue_sizes(ctx, n, labels, K, sizes));
        VP_HIP(hipMemsetAsync(best, 0, 17 * sizeof(uint64_t), st));
        {
            ProfScope p(ctx, VP_K_COMP_SELECT);
            if (mode == VP_COMP_MIN_VOXELS) {
                hipLaunchKernelGGL(comp_keep_min, dim3(stream_blocks(ctx, K)), dim3(256), 0, st, sizes, K, param, keep);
            } else {
                const uint32_t rounds = std::min(param, K);
                VP_HIP(hipMemsetAsync(keep, 0, K, st));
                for (uint32_t r = 0; r < rounds; ++r)
                    hipLaunchKernelGGL(comp_argmax, dim3(stream_blocks(ctx, K)), dim3(256), 0, st, sizes, K, best, r);
                hipLaunchKernelGGL(comp_keep_best, dim3(1), dim3(64), 0, st, best, rounds, keep);
            }
        }
        {
            ProfScope p(ctx, VP_K_COMP_WRITE);
            hipLaunchKernelGGL(comp_write, dim3(stream_blocks(ctx, nvec)), dim3(256), 0, st, (const uint4*)labels, nvec, keep, d_out, best + 16);
        }
        VP_HIP(hipGetLastError());
        VP_HIP(hipMemcpyAsync(ctx->comp.host + 1, best + 16, 8, hipMemcpyDeviceToHost, st));
    }
    VP_HIP(hipStreamSynchronize(st));
    if (h_count) *h_count = K;
    if (h_kept) *h_kept = ctx->comp.host[1];
    return 0;
}

}  // namespace vp
