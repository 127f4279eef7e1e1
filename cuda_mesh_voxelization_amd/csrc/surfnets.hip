// surfnets.hip -- surface nets (Gibson 1998) of a bit-packed grid: one vertex per boundary cell, one quad per exposed voxel face
// (include/vphip.h, vp_surfnets_*).  The next step up from extract.hip: two ordered compactions -- vertices and
// quads -- a rank lookup (a quad names the output index of four neighbouring cells) and an iterative gather (the relaxation).
//
// Cells: (cx, cy, cz) in -1 .. n-1, stored as (i, j, k) = (cx + 1, cy + 1, cz + 1) in 0 .. n; linear index i + (n+1) (j + (n+1) k).
// Corner dx + 2 dy + 4 dz of cell (i, j, k) is voxel (i - 1 + dx, j - 1 + dy, k - 1 + dz); voxels outside the grid are unset.
//
//   VP_ALGO_NAIVE  one thread per cell reads its eight voxel bits one by one; the rank lookup is a uint32 volume of (n+1)^3 vertex indices.
//   VP_ALGO_TILED  one lane per 32 cells of a cell row (rows of n/32 + 1 words: the 33rd, 65th, ... cell has a word of its own), eight
//                  corner words from two words of each of four voxel rows; the rank lookup is the active-cell bit volume plus one
//                  exclusive count per word: index = prefix[word] + popc(bits below).
// Both: per-block counts of vertices and quads (one launch), a one-workgroup scan of both count arrays, the vertex pass (records,
// starting positions, rank structure), the quad pass (gathers four ranks per quad) and one Jacobi launch per relaxation step.
#include "vp_internal.h"
#include "wg_scan.h"

namespace vp {

namespace {

constexpr int kBlock = 256;                         // cells (NAIVE) or cell words (TILED) per workgroup
constexpr uint32_t kNoVertex = 0xFFFFFFFFu;

struct Dim {
    uint32_t n, w;       // voxels per side, words per voxel row
    uint32_t n1, w1;     // cells per side n + 1, words per cell row n/32 + 1
};

__device__ __forceinline__ uint32_t voxel_bit(const Dim& d, const uint32_t* __restrict__ words, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x >= (int)d.n || y >= (int)d.n || z >= (int)d.n) return 0u;
    return (words[((size_t)z * d.n + y) * d.w + (x >> 5)] >> (x & 31)) & 1u;
}

// NAIVE: corner mask of cell (i, j, k), eight single-bit reads
__device__ __forceinline__ uint32_t cell_mask(const Dim& d, const uint32_t* __restrict__ words, int i, int j, int k)
{
    uint32_t m = 0;
    for (int c = 0; c < 8; ++c) m |= voxel_bit(d, words, i - 1 + (c & 1), j - 1 + ((c >> 1) & 1), k - 1 + (c >> 2)) << c;
    return m;
}

// TILED: the eight corner words of cell word wi of cell row (j, k): bit b of c[corner] = that corner of cell i = 32 wi + b
__device__ __forceinline__ void corner_words(const Dim& d, const uint32_t* __restrict__ words, uint32_t wi, int j, int k, uint32_t (&c)[8])
{
    for (int r = 0; r < 4; ++r) {
        const int y = j - 1 + (r & 1), z = k - 1 + (r >> 1);
        uint32_t cur = 0u, prev = 0u;
        if (y >= 0 && z >= 0 && y < (int)d.n && z < (int)d.n) {
            const uint32_t* row = words + ((size_t)z * d.n + y) * d.w;
            if (wi < d.w) cur = row[wi];
            if (wi > 0) prev = row[wi - 1];
        }
        c[2 * r] = (cur << 1) | (prev >> 31);       // dx = 0: voxel x = i - 1
        c[2 * r + 1] = cur;                         // dx = 1: voxel x = i
    }
}

__device__ __forceinline__ uint32_t active_word(const uint32_t (&c)[8])
{
    const uint32_t any = c[0] | c[1] | c[2] | c[3] | c[4] | c[5] | c[6] | c[7];
    const uint32_t all = c[0] & c[1] & c[2] & c[3] & c[4] & c[5] & c[6] & c[7];
    return any & ~all;
}

// the three edges a cell owns leave its corner 0 towards +x, +y, +z: corners 1, 2, 4
__device__ __forceinline__ uint32_t owned_edges(uint32_t mask)      // bit axis
{
    const uint32_t c0 = mask & 1u;
    return ((c0 ^ ((mask >> 1) & 1u))) | ((c0 ^ ((mask >> 2) & 1u)) << 1) | ((c0 ^ ((mask >> 4) & 1u)) << 2);
}

// the workgroup's vertex and quad counts in one sum (one barrier): v in the low half, q in the high half, no carry (v <= 32, q <= 96 per thread)
__device__ __forceinline__ void block_totals(uint32_t v, uint32_t q, uint32_t* __restrict__ cnt_v, uint32_t* __restrict__ cnt_q)
{
    __shared__ unsigned long long part[4];
    const unsigned long long both = wg_sum_256((unsigned long long)v | ((unsigned long long)q << 32), part);
    if (threadIdx.x == 0) { cnt_v[blockIdx.x] = (uint32_t)both; cnt_q[blockIdx.x] = (uint32_t)(both >> 32); }
}

// starting position of the vertex of a cell: the mean of the midpoints of its crossing edges (include/vphip.h)
__device__ __forceinline__ void start_position(uint32_t mask, int i, int j, int k, float (&p)[3])
{
    int m = 0, s[3] = {0, 0, 0};
    for (int axis = 0; axis < 3; ++axis)
        for (int c = 0; c < 8; ++c) {
            if ((c >> axis) & 1) continue;
            if ((((mask >> c) ^ (mask >> (c | (1 << axis)))) & 1u) == 0u) continue;
            ++m;
            for (int a = 0; a < 3; ++a) s[a] += a == axis ? 1 : 2 * ((c >> a) & 1);       // twice the midpoint's coordinate
        }
    const int cell[3] = {i - 1, j - 1, k - 1};
    for (int a = 0; a < 3; ++a) p[a] = ((float)cell[a] + 0.5f) + (float)s[a] / (float)(2 * m);
}

// ---- NAIVE ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
sn_count_naive(Dim d, const uint32_t* __restrict__ words, uint32_t ncells, uint32_t* __restrict__ cnt_v, uint32_t* __restrict__ cnt_q)
{
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    uint32_t v = 0, q = 0;
    if (c < ncells) {
        const uint32_t mask = cell_mask(d, words, (int)(c % d.n1), (int)((c / d.n1) % d.n1), (int)(c / (d.n1 * d.n1)));
        v = mask != 0u && mask != 255u;
        q = __popc(owned_edges(mask));
    }
    block_totals(v, q, cnt_v, cnt_q);
}

__global__ void __launch_bounds__(kBlock)
sn_verts_naive(Dim d, const uint32_t* __restrict__ words, uint32_t ncells, const unsigned long long* __restrict__ off_v,
               uint32_t* __restrict__ index, unsigned long long* __restrict__ cells, float* __restrict__ xyz, size_t capacity)
{
    __shared__ uint32_t smem[4];
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    const int i = (int)(c % d.n1), j = (int)((c / d.n1) % d.n1), k = (int)(c / (d.n1 * d.n1));
    uint32_t mask = 0;
    if (c < ncells) mask = cell_mask(d, words, i, j, k);
    const uint32_t v = mask != 0u && mask != 255u;
    const unsigned long long pos = off_v[blockIdx.x] + wg_exclusive_256(v, smem);
    if (c >= ncells) return;
    index[c] = v ? (uint32_t)pos : kNoVertex;
    if (v && pos < capacity) {
        cells[pos] = (unsigned long long)c | ((unsigned long long)mask << 40);
        float p[3];
        start_position(mask, i, j, k, p);
        xyz[3 * pos] = p[0]; xyz[3 * pos + 1] = p[1]; xyz[3 * pos + 2] = p[2];
    }
}

// the four cells around an owned edge, as offsets in the linear cell index (s1 = n + 1, s2 = (n + 1)^2), in the contract's order
__device__ __forceinline__ void quad_cells(int axis, uint32_t c, uint32_t s1, uint32_t s2, uint32_t (&q)[4])
{
    if (axis == 0)      { q[0] = c - s1 - s2; q[1] = c - s2; q[2] = c; q[3] = c - s1; }
    else if (axis == 1) { q[0] = c - 1 - s2;  q[1] = c - 1;  q[2] = c; q[3] = c - s2; }
    else                { q[0] = c - 1 - s1;  q[1] = c - s1; q[2] = c; q[3] = c - 1; }
}

__global__ void __launch_bounds__(kBlock)
sn_quads_naive(Dim d, const uint32_t* __restrict__ words, uint32_t ncells, const unsigned long long* __restrict__ off_q,
               const uint32_t* __restrict__ index, uint32_t* __restrict__ quads, size_t capacity)
{
    __shared__ uint32_t smem[4];
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    uint32_t mask = 0;
    if (c < ncells) mask = cell_mask(d, words, (int)(c % d.n1), (int)((c / d.n1) % d.n1), (int)(c / (d.n1 * d.n1)));
    const uint32_t own = owned_edges(mask);
    unsigned long long pos = off_q[blockIdx.x] + wg_exclusive_256(__popc(own), smem);
    for (int axis = 0; axis < 3; ++axis) {
        if (!((own >> axis) & 1u)) continue;
        uint32_t q[4];
        quad_cells(axis, c, d.n1, d.n1 * d.n1, q);
        if (pos < capacity) {
            const bool lower = (mask & 1u) != 0u;                    // the lower voxel of the pair is the set one: normal along + axis
            for (int t = 0; t < 4; ++t) quads[4 * pos + t] = index[q[lower ? t : 3 - t]];
        }
        ++pos;
    }
}

// ---- TILED ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
sn_count_tiled(Dim d, const uint32_t* __restrict__ words, uint32_t nwords, uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt_v,
               uint32_t* __restrict__ cnt_q)
{
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    uint32_t v = 0, q = 0;
    if (w < nwords) {
        const uint32_t wi = w % d.w1, row = w / d.w1;
        uint32_t c[8];
        corner_words(d, words, wi, (int)(row % d.n1), (int)(row / d.n1), c);
        const uint32_t act = active_word(c);
        bits[w] = act;
        v = __popc(act);
        q = __popc(c[0] ^ c[1]) + __popc(c[0] ^ c[2]) + __popc(c[0] ^ c[4]);
    }
    block_totals(v, q, cnt_v, cnt_q);
}

__global__ void __launch_bounds__(kBlock)
sn_verts_tiled(Dim d, const uint32_t* __restrict__ words, uint32_t nwords, const unsigned long long* __restrict__ off_v,
               uint32_t* __restrict__ prefix, unsigned long long* __restrict__ cells, float* __restrict__ xyz, size_t capacity)
{
    __shared__ uint32_t smem[4];
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t wi = w % d.w1, row = w / d.w1;
    const int j = (int)(row % d.n1), k = (int)(row / d.n1);
    uint32_t c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (w < nwords) corner_words(d, words, wi, j, k, c);
    uint32_t act = active_word(c);
    unsigned long long pos = off_v[blockIdx.x] + wg_exclusive_256(__popc(act), smem);
    if (w >= nwords) return;
    prefix[w] = (uint32_t)pos;
    while (act) {
        const int b = __ffs((int)act) - 1;
        act &= act - 1;
        uint32_t mask = 0;
        for (int t = 0; t < 8; ++t) mask |= ((c[t] >> b) & 1u) << t;
        if (pos < capacity) {
            const int i = (int)(wi * 32u) + b;
            cells[pos] = (unsigned long long)((uint32_t)i + d.n1 * row) | ((unsigned long long)mask << 40);
            float p[3];
            start_position(mask, i, j, k, p);
            xyz[3 * pos] = p[0]; xyz[3 * pos + 1] = p[1]; xyz[3 * pos + 2] = p[2];
        }
        ++pos;
    }
}

// vertex index of cell i of cell row `row` through the bit volume and its per-word exclusive counts
__device__ __forceinline__ uint32_t rank_of(const Dim& d, const uint32_t* __restrict__ bits, const uint32_t* __restrict__ prefix, uint32_t i, uint32_t row)
{
    const uint32_t w = row * d.w1 + (i >> 5);
    return prefix[w] + __popc(bits[w] & ((1u << (i & 31u)) - 1u));
}

__global__ void __launch_bounds__(kBlock)
sn_quads_tiled(Dim d, const uint32_t* __restrict__ words, uint32_t nwords, const unsigned long long* __restrict__ off_q,
               const uint32_t* __restrict__ bits, const uint32_t* __restrict__ prefix, uint32_t* __restrict__ quads, size_t capacity)
{
    __shared__ uint32_t smem[4];
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t wi = w % d.w1, row = w / d.w1;
    uint32_t c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (w < nwords) corner_words(d, words, wi, (int)(row % d.n1), (int)(row / d.n1), c);
    const uint32_t e[3] = {c[0] ^ c[1], c[0] ^ c[2], c[0] ^ c[4]};
    uint32_t any = e[0] | e[1] | e[2];
    unsigned long long pos = off_q[blockIdx.x] + wg_exclusive_256(__popc(e[0]) + __popc(e[1]) + __popc(e[2]), smem);
    while (any) {
        const int b = __ffs((int)any) - 1;
        any &= any - 1;
        const uint32_t i = wi * 32u + (uint32_t)b;
        const bool lower = ((c[0] >> b) & 1u) != 0u;
        for (int axis = 0; axis < 3; ++axis) {
            if (!((e[axis] >> b) & 1u)) continue;
            // (cell column, cell row) of the four cells, in the contract's order; an owned edge has every one of them inside the cell range
            uint32_t qi[4], qr[4];
            if (axis == 0)      { qi[0] = i;     qr[0] = row - 1 - d.n1; qi[1] = i;     qr[1] = row - d.n1; qi[2] = i; qr[2] = row; qi[3] = i;     qr[3] = row - 1; }
            else if (axis == 1) { qi[0] = i - 1; qr[0] = row - d.n1;     qi[1] = i - 1; qr[1] = row;        qi[2] = i; qr[2] = row; qi[3] = i;     qr[3] = row - d.n1; }
            else                { qi[0] = i - 1; qr[0] = row - 1;        qi[1] = i;     qr[1] = row - 1;    qi[2] = i; qr[2] = row; qi[3] = i - 1; qr[3] = row; }
            if (pos < capacity)
                for (int t = 0; t < 4; ++t) { const int s = lower ? t : 3 - t; quads[4 * pos + t] = rank_of(d, bits, prefix, qi[s], qr[s]); }
            ++pos;
        }
    }
}

// ---- scan of the two block-count arrays by one workgroup: off[i] = sum of cnt[0..i), off[m] = total ----------------
__global__ void __launch_bounds__(1024)
sn_scan(const uint32_t* __restrict__ cnt_v, const uint32_t* __restrict__ cnt_q, size_t m, unsigned long long* __restrict__ off_v,
        unsigned long long* __restrict__ off_q)
{
    __shared__ unsigned long long part[1024];
    for (int which = 0; which < 2; ++which) {
        const uint32_t* cnt = which ? cnt_q : cnt_v;
        unsigned long long* off = which ? off_q : off_v;
        const unsigned long long total = wg_scan_1024(part, m, [&](size_t i) { return (unsigned long long)cnt[i]; },
                                                      [&](size_t i, unsigned long long before) { off[i] = before; });
        if (threadIdx.x == 1023) off[m] = total;
    }
}

// ---- relaxation: one Jacobi step, one lane per vertex ------------------------------------------------------------
// TILED = false: the rank lookup is the index volume; true: bits + prefix.  A neighbour across a face exists iff the face's four corners
// are mixed; the sum runs over -x, +x, -y, +y, -z, +z in that order, then one division and the clamp to the cell shrunk by 1/16.
template <bool TILED>
__global__ void __launch_bounds__(kBlock)
sn_relax(Dim d, const unsigned long long* __restrict__ cells, uint32_t nverts, const uint32_t* __restrict__ index_or_bits,
         const uint32_t* __restrict__ prefix, const float* __restrict__ in, float* __restrict__ out)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nverts) return;
    const unsigned long long rec = cells[v];
    const uint32_t c = (uint32_t)(rec & ((1ull << 40) - 1ull)), mask = (uint32_t)(rec >> 40) & 255u;
    const uint32_t i = c % d.n1, row = c / d.n1;
    const uint32_t face[6] = {0x55u, 0xAAu, 0x33u, 0xCCu, 0x0Fu, 0xF0u};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int deg = 0;
    for (int f = 0; f < 6; ++f) {
        const uint32_t m = mask & face[f];
        if (m == 0u || m == face[f]) continue;
        uint32_t ni = i, nrow = row;
        if (f == 0) ni = i - 1; else if (f == 1) ni = i + 1;
        else if (f == 2) nrow = row - 1; else if (f == 3) nrow = row + 1;
        else if (f == 4) nrow = row - d.n1; else nrow = row + d.n1;
        uint32_t u = TILED ? rank_of(d, index_or_bits, prefix, ni, nrow) : index_or_bits[ni + d.n1 * nrow];
        if (u >= nverts) u = v;                                     // never on a grid the count was taken from
        if (deg == 0) { acc[0] = in[3 * (size_t)u]; acc[1] = in[3 * (size_t)u + 1]; acc[2] = in[3 * (size_t)u + 2]; }
        else { acc[0] += in[3 * (size_t)u]; acc[1] += in[3 * (size_t)u + 1]; acc[2] += in[3 * (size_t)u + 2]; }
        ++deg;
    }
    if (deg == 0) { for (int a = 0; a < 3; ++a) out[3 * (size_t)v + a] = in[3 * (size_t)v + a]; return; }    // no active cell has none
    const int cell[3] = {(int)i - 1, (int)(row % d.n1) - 1, (int)(row / d.n1) - 1};
    for (int a = 0; a < 3; ++a) {
        const float q = acc[a] / (float)deg;
        const float lo = (float)cell[a] + 0.5625f, hi = (float)cell[a] + 1.4375f;
        out[3 * (size_t)v + a] = fminf(fmaxf(q, lo), hi);
    }
}

Dim make_dim(uint32_t n) { Dim d; d.n = n; d.w = n / 32; d.n1 = n + 1; d.w1 = n / 32 + 1; return d; }

size_t unit_count(const Dim& d, int algo)        // cells (NAIVE) or cell words (TILED)
{
    return algo == VP_ALGO_NAIVE ? (size_t)d.n1 * d.n1 * d.n1 : (size_t)d.w1 * d.n1 * d.n1;
}

}  // namespace

// Counts vertices and quads (blocking: the totals are read back) and leaves the block offsets -- TILED: and the active-cell bit volume --
// in the context for launch_surfnets_write.
int launch_surfnets_count(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, int algo, uint64_t* h_vertices, uint64_t* h_quads)
{
    const Dim d = make_dim(n);
    const size_t units = unit_count(d, algo);
    const size_t blocks = (units + kBlock - 1) / kBlock;
    ctx->sn.words = nullptr;
    VP_TRY(reserve(ctx, ctx->sn.cnt, blocks * 8));
    VP_TRY(reserve(ctx, ctx->sn.off, (blocks + 1) * 16));
    if (algo == VP_ALGO_TILED) VP_TRY(reserve(ctx, ctx->sn.rank, units * 8));          // bits, then the per-word exclusive counts
    uint32_t* cnt_v = (uint32_t*)ctx->sn.cnt.ptr;
    uint32_t* cnt_q = cnt_v + blocks;
    unsigned long long* off_v = (unsigned long long*)ctx->sn.off.ptr;
    unsigned long long* off_q = off_v + blocks + 1;
    {
        ProfScope p(ctx, algo == VP_ALGO_NAIVE ? VP_K_SN_CELLS_NAIVE : VP_K_SN_CELLS);
        if (algo == VP_ALGO_NAIVE)
            hipLaunchKernelGGL(sn_count_naive, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d, d_words, (uint32_t)units, cnt_v, cnt_q);
        else
            hipLaunchKernelGGL(sn_count_tiled, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d, d_words, (uint32_t)units,
                               (uint32_t*)ctx->sn.rank.ptr, cnt_v, cnt_q);
    }
    {
        ProfScope p(ctx, VP_K_SN_SCAN);
        hipLaunchKernelGGL(sn_scan, dim3(1), dim3(1024), 0, ctx->stream, cnt_v, cnt_q, blocks, off_v, off_q);
    }
    VP_HIP(hipGetLastError());
    unsigned long long totals[2] = {0, 0};
    VP_HIP(hipMemcpyAsync(&totals[0], off_v + blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(hipMemcpyAsync(&totals[1], off_q + blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sn.words = d_words; ctx->sn.n = n; ctx->sn.algo = algo; ctx->sn.vertices = totals[0]; ctx->sn.quads = totals[1];
    if (h_vertices) *h_vertices = totals[0];
    if (h_quads) *h_quads = totals[1];
    return 0;
}

int launch_surfnets_write(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, int algo, uint32_t iterations, uint64_t* d_cells, float* d_xyz,
                          uint32_t* d_quads, const IsoField* iso)
{
    const Dim d = make_dim(n);
    const size_t units = unit_count(d, algo);
    const size_t blocks = (units + kBlock - 1) / kBlock;
    const size_t nv = (size_t)ctx->sn.vertices, nq = (size_t)ctx->sn.quads;
    if (nv == 0) return 0;                                                // no vertex, hence no quad
    const bool naive = algo == VP_ALGO_NAIVE;
    // the buffers below may regrow: that frees nothing the count left behind (sn_off, and the bits at the front of sn_rank, which the
    // count already reserved at full size)
    if (naive) VP_TRY(reserve(ctx, ctx->sn.rank, units * 4, false));      // vertex-index volume, 4 (n+1)^3 bytes
    if (iterations) VP_TRY(reserve(ctx, ctx->sn.xyz, nv * 12));
    const unsigned long long* off_v = (const unsigned long long*)ctx->sn.off.ptr;
    const unsigned long long* off_q = off_v + blocks + 1;
    uint32_t* rank0 = (uint32_t*)ctx->sn.rank.ptr;                        // NAIVE: index volume; TILED: bits
    uint32_t* prefix = naive ? nullptr : rank0 + units;
    float* other = (float*)ctx->sn.xyz.ptr;
    float* cur = (iterations & 1u) ? other : d_xyz;                       // the result ends in d_xyz for any iteration count
    {
        ProfScope p(ctx, naive ? VP_K_SN_VERTS_NAIVE : VP_K_SN_VERTS);
        if (naive)
            hipLaunchKernelGGL(sn_verts_naive, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d, d_words, (uint32_t)units, off_v, rank0,
                               (unsigned long long*)d_cells, cur, nv);
        else
            hipLaunchKernelGGL(sn_verts_tiled, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d, d_words, (uint32_t)units, off_v, prefix,
                               (unsigned long long*)d_cells, cur, nv);
    }
    if (iso) VP_TRY(launch_iso_place(ctx, n, algo, *iso, d_cells, rank0, cur, nv));      // vp_isonets: positions from the field, not the bits
    {
        ProfScope p(ctx, naive ? VP_K_SN_QUADS_NAIVE : VP_K_SN_QUADS);
        if (naive)
            hipLaunchKernelGGL(sn_quads_naive, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d, d_words, (uint32_t)units, off_q, rank0,
                               d_quads, nq);
        else
            hipLaunchKernelGGL(sn_quads_tiled, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d, d_words, (uint32_t)units, off_q, rank0,
                               prefix, d_quads, nq);
    }
    const unsigned vblocks = (unsigned)((nv + kBlock - 1) / kBlock);
    for (uint32_t it = 0; it < iterations; ++it) {
        float* next = cur == d_xyz ? other : d_xyz;
        ProfScope p(ctx, naive ? VP_K_SN_RELAX_NAIVE : VP_K_SN_RELAX);
        if (naive)
            hipLaunchKernelGGL(sn_relax<false>, dim3(vblocks), dim3(kBlock), 0, ctx->stream, d, (const unsigned long long*)d_cells, (uint32_t)nv,
                               rank0, prefix, cur, next);
        else
            hipLaunchKernelGGL(sn_relax<true>, dim3(vblocks), dim3(kBlock), 0, ctx->stream, d, (const unsigned long long*)d_cells, (uint32_t)nv,
                               rank0, prefix, cur, next);
        cur = next;
    }
    VP_HIP(hipGetLastError());
    return 0;
}

}  // namespace vp
