// regions.hip -- region analysis of a label volume, whole grids, for gfx950 (MI355X): vp_regions (include/vphip.h).
//
// Per label k = 1 .. K a record of VP_REGION_WORDS = 26 unsigned 64-bit words: the voxel count, the bounding box, the first and second moments
// of the integer voxel coordinates, the exposed faces per axis, the contact faces, the lattice points n0 and lattice edges n1 of the closed
// cube complex, sum / min / max of an optional value field and the lowest linear index.  The effective label of a voxel is W(v) where
// 1 <= W(v) <= K, else 0; outside the grid it is 0.  Every word is an integer sum, minimum or maximum over voxels: the atomics commute, so the
// table does not depend on the order of execution and kernel boundaries are the only synchronisation.
//   both   rg_clear   one lane per table word: 0, or all ones for the words that take a minimum (1 - 3, 23, 25)
//          rg_finish  one lane per label: an empty label's record becomes all zero (its minima still hold all ones), words 22 - 24 are zero
//                     without a value field; the totals of the statistics (workgroup sums, one atomic each)
//   NAIVE  rg_naive   one lane per voxel from global memory: its 26 neighbours, then the 26 global 64-bit atomics of a run of one voxel
//   TILED  rg_tiled   one workgroup per block of 32 x 16 x 16 voxels, 256 lanes.  The effective labels of the block and a one-voxel halo are
//                     staged in LDS (the tile of block_list.h = 45,360 B), the values of the block beside them (256 rows,
//                     pitch 33 = 33,792 B).  A lane whose x row holds no label does nothing; every other lane walks its row with the three
//                     columns of nine labels around the voxel in registers and keeps
//                     the RUN of its current label -- consecutive voxels of one label in that row -- in registers, in coordinates local to
//                     the block; y and z are constant along a run, so a run carries V, sum lx, sum lx^2, lo and hi of lx, the six counts
//                     and the values.  At a change of label the run is flushed into one of 16 label slots in LDS, claimed with a
//                     compare-and-swap on the slot's key, with 32-bit LDS atomics (the value sum: one 64-bit LDS atomic).  After a barrier
//                     the occupied slots are shifted to grid coordinates in 64-bit arithmetic, one lane per word, and go out with 26 global
//                     atomics per (block, label).  A run whose label finds no free slot goes to the table directly, as NAIVE's voxels do.
// The 26 equalities of a voxel against its neighbourhood are computed once (bit dx+1 + 3 (dy+1) + 9 (dz+1); bits 0 .. 12 are the neighbours with
// a LOWER linear index): a face is exposed iff its bit is clear; the voxel OWNS a lattice point (edge) iff none of the other seven (three)
// voxels incident on it has the same label and a lower linear index.  Every lattice point (edge) with at least one incident voxel of k has
// exactly one owner in k -- the incident voxel of k with the lowest index -- so the sum of owned elements is n0 (n1), with one writer each.
// Bounds.  Grid: n <= 1024, so sum x^2 <= 1023^2 * 2^30 < 2^51, sum xy likewise, sum of values <= (2^32 - 1) * 2^30 < 2^62, the face, point
// and edge counts <= 12 * 2^30: every word fits 64 bits.  Block-local (a slot): at most 8192 voxels with lx <= 31, ly, lz <= 15, so
// sum lx^2 <= 31^2 * 8192 < 2^23 and every other sum is smaller; counts <= 12 * 8192: every slot word fits 32 bits (the value sum is kept
// in 64).  Every device loop has a compile-time bound.
#include "block_list.h"
#include "vp_internal.h"

namespace vp {

namespace {

constexpr uint32_t kWords = VP_REGION_WORDS;
constexpr uint32_t kValPitch = 33;                                 // values of one x row of the block, pitch in values
constexpr uint32_t kSlots = 16;                                    // label slots of a block
// the words that take a minimum / a maximum; every other word is a sum
constexpr uint32_t kMinWords = (1u << 1) | (1u << 2) | (1u << 3) | (1u << 23) | (1u << 25);
constexpr uint32_t kMaxWords = (1u << 4) | (1u << 5) | (1u << 6) | (1u << 24);
constexpr uint32_t kValueWords = (1u << 22) | (1u << 23) | (1u << 24);
// counters, 64-bit words: sum V | labels with V > 0 | voxels with W > K | sum of the contact faces
constexpr uint32_t kCntVoxels = 0, kCntLabels = 1, kCntIgnored = 2, kCntContact = 3;

constexpr uint32_t nb_bit(int dx, int dy, int dz) { return (uint32_t)((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)); }
constexpr uint32_t kFaceBits = (1u << nb_bit(-1, 0, 0)) | (1u << nb_bit(1, 0, 0)) | (1u << nb_bit(0, -1, 0)) | (1u << nb_bit(0, 1, 0)) |
                               (1u << nb_bit(0, 0, -1)) | (1u << nb_bit(0, 0, 1));
constexpr uint32_t kLower = (1u << 13) - 1u;                       // the neighbours with a lower linear index

// corner c = cx + 2 cy + 4 cz of a voxel: the other voxels incident on that lattice point that have a lower linear index
constexpr uint32_t corner_mask(int c)
{
    uint32_t m = 0;
    for (int a = 0; a < 8; ++a) {
        const int dx = (c & 1) - 1 + (a & 1), dy = ((c >> 1) & 1) - 1 + ((a >> 1) & 1), dz = ((c >> 2) & 1) - 1 + ((a >> 2) & 1);
        m |= 1u << nb_bit(dx, dy, dz);
    }
    return m & kLower;
}
// edge e = 4 axis + ca + 2 cb of a voxel: the other voxels incident on that lattice edge that have a lower linear index
constexpr uint32_t edge_mask(int e)
{
    uint32_t m = 0;
    const int axis = e >> 2;
    for (int a = 0; a < 4; ++a) {
        const int d1 = (e & 1) - 1 + (a & 1), d2 = ((e >> 1) & 1) - 1 + ((a >> 1) & 1);
        m |= 1u << (axis == 0 ? nb_bit(0, d1, d2) : axis == 1 ? nb_bit(d1, 0, d2) : nb_bit(d1, d2, 0));
    }
    return m & kLower;
}

// consecutive voxels of one label in one x row, x relative to some x0: V, sum x, sum x^2, lowest and highest x, the counts, the values
struct Run {
    uint32_t v, sx, sxx, lo, hi, fx, fy, fz, ct, n0, n1, vmin, vmax;
    unsigned long long sval;
};

__device__ __forceinline__ Run run_at(uint32_t x) { return Run{0u, 0u, 0u, x, x, 0u, 0u, 0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0ull}; }

// one voxel at x joins the run: eq = its neighbours with its own label, nz = its neighbours with any label
__device__ __forceinline__ void run_add(Run& r, uint32_t x, uint32_t eq, uint32_t nz)
{
    const uint32_t open = ~eq;
    r.v += 1u; r.sx += x; r.sxx += x * x; r.hi = x;
    r.fx += ((open >> nb_bit(-1, 0, 0)) & 1u) + ((open >> nb_bit(1, 0, 0)) & 1u);
    r.fy += ((open >> nb_bit(0, -1, 0)) & 1u) + ((open >> nb_bit(0, 1, 0)) & 1u);
    r.fz += ((open >> nb_bit(0, 0, -1)) & 1u) + ((open >> nb_bit(0, 0, 1)) & 1u);
    r.ct += (uint32_t)__popc(open & nz & kFaceBits);
#pragma unroll
    for (int c = 0; c < 8; ++c) r.n0 += (eq & corner_mask(c)) == 0u;
#pragma unroll
    for (int e = 0; e < 12; ++e) r.n1 += (eq & edge_mask(e)) == 0u;
}

__device__ __forceinline__ void run_value(Run& r, uint32_t value)
{
    r.sval += value; r.vmin = min(r.vmin, value); r.vmax = max(r.vmax, value);
}

template <typename T> __device__ __forceinline__ void put_add(T* p, T v) { if (v) atomicAdd(p, v); }

// the run of the row (y, z), its x relative to x0, into a record of words of type T -- the table (64-bit, grid coordinates) or a slot (32-bit,
// block coordinates: x0 = 0); vsum = where the value sum of the record lives, first = the linear index of the run's first voxel
template <typename T>
__device__ __forceinline__ void run_put(T* rec, unsigned long long* vsum, const Run& r, T x0, T y, T z, T first, bool values)
{
    const T v = r.v, sx = (T)r.sx + v * x0;
    atomicAdd(rec + 0, v);
    atomicMin(rec + 1, (T)r.lo + x0); atomicMin(rec + 2, y); atomicMin(rec + 3, z);
    atomicMax(rec + 4, (T)r.hi + x0); atomicMax(rec + 5, y); atomicMax(rec + 6, z);
    put_add(rec + 7, sx); put_add(rec + 8, v * y); put_add(rec + 9, v * z);
    put_add(rec + 10, (T)r.sxx + (T)2 * x0 * (T)r.sx + v * x0 * x0); put_add(rec + 11, v * y * y); put_add(rec + 12, v * z * z);
    put_add(rec + 13, sx * y); put_add(rec + 14, sx * z); put_add(rec + 15, v * y * z);
    put_add(rec + 16, (T)r.fx); put_add(rec + 17, (T)r.fy); put_add(rec + 18, (T)r.fz); put_add(rec + 19, (T)r.ct);
    put_add(rec + 20, (T)r.n0); put_add(rec + 21, (T)r.n1);
    if (values) {
        put_add(vsum, r.sval);
        atomicMin(rec + 23, (T)r.vmin); atomicMax(rec + 24, (T)r.vmax);
    }
    atomicMin(rec + 25, first);
}

__device__ __forceinline__ void run_to_table(unsigned long long* __restrict__ table, uint32_t label, const Run& r, uint32_t x0, uint32_t y, uint32_t z,
                                             uint32_t n, bool values)
{
    unsigned long long* rec = table + (size_t)(label - 1u) * kWords;
    run_put<unsigned long long>(rec, rec + 22, r, x0, y, z, r.lo + x0 + (unsigned long long)n * (y + (unsigned long long)n * z), values);
}

// ---- both --------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
rg_clear(unsigned long long* __restrict__ table, size_t words)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) table[i] = ((kMinWords >> (uint32_t)(i % kWords)) & 1u) ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(256)
rg_finish(unsigned long long* __restrict__ table, uint32_t count, int values, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[3][4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    unsigned long long v = 0ull, contact = 0ull;
    if (k < count) {
        unsigned long long* rec = table + (size_t)k * kWords;
        v = rec[0];
        contact = rec[19];
        if (v == 0ull) {
#pragma unroll
            for (uint32_t j = 0; j < kWords; ++j)
                if ((kMinWords >> j) & 1u) rec[j] = 0ull;
        } else if (!values) {
            rec[23] = 0ull;
        }
    }
    const unsigned long long voxels = wg_sum_256(v, smem[0]);
    const unsigned long long labels = wg_sum_256((unsigned long long)(v != 0ull), smem[1]);
    const unsigned long long faces = wg_sum_256(contact, smem[2]);
    if (threadIdx.x == 0) {
        if (voxels) atomicAdd(&counters[kCntVoxels], voxels);
        if (labels) atomicAdd(&counters[kCntLabels], labels);
        if (faces) atomicAdd(&counters[kCntContact], faces);
    }
}

// ---- NAIVE -------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
rg_naive(const uint32_t* __restrict__ W, const uint32_t* __restrict__ values, uint32_t n, uint32_t count, unsigned long long* __restrict__ table,
         unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long smem[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t x = (uint32_t)(i % n), y = (uint32_t)((i / n) % n), z = (uint32_t)(i / ((size_t)n * n));
    const uint32_t w = W[i];
    if (w >= 1u && w <= count) {
        uint32_t eq = 0u, nz = 0u;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
            if (k == 13) continue;
            const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
            if (qx >= n || qy >= n || qz >= n) continue;             // outside the grid: label 0
            const uint32_t l = W[qx + (size_t)n * (qy + (size_t)n * qz)];
            eq |= (uint32_t)(l == w) << k;
            nz |= (uint32_t)(l >= 1u && l <= count) << k;
        }
        Run r = run_at(x);
        run_add(r, x, eq, nz);
        if (values) run_value(r, values[i]);
        run_to_table(table, w, r, 0u, y, z, n, values != nullptr);
    }
    const unsigned long long ignored = wg_sum_256((unsigned long long)(w > count), smem);
    if (threadIdx.x == 0 && ignored) atomicAdd(&counters[kCntIgnored], ignored);
}

// ---- TILED -------------------------------------------------------------------------------------------------------------------------

// the nine labels of column c around the row at `row`, j = dy + 1 + 3 (dz + 1)
__device__ __forceinline__ void rg_column(const uint32_t* row, uint32_t c, uint32_t (&col)[9])
{
    constexpr int P = (int)kRowPitch, Z = (int)(kHalo * kRowPitch);
#pragma unroll
    for (int j = 0; j < 9; ++j) col[j] = row[(int)c + (j % 3 - 1) * P + (j / 3 - 1) * Z];
}

__global__ void __launch_bounds__(256)
rg_tiled(const uint32_t* __restrict__ W, const uint32_t* __restrict__ values, uint32_t n, uint32_t count, unsigned long long* __restrict__ table,
         unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t tile[kHalo * kHalo * kRowPitch];
    __shared__ uint32_t vtile[256 * kValPitch];
    __shared__ uint32_t keys[kSlots];                              // the label a slot serves, 0: free
    __shared__ uint32_t slots[kSlots][kWords];                     // its record in block coordinates, word 22 unused
    __shared__ unsigned long long slot_values[kSlots];             // its value sum
    __shared__ unsigned long long smem[4];
    const uint32_t t = threadIdx.x;
    const BlockAt at = block_at(blockIdx.x, n);
    const uint32_t x0 = at.x0(), y0 = at.y0(), z0 = at.z0();
    uint32_t ignored = 0u;
    stage_halo(tile, at, n, [&](uint32_t x, uint32_t y, uint32_t z, bool inside, uint32_t c, uint32_t ry, uint32_t rz) {
        if (!inside) return 0u;
        const uint32_t l = W[x + (size_t)n * (y + (size_t)n * z)];
        if (l <= count) return l;
        ignored += c >= 1u && c <= 32u && ry >= 1u && ry <= kBlockY && rz >= 1u && rz <= kBlockZ;   // counted by its own block
        return 0u;
    });
    if (values) {
#pragma unroll 4
        for (uint32_t k = 0; k < 32u; ++k) {                       // lanes along x: row r of the block, voxel x
            const uint32_t e = k * 256u + t, x = e & 31u, r = e >> 5;
            vtile[r * kValPitch + x] = values[at.voxel(n, x, r & 15u, r >> 4)];
        }
    }
    if (t < kSlots) { keys[t] = 0u; slot_values[t] = 0ull; }
    for (uint32_t e = t; e < kSlots * kWords; e += 256u) slots[e / kWords][e % kWords] = ((kMinWords >> (e % kWords)) & 1u) ? 0xFFFFFFFFu : 0u;
    __syncthreads();

    const uint32_t ly = t & 15u, lz = t >> 4;
    const uint32_t* row = tile_row(tile, ly, lz);
    const uint32_t* vrow = vtile + t * kValPitch;
    uint32_t any = 0u;                                             // a row without a label (most rows of most grids) is not walked
#pragma unroll
    for (uint32_t c = 1; c <= 32u; ++c) any |= row[c];
    uint32_t left[9], mid[9], right[9];
    rg_column(row, 0u, left);
    rg_column(row, 1u, mid);
    uint32_t cur = 0u;
    Run r = run_at(0u);
#pragma unroll 1
    for (uint32_t x = 0; any != 0u && x <= 32u; ++x) {             // x = 32 ends the row: the last run is flushed like every other
        uint32_t l = 0u;
        if (x < 32u) {
            rg_column(row, x + 2u, right);
            l = mid[4];
        }
        if (l != cur) {
            if (cur != 0u) {
                uint32_t s = kSlots;
#pragma unroll 1
                for (uint32_t j = 0; j < kSlots; ++j) {
                    uint32_t held = __hip_atomic_load(&keys[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (held == 0u) held = atomicCAS(&keys[j], 0u, cur);     // a key goes from 0 to its label once and stays
                    if (held == 0u || held == cur) { s = j; break; }
                }
                if (s < kSlots) run_put<uint32_t>(slots[s], &slot_values[s], r, 0u, ly, lz, r.lo + 32u * (ly + kBlockY * lz), values != nullptr);
                else run_to_table(table, cur, r, x0, y0 + ly, z0 + lz, n, values != nullptr);
            }
            cur = l;
            r = run_at(x);
        }
        if (l != 0u) {
            uint32_t eq = 0u;
#pragma unroll
            for (int j = 0; j < 9; ++j)
                eq |= ((uint32_t)(left[j] == l) << (3 * j)) | ((uint32_t)(mid[j] == l) << (3 * j + 1)) | ((uint32_t)(right[j] == l) << (3 * j + 2));
            const uint32_t nz = ((uint32_t)(left[4] != 0u) << nb_bit(-1, 0, 0)) | ((uint32_t)(right[4] != 0u) << nb_bit(1, 0, 0)) |
                                ((uint32_t)(mid[3] != 0u) << nb_bit(0, -1, 0)) | ((uint32_t)(mid[5] != 0u) << nb_bit(0, 1, 0)) |
                                ((uint32_t)(mid[1] != 0u) << nb_bit(0, 0, -1)) | ((uint32_t)(mid[7] != 0u) << nb_bit(0, 0, 1));
            run_add(r, x, eq & ~(1u << 13), nz);
            if (values) run_value(r, vrow[x]);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) { left[j] = mid[j]; mid[j] = right[j]; }
    }
    __syncthreads();

    // the occupied slots to grid coordinates, one lane per word: sum x = sum lx + V x0, sum x^2 = sum lx^2 + 2 x0 sum lx + V x0^2,
    // sum xy = sum lx ly + x0 sum ly + y0 sum lx + V x0 y0
    for (uint32_t e = t; e < kSlots * kWords; e += 256u) {
        const uint32_t s = e / kWords, j = e % kWords, label = keys[s];
        if (label == 0u || (!values && ((kValueWords >> j) & 1u))) continue;
        const uint32_t* q = slots[s];
        const unsigned long long V = q[0], X = x0, Y = y0, Z = z0;
        unsigned long long v = q[j];
        switch (j) {
            case 1: case 4: case 7: v += (j == 7 ? V : 1ull) * X; break;
            case 2: case 5: case 8: v += (j == 8 ? V : 1ull) * Y; break;
            case 3: case 6: case 9: v += (j == 9 ? V : 1ull) * Z; break;
            case 10: v += 2ull * X * q[7] + V * X * X; break;
            case 11: v += 2ull * Y * q[8] + V * Y * Y; break;
            case 12: v += 2ull * Z * q[9] + V * Z * Z; break;
            case 13: v += X * q[8] + Y * q[7] + V * X * Y; break;
            case 14: v += X * q[9] + Z * q[7] + V * X * Z; break;
            case 15: v += Y * q[9] + Z * q[8] + V * Y * Z; break;
            case 22: v = slot_values[s]; break;
            case 25: v = X + (v & 31u) + (unsigned long long)n * (Y + ((v >> 5) & 15u) + (unsigned long long)n * (Z + (v >> 9))); break;
            default: break;
        }
        unsigned long long* dst = table + (size_t)(label - 1u) * kWords + j;
        if ((kMinWords >> j) & 1u) atomicMin(dst, v);
        else if ((kMaxWords >> j) & 1u) atomicMax(dst, v);
        else if (v) atomicAdd(dst, v);
    }
    const unsigned long long sum = wg_sum_256((unsigned long long)ignored, smem);
    if (t == 0 && sum) atomicAdd(&counters[kCntIgnored], sum);
}

}  // namespace

// The caller has validated everything.  Blocks once: the four totals are read back.
int launch_regions(vp_ctx* ctx, const Frame& f, const uint32_t* d_labels, uint32_t count, const uint32_t* d_values, int algo, uint64_t* h_stats)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = f.n;
    const size_t voxels = (size_t)n * n * n, words = (size_t)count * kWords;
    ctx->rg.n = 0;                                                 // from here on the previous result is gone
    ctx->rg.count = 0;
    VP_TRY(reserve(ctx, ctx->rg.table, words * 8, false));
    VP_TRY(reserve(ctx, ctx->rg.aux, kAuxHead, false));
    VP_TRY(ctx->rg.host.need(4));
    unsigned long long* table = (unsigned long long*)ctx->rg.table.ptr;
    unsigned long long* counters = (unsigned long long*)ctx->rg.aux.ptr;
    VP_HIP(hipMemsetAsync(counters, 0, kAuxHead, st));
    if (count) {
        ProfScope p(ctx, VP_K_MD_FILL);
        hipLaunchKernelGGL(rg_clear, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, table, words);
    }
    if (algo == VP_ALGO_TILED) {
        ProfScope p(ctx, VP_K_MD_BRICK);
        hipLaunchKernelGGL(rg_tiled, dim3(block_count(n)), dim3(256), 0, st, d_labels, d_values, n, count, table, counters);
    } else {
        ProfScope p(ctx, VP_K_MD_NAIVE);
        hipLaunchKernelGGL(rg_naive, dim3((unsigned)(voxels / 256)), dim3(256), 0, st, d_labels, d_values, n, count, table, counters);
    }
    if (count) {
        ProfScope p(ctx, VP_K_MD_SPLIT);
        hipLaunchKernelGGL(rg_finish, dim3((count + 255u) / 256u), dim3(256), 0, st, table, count, d_values ? 1 : 0, counters);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(ctx->rg.host, counters, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    ctx->rg.stats[0] = ctx->rg.host[kCntVoxels];
    ctx->rg.stats[1] = ctx->rg.host[kCntLabels];
    ctx->rg.stats[2] = ctx->rg.host[kCntIgnored];
    ctx->rg.stats[3] = ctx->rg.host[kCntContact] / 2;
    if (h_stats) std::copy(ctx->rg.stats, ctx->rg.stats + 4, h_stats);
    ctx->rg.n = n;
    ctx->rg.count = count;
    return 0;
}

}  // namespace vp
