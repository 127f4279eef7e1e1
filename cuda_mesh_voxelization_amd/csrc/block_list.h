// block_list.h -- what the kernels that run one workgroup per block of 32 x 16 x 16 voxels of a whole grid share (skeleton.hip, geodesic.hip,
// watershed.hip, regions.hip): the coordinates of a block, the layout of the aux buffer, the list of ACTIVE blocks
// from the block flags with its host step, the rule that maps a changed voxel to the neighbour blocks whose halo holds it and the raising
// of their flags, and the tile of a block with its one-voxel halo.  The sweeps stay with their feature.
#pragma once

#include "vp_internal.h"
#include "wg_scan.h"

namespace vp {

constexpr uint32_t kBlockY = 16, kBlockZ = 16;                    // a block is one word (32 voxels) x 16 x 16: 256 lanes, one per word / x row
constexpr uint32_t kMaxBlocksPerThread = 128;                     // n = 1024: 32 * 64 * 64 blocks / 1024 threads
// The aux buffer: kAuxHead bytes of the feature's own counters, one flag per block, then the list (8 bytes per block in all)
constexpr size_t kAuxHead = 64;
inline uint32_t block_count(uint32_t n) { return (n / 32) * (n / kBlockY) * (n / kBlockZ); }
inline size_t block_aux_bytes(uint32_t nblocks) { return kAuxHead + (size_t)nblocks * 8; }
inline uint32_t* block_flags(void* aux) { return (uint32_t*)((char*)aux + kAuxHead); }
// The tile of a block with its one-voxel halo: kHalo rows per axis of kRowVals values (x - 1 .. x + 32) at a pitch of kRowPitch values; the
// odd pitch keeps the 32 rows that a half-wave reads on distinct banks but for two.  kStaged = 11,016 values.
constexpr uint32_t kHalo = 18, kRowVals = 34, kRowPitch = 35, kStaged = kHalo * kHalo * kRowVals;

namespace {   // a kernel of its own in every file that includes this one

// block b of a grid of side n: its coordinates among the w x nb x nb blocks
struct BlockAt {
    uint32_t bx, by, bz, w, nb;
    __device__ __forceinline__ uint32_t x0() const { return bx * 32u; }                  // x0, y0, z0: the origin voxel
    __device__ __forceinline__ uint32_t y0() const { return by * kBlockY; }
    __device__ __forceinline__ uint32_t z0() const { return bz * kBlockZ; }
    // the word of row (ly, lz) in a bit grid, and voxel x of that row in a volume
    __device__ __forceinline__ size_t word(uint32_t n, uint32_t ly, uint32_t lz) const { return bx + (size_t)w * (y0() + ly + (size_t)n * (z0() + lz)); }
    __device__ __forceinline__ size_t voxel(uint32_t n, uint32_t x, uint32_t ly, uint32_t lz) const { return x0() + x + (size_t)n * (y0() + ly + (size_t)n * (z0() + lz)); }
};

__device__ __forceinline__ BlockAt block_at(uint32_t b, uint32_t n)
{
    const uint32_t w = n / 32, nb = n / kBlockY;
    return BlockAt{b % w, (b / w) % nb, b / (w * nb), w, nb};
}

constexpr uint32_t kFaceBlocks = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);   // of bit dx+1 + 3 (dy+1) + 9 (dz+1)

// The blocks whose staged tile holds one of the voxels `bits` of the row (ly, lz) of a block, bit dx+1 + 3 (dy+1) + 9 (dz+1) per block offset,
// the block itself (bit 13) included: -1 / +1 along an axis needs the voxel on that face.  Face neighbours only where no step is diagonal.
__device__ __forceinline__ uint32_t block_seen_by(uint32_t bits, uint32_t ly, uint32_t lz, bool diagonal)
{
    if (bits == 0u) return 0u;
    const uint32_t xm = (bits & 1u) | 2u | ((bits >> 31) << 2);
    const uint32_t xy = (ly == 0u ? xm : 0u) | (xm << 3) | (ly == kBlockY - 1u ? xm << 6 : 0u);
    const uint32_t see = (lz == 0u ? xy : 0u) | (xy << 9) | (lz == kBlockZ - 1u ? xy << 18 : 0u);
    return diagonal ? see : see & (kFaceBlocks | 1u << 13);
}

// k < 27: raises, with a plain store of 1, the flag of the block at offset k (as above) from `at` if bit k of `bits` is set and the block exists
__device__ __forceinline__ void block_raise(uint32_t* __restrict__ flags, uint32_t bits, BlockAt at, uint32_t k)
{
    const uint32_t nx = at.bx + k % 3u - 1u, ny = at.by + (k / 3u) % 3u - 1u, nz = at.bz + k / 9u - 1u;   // wraps below 0: >= the count
    if (((bits >> k) & 1u) && nx < at.w && ny < at.nb && nz < at.nb) flags[nx + at.w * (ny + at.nb * nz)] = 1u;
}

// column 0 of the lane's row (ly, lz) of a tile: column c = voxel c - 1 of the row
template <typename T> __device__ __forceinline__ T* tile_row(T* tile, uint32_t ly, uint32_t lz) { return tile + ((lz + 1u) * kHalo + ly + 1u) * kRowPitch; }

// 256 lanes stage the tile of block `at`: load(x, y, z, inside, c, ry, rz) gives the value of the voxel (x, y, z), which lies in the grid iff
// `inside` (its coordinates are not to be used otherwise), for column c of row (ry, rz) of the tile.  The caller's barrier publishes the tile.
template <typename T, typename Load>
__device__ __forceinline__ void stage_halo(T* tile, BlockAt at, uint32_t n, Load load)
{
    for (uint32_t k = 0; k < (kStaged + 255u) / 256u; ++k) {
        const uint32_t e = k * 256u + threadIdx.x;
        if (e < kStaged) {
            const uint32_t c = e % kRowVals, r = e / kRowVals, ry = r % kHalo, rz = r / kHalo;
            const uint32_t x = at.x0() + c - 1u, y = at.y0() + ry - 1u, z = at.z0() + rz - 1u;   // wraps below 0: >= n
            tile[r * kRowPitch + c] = load(x, y, z, x < n && y < n && z < n, c, ry, rz);
        }
    }
}

// 256 lanes along x visit the voxels named by lowered[256] (one word per row r = ly + 16 lz of the block): f(r, x, index of the voxel in a
// volume, its offset in the tile)
template <typename F>
__device__ __forceinline__ void store_lowered(const uint32_t* lowered, BlockAt at, uint32_t n, F f)
{
#pragma unroll 4
    for (uint32_t k = 0; k < 32u; ++k) {
        const uint32_t e = k * 256u + threadIdx.x, x = e & 31u, r = e >> 5;
        if ((lowered[r] >> x) & 1u)
            f(r, x, at.voxel(n, x, r & 15u, r >> 4), ((r >> 4) + 1u) * kHalo * kRowPitch + ((r & 15u) + 1u) * kRowPitch + x + 1u);
    }
}

// one lane per voxel i, whole waves: the bits of 64 consecutive voxels of a bit grid are one ballot = two words
__device__ __forceinline__ void store_ballot(uint32_t* __restrict__ grid, size_t i, bool bit)
{
    const unsigned long long hit = __ballot(bit);
    if ((threadIdx.x & 63u) == 0) { grid[i >> 5] = (uint32_t)hit; grid[(i >> 5) + 1] = (uint32_t)(hit >> 32); }
}

// one workgroup: list = the indices of the raised flags in ascending order, *count = their number; the flags are cleared
__global__ void __launch_bounds__(1024)
block_list(uint32_t* __restrict__ flags, uint32_t nblocks, uint32_t* __restrict__ list, uint32_t* __restrict__ count)
{
    __shared__ uint32_t part[1024];
    const uint32_t total = wg_scan_1024<uint32_t, uint32_t>(
        part, nblocks, [&](uint32_t i) { return flags[i] ? 1u : 0u; }, [&](uint32_t i, uint32_t v) { if (flags[i]) list[v] = i; });
    __syncthreads();
    for (uint32_t k = 0; k < kMaxBlocksPerThread; ++k) {
        const uint32_t i = k * 1024u + threadIdx.x;
        if (i < nblocks) flags[i] = 0u;
    }
    if (threadIdx.x == 0) *count = total;
}

// The host step of a round: the list from the flags (booked under md_scan; `first`, if any, launches in front of it under the same
// bracket), then `bytes` from the count word on -- the count and whatever the feature keeps behind it -- come back through `host` in one
// synchronisation.  *active = the count.
template <typename First = void (*)()>
int list_active(vp_ctx* ctx, uint32_t* flags, uint32_t nblocks, uint32_t* list, uint32_t* d_count, volatile uint32_t* host, size_t bytes,
                uint32_t* active, First first = [] {})
{
    {
        ProfScope p(ctx, VP_K_MD_SCAN);
        first();
        hipLaunchKernelGGL(block_list, dim3(1), dim3(1024), 0, ctx->stream, flags, nblocks, list, d_count);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync((void*)host, d_count, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    *active = host[0];
    return 0;
}

}  // namespace

}  // namespace vp
