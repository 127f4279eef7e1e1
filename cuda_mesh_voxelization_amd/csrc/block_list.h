// block_list.h -- the list of active blocks shared by the kernels that run one workgroup per ACTIVE block of a whole grid (skeleton.hip,
// geodesic.hip, watershed.hip): the block shape, the layout of the aux buffer and the one-workgroup compaction of the block flags into the list.
// The kernels that raise the flags stay with their feature; the rule that maps a changed voxel to the neighbour blocks whose halo holds it
// (block_seen_by) is shared by the two that stage a one-voxel halo.
#pragma once

#include "wg_scan.h"

namespace vp {

constexpr uint32_t kBlockY = 16, kBlockZ = 16;                    // a block is one word (32 voxels) x 16 x 16: 256 lanes, one per word / x row
constexpr uint32_t kMaxBlocksPerThread = 128;                     // n = 1024: 32 * 64 * 64 blocks / 1024 threads
// The aux buffer: kAuxHead bytes of the feature's own counters, one flag per block, then the list (8 bytes per block in all)
constexpr size_t kAuxHead = 64;
inline uint32_t block_count(uint32_t n) { return (n / 32) * (n / kBlockY) * (n / kBlockZ); }
inline size_t block_aux_bytes(uint32_t nblocks) { return kAuxHead + (size_t)nblocks * 8; }
inline uint32_t* block_flags(void* aux) { return (uint32_t*)((char*)aux + kAuxHead); }

namespace {   // a kernel of its own in every file that includes this one

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

}  // namespace

}  // namespace vp
