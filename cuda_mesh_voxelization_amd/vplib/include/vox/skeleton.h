// skeleton.h -- VOX::Skeletonize: topological thinning of a bit grid to its curve skeleton or its homotopy kernel (include/vphip.h,
// vp_skeleton).  No reference counterpart.
//
// An 8-subfield parallel thinning for (26, 6) connectivity: per iteration the border voxels are taken once, then the subfields
// s = (x & 1) | (y & 1) << 1 | (z & 1) << 2 are examined in ascending order against the current grid; a voxel is deleted iff it is a simple
// point and, in curve mode, not a line end.  Outside the grid counts as empty.  The 26-components of the solid and the 6-components of
// its complement are those of the input.
//   SEQUENTIAL / OPENMP   host restatement (skeleton.cpp): the plain sequential form on a padded byte volume with the flood-fill simple();
//                         it does not call the library.  OPENMP examines the candidates of a subfield in parallel (no two of them are
//                         neighbours).  Any grid side
//   NAIVE / TILED         vp_skeleton_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bits and the same statistics.
#ifndef VPLIB_SKELETON_H
#define VPLIB_SKELETON_H

#include <cstdint>

#include "vox/vox.h"

namespace VOX {

enum SkeletonMode : int { SKELETON_KERNEL = 0, SKELETON_CURVE = 1 };                 // VP_SKEL_KERNEL, VP_SKEL_CURVE

struct SkeletonStats { uint64_t voxels, iterations, deleted; };                     // voxels left, iterations run (the empty last one included), voxels deleted

namespace detail {
SkeletonStats SkeletonHost(bool parallel, const uint32_t* words, const uint32_t* anchor, size_t n, int mode, uint32_t maxIters, uint32_t* out);
SkeletonStats SkeletonDevice(int algo, const char* label, const uint32_t* words, const uint32_t* anchor, size_t n, float voxelSize,
                             const float origin[3], int mode, uint32_t maxIters, uint32_t* out);
}  // namespace detail

// `skeleton` is replaced by the thinned grid (it keeps the frame of `grid`; it may not be `grid` itself).  maxIters = 0: until an iteration
// deletes nothing; k > 0: the state after k iterations, a partial homotopic erosion.  `anchor` (optional, same side): voxels that are
// never deleted.
template <Types type, VGType T>
SkeletonStats Skeletonize(const HostVoxelsGrid<T>& grid, HostVoxelsGrid<T>& skeleton, SkeletonMode mode = SKELETON_CURVE, uint32_t maxIters = 0,
                          const HostVoxelsGrid<T>* anchor = nullptr)
{
    const auto& v = grid.View();
    const size_t n = v.VoxelsPerSide();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    skeleton = HostVoxelsGrid<T>(n, v.VoxelSize());
    skeleton.View().SetOrigin(origin[0], origin[1], origin[2]);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    const uint32_t* aw = anchor ? reinterpret_cast<const uint32_t*>(anchor->View().Data()) : nullptr;
    uint32_t* out = reinterpret_cast<uint32_t*>(skeleton.View().Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::SkeletonHost(type == Types::OPENMP, words, aw, n, mode, maxIters, out);
    else
        return detail::SkeletonDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveSkeleton" : "TiledSkeleton", words, aw, n,
                                      v.VoxelSize(), origin, mode, maxIters, out);
}

}  // namespace VOX

#endif
