// geodesic.h -- VOX::GeodesicDistance: the length of the shortest path that stays inside a mask, from a set of seed voxels to every voxel
// of the mask (include/vphip.h, vp_geodesic).  No reference counterpart.
//
// A step goes from a voxel of the mask to one of its neighbours in the mask and costs w1, w2 or w3 when it changes 1, 2 or 3 coordinates:
// GEODESIC_6 (1, -, -) face steps only, GEODESIC_26 (1, 1, 1), GEODESIC_CHAMFER (3, 4, 5; divide by 3 for voxels).  A diagonal step needs
// no other voxel to be set.  Outside the grid counts as not in the mask; seed voxels outside the mask are ignored.  `dist` gets one uint32
// per voxel, x fastest: 0 at the seeds, GEODESIC_NONE where no path arrives and outside the mask; sums saturate at 0xFFFFFFFE.
//   SEQUENTIAL / OPENMP   host restatement (geodesic.cpp): Dial's algorithm -- a ring of buckets, one per distance level, settled in
//                         ascending order -- on a volume padded by one layer; it does not call the library.  OPENMP runs the conversions
//                         around it in parallel, the queue itself is sequential.  Any grid side
//   NAIVE / TILED         vp_geodesic_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bytes and the same statistics.
#ifndef VPLIB_GEODESIC_H
#define VPLIB_GEODESIC_H

#include <cstdint>

#include "vox/vox.h"

namespace VOX {

enum GeodesicMetric : int { GEODESIC_6 = 0, GEODESIC_26 = 1, GEODESIC_CHAMFER = 2 };    // VP_GEO_6, VP_GEO_26, VP_GEO_CHAMFER

constexpr uint32_t GEODESIC_NONE = 0xFFFFFFFFu;                                          // VP_GEO_NONE

// seeds used (those inside the mask), voxels reached, the largest finite distance and the lowest linear index x + n (y + n z) that attains
// it; all zero when no seed lies in the mask
struct GeodesicStats { uint64_t seeds, reached, maxDist, maxIndex; };

namespace detail {
GeodesicStats GeodesicHost(bool parallel, const uint32_t* mask, const uint32_t* seeds, size_t n, int metric, uint32_t* dist, uint32_t* reach);
GeodesicStats GeodesicDevice(int algo, const char* label, const uint32_t* mask, const uint32_t* seeds, size_t n, float voxelSize,
                             const float origin[3], int metric, uint32_t* dist, uint32_t* reach);
}  // namespace detail

// `dist` is replaced by the distance map (side and frame of `mask`); `reach`, when given, by the grid of the voxels with a finite distance
// -- the components of the mask that touch a seed.  `seeds` has the side of `mask`.
template <Types type, VGType T>
GeodesicStats GeodesicDistance(const HostVoxelsGrid<T>& mask, const HostVoxelsGrid<T>& seeds, GeodesicMetric metric, HostGrid<uint32_t>& dist,
                               HostVoxelsGrid<T>* reach = nullptr)
{
    const auto& v = mask.View();
    const size_t n = v.VoxelsPerSide();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    if (dist.View().SizeX() != n || dist.View().SizeY() != n || dist.View().SizeZ() != n) dist = HostGrid<uint32_t>(n, 0u);
    uint32_t* rw = nullptr;
    if (reach) {
        *reach = HostVoxelsGrid<T>(n, v.VoxelSize());
        reach->View().SetOrigin(origin[0], origin[1], origin[2]);
        rw = reinterpret_cast<uint32_t*>(reach->View().Data());
    }
    const uint32_t* mw = reinterpret_cast<const uint32_t*>(v.Data());
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(seeds.View().Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::GeodesicHost(type == Types::OPENMP, mw, sw, n, metric, dist.View().Data(), rw);
    else
        return detail::GeodesicDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveGeodesic" : "TiledGeodesic", mw, sw, n,
                                      v.VoxelSize(), origin, metric, dist.View().Data(), rw);
}

}  // namespace VOX

#endif
