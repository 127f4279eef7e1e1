// reconstruct.h -- VOX::Reconstruct and VOX::Extrema: grayscale geodesic reconstruction of a marker field under a mask field, and the
// h-maxima / h-minima and extended extrema of a value field that it gives (include/vphip.h, vp_reconstruct / vp_extrema; DESIGN.md section
// 25).  No reference counterpart.
//
// Fields hold one uint32 per voxel, x fastest; the domain is a grid (nullptr: every voxel), outside the grid counts as not in it.  By
// dilation the marker is raised under the mask along paths inside the domain, R(p) = the maximum over paths q .. p of min(min(F, G)(q),
// min of G along the path); by erosion the same on the complemented values.  Off the domain the result reads 0 / 0xFFFFFFFF; a work value
// of 0 inside the domain (G = 0 for dilation, G = 0xFFFFFFFF for erosion) is a wall.  Neighbours under connectivity 6 or 26; a diagonal step
// needs no other voxel.
//   SEQUENTIAL / OPENMP   host restatement (reconstruct.cpp): a priority queue -- the voxels are settled from the largest work value
//                         down, each one final when it is taken -- on a volume padded by one layer; it does not call the library.  OPENMP
//                         runs the conversions around it in parallel, the queue itself is sequential.  Any grid side
//   NAIVE / TILED         vp_reconstruct_host / vp_extrema_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bytes and the same statistics.
#ifndef VPLIB_RECONSTRUCT_H
#define VPLIB_RECONSTRUCT_H

#include <cstdint>

#include "vox/vox.h"

namespace VOX {

enum ReconstructMode : int { RECONSTRUCT_DILATION = 0, RECONSTRUCT_EROSION = 1 };       // VP_REC_DILATION, VP_REC_EROSION
enum ExtremaKind : int { EXTREMA_MAXIMA = 0, EXTREMA_MINIMA = 1 };                        // VP_EXT_MAXIMA, VP_EXT_MINIMA
enum ExtremaScale : int { EXTREMA_LINEAR = 0, EXTREMA_SQRT16 = 1 };                       // VP_EXT_LINEAR, VP_EXT_SQRT16

// voxels of the domain, those whose value differs from min(F, G) (erosion: max), the sum of the field over the domain, its largest value
// (erosion: the smallest; 0 for an empty domain)
struct ReconstructStats { uint64_t domain, changed, sum, top; };
// voxels of the domain, voxels of the extended extrema, the largest value of the flattened field over the domain (minima: the smallest),
// voxels of the domain where the flattened field differs from the scaled one
struct ExtremaStats { uint64_t domain, extrema, top, flattened; };

// floor(sqrt(256 v)) in exact integers: EXTREMA_SQRT16 of one value
uint32_t Sqrt16(uint32_t v);

namespace detail {
ReconstructStats ReconstructHost(bool parallel, const uint32_t* domain, const uint32_t* marker, const uint32_t* mask, size_t n, int mode,
                                 int connectivity, uint32_t* field);
ReconstructStats ReconstructDevice(int algo, const char* label, const uint32_t* domain, const uint32_t* marker, const uint32_t* mask, size_t n,
                                   float voxelSize, const float origin[3], int mode, int connectivity, uint32_t* field);
ExtremaStats ExtremaHost(bool parallel, const uint32_t* domain, const uint32_t* values, size_t n, int kind, int scale, uint32_t h, int connectivity,
                         uint32_t* scaled, uint32_t* flat, uint32_t* extrema);
ExtremaStats ExtremaDevice(int algo, const char* label, const uint32_t* domain, const uint32_t* values, size_t n, float voxelSize,
                           const float origin[3], int kind, int scale, uint32_t h, int connectivity, uint32_t* scaled, uint32_t* flat, uint32_t* extrema);
}  // namespace detail

// `field` is replaced by the reconstruction (side of `mask`); `marker` has the side of `mask`, `domain` (may be nullptr) too.
template <Types type, VGType T>
ReconstructStats Reconstruct(const HostVoxelsGrid<T>* domain, const HostGrid<uint32_t>& marker, const HostGrid<uint32_t>& mask, ReconstructMode mode,
                             int connectivity, HostGrid<uint32_t>& field)
{
    const size_t n = mask.View().SizeX();
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float origin[3] = {domain ? domain->View().OriginX() : 0.0f, domain ? domain->View().OriginY() : 0.0f, domain ? domain->View().OriginZ() : 0.0f};
    if (field.View().SizeX() != n || field.View().SizeY() != n || field.View().SizeZ() != n) field = HostGrid<uint32_t>(n, 0u);
    const uint32_t* dw = domain ? reinterpret_cast<const uint32_t*>(domain->View().Data()) : nullptr;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::ReconstructHost(type == Types::OPENMP, dw, marker.View().Data(), mask.View().Data(), n, mode, connectivity, field.View().Data());
    else
        return detail::ReconstructDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveReconstruct" : "TiledReconstruct", dw,
                                         marker.View().Data(), mask.View().Data(), n, domain ? domain->View().VoxelSize() : 1.0f,
                                         domain ? origin : zero, mode, connectivity, field.View().Data());
}

// `scaled` and `flat` are replaced by V and H (side of `values`), `extrema` by the grid of the extended extrema in the frame of `frame`,
// which is also the domain unless everyVoxel is set.
template <Types type, VGType T>
ExtremaStats Extrema(const HostVoxelsGrid<T>& frame, bool everyVoxel, const HostGrid<uint32_t>& values, ExtremaKind kind, ExtremaScale scale, uint32_t h,
                     int connectivity, HostGrid<uint32_t>& scaled, HostGrid<uint32_t>& flat, HostVoxelsGrid<T>& extrema)
{
    const auto& v = frame.View();
    const size_t n = v.VoxelsPerSide();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    for (HostGrid<uint32_t>* g : {&scaled, &flat})
        if (g->View().SizeX() != n || g->View().SizeY() != n || g->View().SizeZ() != n) *g = HostGrid<uint32_t>(n, 0u);
    extrema = HostVoxelsGrid<T>(n, v.VoxelSize());
    extrema.View().SetOrigin(origin[0], origin[1], origin[2]);
    const uint32_t* dw = everyVoxel ? nullptr : reinterpret_cast<const uint32_t*>(v.Data());
    uint32_t* ew = reinterpret_cast<uint32_t*>(extrema.View().Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::ExtremaHost(type == Types::OPENMP, dw, values.View().Data(), n, kind, scale, h, connectivity, scaled.View().Data(),
                                   flat.View().Data(), ew);
    else
        return detail::ExtremaDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveExtrema" : "TiledExtrema", dw, values.View().Data(), n,
                                     v.VoxelSize(), origin, kind, scale, h, connectivity, scaled.View().Data(), flat.View().Data(), ew);
}

}  // namespace VOX

#endif
