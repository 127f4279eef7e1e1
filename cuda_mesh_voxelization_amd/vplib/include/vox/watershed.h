// watershed.h -- VOX::Watershed: marker-controlled watershed of a mask over a priority field, and the geodesic influence zones of the
// markers when there is none (include/vphip.h, vp_watershed).  No reference counterpart.
//
// `markers` holds one uint32 per voxel, x fastest (0 = no marker, labels 1 .. WATERSHED_LABEL_MAX; markers outside the mask are ignored),
// `priority` one uint32 per voxel or nullptr (zones: one level that holds the whole mask; quantum and order are then ignored).  The levels
// priority / quantum present in the mask are flooded in `order`; inside a level a voxel takes the label of its minimum key (hops, level of
// the source in flood order, label) over the paths from the voxels labelled before the level.  `labels` gets the label volume, `cut` the
// grid of the labelled voxels that no neighbour with a larger label touches: the parts, separated by a one-voxel, one-sided cut.
//   SEQUENTIAL / OPENMP   host restatement (watershed.cpp): a hierarchical queue -- one FIFO of sources per level -- and breadth-first
//                         layers that carry the explicit 64-bit key, on a volume padded by one layer; it does not call the library.
//                         OPENMP runs the conversions around it in parallel, the queue itself is sequential.  Any grid side
//   NAIVE / TILED         vp_watershed_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bytes and the same statistics.
#ifndef VPLIB_WATERSHED_H
#define VPLIB_WATERSHED_H

#include <cstdint>

#include "vox/vox.h"

namespace VOX {

enum WatershedOrder : int { WATERSHED_ASCENDING = 0, WATERSHED_DESCENDING = 1 };        // VP_WS_ASCENDING, VP_WS_DESCENDING

constexpr uint32_t WATERSHED_LABEL_MAX = 0xFFFFFu;                                        // VP_WS_LABEL_MAX
constexpr uint32_t WATERSHED_MAX_SPAN = 16384u;                                           // VP_WS_MAX_SPAN

// marker voxels used (those inside the mask), voxels labelled, distinct levels present in the mask (1 in zones mode, 0 for an empty mask),
// voxels cut = labelled - |cut|
struct WatershedStats { uint64_t markers, labelled, levels, cutVoxels; };

namespace detail {
// the host form refuses what the library refuses (a label above the bound, a level span of WATERSHED_MAX_SPAN or more, quantum 0, an unknown
// order or connectivity) with cpuAssert
WatershedStats WatershedHost(bool parallel, const uint32_t* mask, const uint32_t* markers, const uint32_t* priority, size_t n, int order,
                             uint32_t quantum, int connectivity, uint32_t* labels, uint32_t* cut);
WatershedStats WatershedDevice(int algo, const char* label, const uint32_t* mask, const uint32_t* markers, const uint32_t* priority, size_t n,
                               float voxelSize, const float origin[3], int order, uint32_t quantum, int connectivity, uint32_t* labels, uint32_t* cut);
}  // namespace detail

// `labels` is replaced by the label volume (side of `mask`); `cut`, when given, by the cut grid (frame of `mask`).  `markers` and
// `priority` (may be nullptr) have the side of `mask`.  connectivity: 6 or 26.
template <Types type, VGType T>
WatershedStats Watershed(const HostVoxelsGrid<T>& mask, const HostGrid<uint32_t>& markers, const HostGrid<uint32_t>* priority, WatershedOrder order,
                         uint32_t quantum, int connectivity, HostGrid<uint32_t>& labels, HostVoxelsGrid<T>* cut = nullptr)
{
    const auto& v = mask.View();
    const size_t n = v.VoxelsPerSide();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    if (labels.View().SizeX() != n || labels.View().SizeY() != n || labels.View().SizeZ() != n) labels = HostGrid<uint32_t>(n, 0u);
    uint32_t* cw = nullptr;
    if (cut) {
        *cut = HostVoxelsGrid<T>(n, v.VoxelSize());
        cut->View().SetOrigin(origin[0], origin[1], origin[2]);
        cw = reinterpret_cast<uint32_t*>(cut->View().Data());
    }
    const uint32_t* mw = reinterpret_cast<const uint32_t*>(v.Data());
    const uint32_t* lw = markers.View().Data();
    const uint32_t* pw = priority ? priority->View().Data() : nullptr;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::WatershedHost(type == Types::OPENMP, mw, lw, pw, n, order, quantum, connectivity, labels.View().Data(), cw);
    else
        return detail::WatershedDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveWatershed" : "TiledWatershed", mw, lw, pw, n,
                                       v.VoxelSize(), origin, order, quantum, connectivity, labels.View().Data(), cw);
}

}  // namespace VOX

#endif
