// jfa.h -- JFA::Compute (/root/reference/vplib/src/jfa/jfa.h:19-20,42-43).
// `sdf` must be pre-filled by the caller (the CLI uses -INFINITY, apps/cli/main.cpp:200) and receives
// the signed SQUARED distance: 0 on inside-border voxels, > 0 inside, < 0 outside.
#ifndef VPLIB_JFA_H
#define VPLIB_JFA_H

#include "grid/grid.h"
#include "grid/voxels_grid.h"
#include "mesh/mesh.h"
#include "proc_utils.h"
#include "vphip.h"

namespace JFA {

inline float CalculateDistance(Position p0, Position p1)
{ return ((p1.X - p0.X) * (p1.X - p0.X)) + ((p1.Y - p0.Y) * (p1.Y - p0.Y)) + ((p1.Z - p0.Z) * (p1.Z - p0.Z)); }

namespace detail {
void Host(bool parallel, const uint32_t* words, size_t n, float voxelSize, const float origin[3], float* sdf);
void Device(int algo, const char* label, const uint32_t* words, size_t n, float voxelSize, const float origin[3], float* sdf);
// the exact field (edt.cpp): host restatement and the GPU marshalling
void ExactHost(bool parallel, const uint32_t* words, size_t n, float voxelSize, float* sdf);
void ExactDevice(int algo, const char* label, const uint32_t* words, size_t n, float voxelSize, const float origin[3], float* sdf);
}  // namespace detail

template <Types type, VGType T>
void Compute(HostVoxelsGrid<T>& grid, HostGrid<float>& sdf)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    float* out = sdf.View().Data();
    if constexpr (type == Types::SEQUENTIAL) detail::Host(false, words, v.VoxelsPerSide(), v.VoxelSize(), origin, out);
    else if constexpr (type == Types::OPENMP) detail::Host(true, words, v.VoxelsPerSide(), v.VoxelSize(), origin, out);
    else if constexpr (type == Types::NAIVE) detail::Device(VP_ALGO_NAIVE, "NaiveJFA", words, v.VoxelsPerSide(), v.VoxelSize(), origin, out);
    else detail::Device(VP_ALGO_TILED, "TiledJFA", words, v.VoxelsPerSide(), v.VoxelSize(), origin, out);
}

// ComputeExact: Compute without the error of Jump Flooding (include/vphip.h, vp_edt_sdf).  Same calling convention, same seeds, same sign
// rule and the same zeros; the magnitude is the exact squared distance to the nearest border voxel: (float)D * (voxelSize * voxelSize) with
// D the integer squared voxel distance.  |Compute| >= |ComputeExact| everywhere.  No reference counterpart.
//   SEQUENTIAL / OPENMP   host restatement (x sweeps, then the lower envelope of parabolas along y and z; any grid side)
//   NAIVE / TILED         vp_edt_sdf_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024, one device)
template <Types type, VGType T>
void ComputeExact(HostVoxelsGrid<T>& grid, HostGrid<float>& sdf)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    float* out = sdf.View().Data();
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::ExactHost(type == Types::OPENMP, words, v.VoxelsPerSide(), v.VoxelSize(), out);
    else
        detail::ExactDevice(type == Types::NAIVE ? VP_ALGO_NAIVE : VP_ALGO_TILED, type == Types::NAIVE ? "NaiveExactSDF" : "TiledExactSDF", words,
                            v.VoxelsPerSide(), v.VoxelSize(), origin, out);
}

}  // namespace JFA

#endif
