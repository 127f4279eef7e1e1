// grid_to_mesh.h -- voxel grid -> OBJ-ready meshes for the CLI's -e exports
// (/root/reference/vplib/src/mesh/grid_to_mesh.h:15-22,133-157; apps/cli/main.cpp:118-124,192-197,220-230).
//   VoxelsGridToMeshCompressed  cube faces with shared vertices (white): the reference's mesh -- every face of every set
//                               voxel once, interior faces included, its vertex order, winding and normal indices
//                               (grid_to_mesh.h:25-92; pinned face by face by tests/test_export.py)
//   VoxelsGridToSurfaceMesh     (this build's addition, `vpcli --surface-only`) only the faces between a set voxel and an unset /
//                               outside neighbour: the visible surface without the interior quads
//   VoxelsGridToMesh            one 8-vertex cube per set voxel with a finite sdf, coloured by SDFToRGB(sqrt(sdf), diag)
//   VoxelsGridToPointCloud      one vertex at the centre of every set voxel, same colouring
//   VoxelsGridToSurfaceNets     (this build's addition, `vpcli --surface-nets ITERS`) the surface-nets mesh (Gibson 1998; include/vphip.h,
//                               vp_surfnets_*): one vertex per boundary cell, one quad (two triangles) per exposed voxel face, closed, with
//                               `iterations` (0 .. 64) relaxation steps that take the stairs out while every vertex stays in its cell.
//                               World vertices are origin + (p * voxel size) of the lattice positions p.  SurfaceNetsLattice gives the
//                               lattice form itself: records, positions and quads as vp_surfnets writes them.  The host variant is a
//                               straight scan over the cells in index order; the device variant (n % 32 == 0, n <= 1024) produces the
//                               same bytes
// Never on the timed path (benchmark mode disables -e, main.cpp:57).  The *Device variants (used by the CLI for -t 1 / -t 2)
// leave the O(n^3) walk over the grid to the GPU (vp_extract, include/vphip.h) and write byte-identical files.
#ifndef VPLIB_GRID_TO_MESH_H
#define VPLIB_GRID_TO_MESH_H

#include <algorithm>
#include <cmath>
#include <tuple>
#include <vector>

#include "grid/grid.h"
#include "grid/voxels_grid.h"
#include "mesh/mesh.h"

// grid_to_mesh.h:15-22: blue (near) -> red (far), cube-root ramp
inline std::tuple<float, float, float> SDFToRGB(float v, float max)
{
    float t = std::max(0.0f, std::min(v, max)) / max;
    t = std::cbrt(t);
    return {t, 0.0f, 1.0f - t};
}

template <VGType T> bool VoxelsGridToMeshCompressed(const VoxelsGrid<T>& grid, Mesh& mesh);
template <VGType T> bool VoxelsGridToMesh(const VoxelsGrid<T>& grid, const Grid<float>& sdf, Mesh& mesh);
template <VGType T> bool VoxelsGridToPointCloud(const VoxelsGrid<T>& grid, const Grid<float>& sdf, Mesh& mesh);
template <VGType T> bool VoxelsGridToSurfaceMesh(const VoxelsGrid<T>& grid, Mesh& mesh);
template <VGType T> bool VoxelsGridToMeshCompressedDevice(const VoxelsGrid<T>& grid, Mesh& mesh);
template <VGType T> bool VoxelsGridToSurfaceMeshDevice(const VoxelsGrid<T>& grid, Mesh& mesh);
template <VGType T> bool VoxelsGridToMeshDevice(const VoxelsGrid<T>& grid, const Grid<float>& sdf, Mesh& mesh);
template <VGType T> bool VoxelsGridToPointCloudDevice(const VoxelsGrid<T>& grid, const Grid<float>& sdf, Mesh& mesh);

// the lattice form of the surface-nets mesh: V records (cell index | corner mask << 40), 3 V lattice coordinates, 4 Q vertex indices
struct SurfaceNets {
    std::vector<uint64_t> Cells;
    std::vector<float> Xyz;
    std::vector<uint32_t> Quads;
};
template <VGType T> void SurfaceNetsLattice(const VoxelsGrid<T>& grid, uint32_t iterations, SurfaceNets& out);
template <VGType T> void SurfaceNetsLatticeDevice(const VoxelsGrid<T>& grid, uint32_t iterations, SurfaceNets& out);
template <VGType T> bool VoxelsGridToSurfaceNets(const VoxelsGrid<T>& grid, uint32_t iterations, Mesh& mesh);
template <VGType T> bool VoxelsGridToSurfaceNetsDevice(const VoxelsGrid<T>& grid, uint32_t iterations, Mesh& mesh);
// host scan, second half: the quads (by owner cell, then axis) from the vertex-index volume of the (n+1)^3 cells, then `iterations` relaxation
// steps on out.Xyz; out.Cells and out.Xyz hold the records and the starting positions
void SurfaceNetsFinishHost(int64_t n, uint32_t iterations, const std::vector<uint32_t>& index, SurfaceNets& out);

// Iso-surface nets (include/vphip.h, vp_isonets*): the surface-nets mesh of the inside set {h >= +0} of a float field, h = g - iso, with the
// vertices at the field's edge crossings and normals from its gradient.  `field` holds n^3 values at the voxel centres, x fastest.
//   IsoTransform::LINEAR          g = v
//   IsoTransform::SIGNED_SQUARE   g = copysign(sqrt(|v|), v): every sdf of this library (JFA::Compute, JFA::ComputeExact, VOX::MeshDistance)
// IsoSurfaceNetsLattice is the host restatement -- a straight scan over the cells, any n; the Device form goes through vp_isonets_host
// (n % 32 == 0, n <= 1024; algo = VP_ALGO_NAIVE or VP_ALGO_TILED) and produces the same bytes.  IsoSurfaceNets emits the world mesh:
// vertices origin + (p * voxel size), triangles (a, b, c) and (a, c, d) per quad, one normal per vertex (faces "f a//a" in the OBJ).
enum class IsoTransform : int { LINEAR = 0, SIGNED_SQUARE = 1 };
struct IsoNets : SurfaceNets {
    std::vector<float> Normals;       // 3 V, of the unrelaxed cells; zero where the cell has a corner outside the grid
};
struct IsoFrame { float OriginX = 0.0f, OriginY = 0.0f, OriginZ = 0.0f, VoxelSize = 1.0f; };
void IsoSurfaceNetsLattice(const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, IsoNets& out);
void IsoSurfaceNetsLatticeDevice(const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, int algo, IsoNets& out);
bool IsoSurfaceNets(const Grid<float>& field, const IsoFrame& frame, IsoTransform transform, float iso, uint32_t iterations, Mesh& mesh);
bool IsoSurfaceNetsDevice(const Grid<float>& field, const IsoFrame& frame, IsoTransform transform, float iso, uint32_t iterations, int algo,
                          Mesh& mesh);

#endif
