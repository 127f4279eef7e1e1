// vox.h -- VOX::Compute, the voxelizer entry points of the reference
// (/root/reference/vplib/src/vox/vox.h:22-32,107-111).
//   Compute<Types::SEQUENTIAL | OPENMP>(grid, mesh)  CPU path, XOR-accumulates into `grid`
//                                                    (vox/sequential.cpp:6-63; the CLI runs SEQUENTIAL for -t 3 too)
//   Compute<Types::NAIVE>(grid, mesh)                GPU, one thread per triangle   (vox/naive.cu:86-122)
//   Compute<Types::TILED>(blockSize, grid, mesh)     GPU, tile-binned hybrid        (vox/tiled.cu:488-576)
// GPU variants replace the grid contents (as the reference's do, tiled.cu:572-575) and keep its
// origin / voxel size.  All variants produce the sequential path's bitmask.
#ifndef VPLIB_VOX_H
#define VPLIB_VOX_H

#include <cstddef>

#include "grid/voxels_grid.h"
#include "mesh/mesh.h"
#include "proc_utils.h"
#include "vphip.h"

namespace VOX {

inline float CalculateEdgeFunctionZY(const Position& V0, const Position& V1, float y, float z)
{ return ((z - V0.Z) * (V1.Y - V0.Y)) - ((y - V0.Y) * (V1.Z - V0.Z)); }

inline Normal CalculateNormalZY(const Position& V0, const Position& V1)
{ return Position(0, V1.Z - V0.Z, -(V1.Y - V0.Y)); }

inline Normal CalculateFaceNormal(const Position& V0, const Position& V1, const Position& V2)
{ return Vec3<float>::Cross(V1 - V0, V2 - V1); }

namespace detail {
// grid words viewed as uint32 (see voxels_grid.h on why this is layout-neutral)
void Sequential(uint32_t* words, size_t n, float voxelSize, const float origin[3], const Mesh& mesh);
void Device(int algo, const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3], const Mesh& mesh);
// conservative surface voxelization (cvox.cpp): host restatement (ORs into `words`; parallel over z when `parallel`) and the GPU marshalling
void ConservativeHost(bool parallel, uint32_t* words, size_t n, float voxelSize, const float origin[3], const Mesh& mesh);
void ConservativeDevice(int algo, const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3], const Mesh& mesh);
// interior fill (fill.cpp): host breadth-first flood from the boundary, and the GPU marshalling; both fill `words` in place
void FillHost(uint32_t* words, size_t n);
void FillDevice(const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3]);
// ball morphology (morph.cpp): host restatement by separable capped squared distances, and the GPU marshalling; both work in place
void MorphHost(bool parallel, uint32_t* words, size_t n, int op, uint32_t radius);
void MorphDevice(int algo, const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3], int op, uint32_t radius);
// exact distance transform (edt.cpp): host restatement by row sweeps and lower envelopes of parabolas, and the GPU marshalling; the
// morphology works in place
void EdtHost(bool parallel, const uint32_t* words, size_t n, int seeds, uint32_t* dist);
void EdtDevice(int algo, const char* label, const uint32_t* words, size_t n, float voxelSize, const float origin[3], int seeds, uint32_t* dist);
void MorphExactHost(bool parallel, uint32_t* words, size_t n, int op, uint32_t radius);
void MorphExactDevice(int algo, const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3], int op, uint32_t radius);
// mesh distance (meshdist.cpp): host restatement by plain loops over the triangles and their band boxes, and the GPU marshalling; `sign`
// (grid words) and `nearest` may be null
void MeshDistanceHost(bool parallel, const uint32_t* sign, size_t n, float voxelSize, const float origin[3], const Mesh& mesh, uint32_t band,
                      float* dist2, uint32_t* nearest);
void MeshDistanceDevice(int algo, const char* label, const uint32_t* sign, size_t n, float voxelSize, const float origin[3], const Mesh& mesh,
                        uint32_t band, float* dist2, uint32_t* nearest);
// generalized winding number (winding.cpp): host restatement (pyramid by loops, one recursive walk per brick, one voxel at a time) and the
// GPU marshalling; `w` (the field, n^3 floats) may be null
void WindingHost(bool parallel, uint32_t* words, size_t n, float voxelSize, const float origin[3], const Mesh& mesh, float beta, float level,
                 float* w);
void WindingDevice(int algo, const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3], const Mesh& mesh, float beta,
                   float level, float* w);
// local thickness (thickness.cpp): host restatement (the definition by loops, one target plane at a time) and the GPU marshalling; `t2`
// (n^3 values) is always written, `thin` (grid words) may be null; both return the number of thin voxels
uint64_t ThicknessHost(bool parallel, const uint32_t* words, size_t n, uint32_t rmax, uint32_t thin2, uint32_t* t2, uint32_t* thin);
uint64_t ThicknessDevice(int algo, const char* label, const uint32_t* words, size_t n, float voxelSize, const float origin[3], uint32_t rmax,
                         uint32_t thin2, uint32_t* t2, uint32_t* thin);
// connected components (components.cpp): host restatement by a scan in index order with an explicit-stack flood per component, and the
// GPU marshalling; the filters work in place
struct ComponentStats { uint32_t count; uint64_t kept; };      // K components found, voxels kept
uint32_t LabelHost(bool parallel, const uint32_t* words, size_t n, uint32_t* labels, int conn);
ComponentStats FilterHost(bool parallel, uint32_t* words, size_t n, int mode, uint32_t param, int conn);
uint32_t LabelDevice(int algo, const char* label, const uint32_t* words, size_t n, float voxelSize, const float origin[3], uint32_t* labels, int conn);
ComponentStats FilterDevice(int algo, const char* label, uint32_t* words, size_t n, float voxelSize, const float origin[3], int mode,
                            uint32_t param, int conn);
}  // namespace detail

template <Types type, VGType T>
void Compute(HostVoxelsGrid<T>& grid, const Mesh& mesh)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::Sequential(words, v.VoxelsPerSide(), v.VoxelSize(), origin, mesh);
    else if constexpr (type == Types::NAIVE)
        detail::Device(VP_ALGO_NAIVE, "NaiveVox", words, v.VoxelsPerSide(), v.VoxelSize(), origin, mesh);
    else
        detail::Device(VP_ALGO_TILED, "TiledVox", words, v.VoxelsPerSide(), v.VoxelSize(), origin, mesh);
}

// blockSize is the reference's -b knob (threads per tile workgroup, tiled.cu:557-566); the HIP tile
// kernel has one fixed wave64-shaped workgroup, so the value is accepted and ignored.
template <Types type, VGType T>
void Compute(const size_t /*blockSize*/, HostVoxelsGrid<T>& grid, const Mesh& mesh)
{
    Compute<type, T>(grid, mesh);
}

// ComputeConservative: the SURFACE grid of any mesh, open or closed -- voxel set iff its closed box overlaps a closed triangle (the
// 26-separating test of Schwarz & Seidel 2010; the float32 predicate of include/vphip.h, vp_voxelize_conservative).  No reference
// counterpart: the reference promises surface grids but has only the solid rule above.
//   SEQUENTIAL / OPENMP   host restatement, ORs into `grid` (OPENMP: parallel over z planes)
//   NAIVE / TILED         vp_voxelize_conservative_host: replace the grid contents, like the GPU Compute variants
// Every variant produces the same bits.
template <Types type, VGType T>
void ComputeConservative(HostVoxelsGrid<T>& grid, const Mesh& mesh)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::ConservativeHost(type == Types::OPENMP, words, v.VoxelsPerSide(), v.VoxelSize(), origin, mesh);
    else if constexpr (type == Types::NAIVE)
        detail::ConservativeDevice(VP_ALGO_NAIVE, "NaiveConservativeVox", words, v.VoxelsPerSide(), v.VoxelSize(), origin, mesh);
    else
        detail::ConservativeDevice(VP_ALGO_TILED, "TiledConservativeVox", words, v.VoxelsPerSide(), v.VoxelSize(), origin, mesh);
}

// blockSize: as for Compute, accepted and ignored
template <Types type, VGType T>
void ComputeConservative(const size_t /*blockSize*/, HostVoxelsGrid<T>& grid, const Mesh& mesh)
{
    ComputeConservative<type, T>(grid, mesh);
}

// FillInterior: the SOLID of a grid -- every empty voxel that no 6-connected path of empty voxels joins to the grid boundary is set
// (include/vphip.h, vp_fill_interior; scipy.ndimage.binary_fill_holes).  Run on a ComputeConservative grid it gives the solid of a mesh
// whose holes are smaller than a voxel, or of a soup that covers a closed surface.  No reference counterpart.
//   SEQUENTIAL / OPENMP   host flood: an explicit-stack search from every empty boundary voxel over a visited bit grid (one thread)
//   NAIVE / TILED         vp_fill_interior_host (one GPU path, like CSG)
// Every variant produces the same bits.
template <Types type, VGType T>
void FillInterior(HostVoxelsGrid<T>& grid)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::FillHost(words, v.VoxelsPerSide());
    else
        detail::FillDevice(type == Types::NAIVE ? "NaiveFill" : "TiledFill", words, v.VoxelsPerSide(), v.VoxelSize(), origin);
}

// Morph: ball morphology of a grid, in place (include/vphip.h, vp_morph).  B_r = {d in Z^3 : |d|^2 <= r^2}, r = 0 .. 32 (0 = identity).
//   DILATE  set iff some set voxel lies within B_r (outside the grid reads as empty)   scipy binary_dilation(border_value=0)
//   ERODE   NOT dilate(NOT grid) (outside the grid reads as set)                       scipy binary_erosion(border_value=1)
//   OPEN = dilate(erode), CLOSE = erode(dilate): idempotent, open a subset and close a superset of the grid.
// To repair a shell with holes up to about 2 r voxels wide: Morph(DILATE, r), FillInterior, Morph(ERODE, r) -- not CLOSE then fill,
// which leaks (the erosion inside CLOSE re-opens the plug before the fill sees it).  No reference counterpart.
//   SEQUENTIAL / OPENMP   host restatement in another formulation: the exact capped squared distance in three separable integer passes
//                         (x, then y, then z), then <= r^2; OPENMP runs the planes in parallel
//   NAIVE / TILED         vp_morph_host with VP_ALGO_NAIVE / VP_ALGO_TILED
// Every variant produces the same bits.
enum class MorphOp : int { DILATE = 0, ERODE = 1, OPEN = 2, CLOSE = 3 };     // = VP_MORPH_*

template <Types type, VGType T>
void Morph(HostVoxelsGrid<T>& grid, MorphOp op, uint32_t radius)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::MorphHost(type == Types::OPENMP, words, v.VoxelsPerSide(), static_cast<int>(op), radius);
    else
        detail::MorphDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveMorph" : "TiledMorph", words, v.VoxelsPerSide(),
                            v.VoxelSize(), origin, static_cast<int>(op), radius);
}

// DistanceTransform / MorphExact: the exact Euclidean distance transform of a grid and ball morphology through it (include/vphip.h, vp_edt /
// vp_edt_morph).  No reference counterpart.
//   DistanceTransform  dist(x, y, z) = the smallest squared distance, in voxels, to a seed voxel -- EdtSeeds::SET (the set voxels), UNSET (the
//                      unset voxels) or BORDER (the JFA's seeds: set voxels with an unset or outside 26-neighbour); voxels outside the grid are
//                      never seeds; VP_EDT_NONE everywhere if there is no seed.  `dist` is resized to the grid.
//   MorphExact         Morph for any radius 0 .. 65535, in place: dilate = D_SET <= r^2, erode = D_UNSET > r^2, open and close composed.
//   SEQUENTIAL / OPENMP   host restatement in another formulation (row sweeps, then lower envelopes of parabolas); any grid side
//   NAIVE / TILED         vp_edt_host / vp_edt_morph_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same values and bits.
enum class EdtSeeds : int { SET = 0, UNSET = 1, BORDER = 2 };     // = VP_EDT_SEEDS_*

template <Types type, VGType T>
void DistanceTransform(const HostVoxelsGrid<T>& grid, HostGrid<uint32_t>& dist, EdtSeeds seeds = EdtSeeds::SET)
{
    const auto& v = grid.View();
    const size_t n = v.VoxelsPerSide();
    if (dist.View().SizeX() != n || dist.View().SizeY() != n || dist.View().SizeZ() != n) dist = HostGrid<uint32_t>(n, 0u);
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::EdtHost(type == Types::OPENMP, words, n, static_cast<int>(seeds), dist.View().Data());
    else
        detail::EdtDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveEdt" : "TiledEdt", words, n, v.VoxelSize(), origin,
                          static_cast<int>(seeds), dist.View().Data());
}

template <Types type, VGType T>
void MorphExact(HostVoxelsGrid<T>& grid, MorphOp op, uint32_t radius)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::MorphExactHost(type == Types::OPENMP, words, v.VoxelsPerSide(), static_cast<int>(op), radius);
    else
        detail::MorphExactDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveMorphExact" : "TiledMorphExact", words,
                                 v.VoxelsPerSide(), v.VoxelSize(), origin, static_cast<int>(op), radius);
}

// MeshDistance: the narrow-band distance field to the TRIANGLES of `mesh`, sampled at the voxel centres of `grid`'s frame (include/vphip.h,
// vp_mesh_distance): dist2(x, y, z) = min(B2, the squared distance from the centre to the nearest triangle), B = band voxels (1 .. 32),
// positive on the set voxels of `grid` and negative on the unset ones when `withSign` (the grid is then whatever solid the caller made of
// the mesh), +everywhere otherwise; `nearest` (optional) = the index of the nearest face, VP_MESH_NONE outside the band.  Both are resized
// to the grid.  No reference counterpart.
//   SEQUENTIAL / OPENMP   host restatement: plain loops over the triangles and the voxels of their band boxes, the header's float32
//                         expressions (OPENMP: parallel over z planes); any grid side
//   NAIVE / TILED         vp_mesh_distance_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bits.
template <Types type, VGType T>
void MeshDistance(const HostVoxelsGrid<T>& grid, const Mesh& mesh, uint32_t band, HostGrid<float>& dist2, HostGrid<uint32_t>* nearest = nullptr,
                  bool withSign = true)
{
    const auto& v = grid.View();
    const size_t n = v.VoxelsPerSide();
    if (dist2.View().SizeX() != n || dist2.View().SizeY() != n || dist2.View().SizeZ() != n) dist2 = HostGrid<float>(n, 0.0f);
    if (nearest && (nearest->View().SizeX() != n || nearest->View().SizeY() != n || nearest->View().SizeZ() != n)) *nearest = HostGrid<uint32_t>(n, 0u);
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    const uint32_t* words = withSign ? reinterpret_cast<const uint32_t*>(v.Data()) : nullptr;
    uint32_t* near = nearest ? nearest->View().Data() : nullptr;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::MeshDistanceHost(type == Types::OPENMP, words, n, v.VoxelSize(), origin, mesh, band, dist2.View().Data(), near);
    else
        detail::MeshDistanceDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveMeshDistance" : "TiledMeshDistance", words, n,
                                   v.VoxelSize(), origin, mesh, band, dist2.View().Data(), near);
}

// ComputeWinding: the SOLID grid of any mesh -- closed, open, a soup, self-intersecting -- from its generalized winding number (include/vphip.h,
// vp_winding): voxel set iff w(centre) >= level, w = the sum of the signed solid angles of the triangles / 4 pi (1 inside a closed
// outward-oriented mesh, 0 outside, k where k shells overlap: level 0.5 is the union, 1.5 the intersection of two).  The sign is exact at
// the voxel CENTRE, which Compute's column rule is not.  beta = 0: every triangle exactly; 1 .. 64: far nodes of the brick pyramid as one
// dipole each (2 is the usual choice).  Replaces the grid contents; `field` (optional) receives w and is resized to the grid.  No
// reference counterpart.
//   SEQUENTIAL / OPENMP   host restatement (OPENMP: bricks in parallel); any grid side that is a multiple of 8
//   NAIVE / TILED         vp_winding_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bits.
template <Types type, VGType T>
void ComputeWinding(HostVoxelsGrid<T>& grid, const Mesh& mesh, float level = 0.5f, float beta = 2.0f, HostGrid<float>* field = nullptr)
{
    auto& v = grid.View();
    const size_t n = v.VoxelsPerSide();
    if (field && (field->View().SizeX() != n || field->View().SizeY() != n || field->View().SizeZ() != n)) *field = HostGrid<float>(n, 0.0f);
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    float* w = field ? field->View().Data() : nullptr;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::WindingHost(type == Types::OPENMP, words, n, v.VoxelSize(), origin, mesh, beta, level, w);
    else
        detail::WindingDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveWinding" : "TiledWinding", words, n, v.VoxelSize(),
                              origin, mesh, beta, level, w);
}

// LocalThickness: for every set voxel the squared radius T2 of the largest ball that fits inside the solid and contains the voxel, in a band
// of rmax = 1 .. 32 voxels (include/vphip.h, vp_thickness; Hildebrand & Ruegsegger 1997): t2(x, y, z) = max { D(c) : |p - c|^2 < D(c) } with
// D = min(squared distance to the nearest unset voxel, squared distance to the nearest voxel outside the grid, rmax^2); 0 on unset voxels,
// rmax^2 where the part is thicker than 2 rmax.  The thickness in voxels is 2 sqrt(t2).  `thin` (optional; replaced, keeps the frame of
// `grid`) receives the set voxels with t2 < thin2 (0 .. rmax^2); the return value is their number.  `t2` is resized to the grid.  Pore or
// channel width: the same call on the complemented grid (the frame's wall then acts as solid).  No reference counterpart.
//   SEQUENTIAL / OPENMP   host restatement: the definition by loops (OPENMP: target planes in parallel); any grid side
//   NAIVE / TILED         vp_thickness_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same values and bits.
template <Types type, VGType T>
uint64_t LocalThickness(const HostVoxelsGrid<T>& grid, uint32_t rmax, HostGrid<uint32_t>& t2, uint32_t thin2 = 0, HostVoxelsGrid<T>* thin = nullptr)
{
    const auto& v = grid.View();
    const size_t n = v.VoxelsPerSide();
    if (t2.View().SizeX() != n || t2.View().SizeY() != n || t2.View().SizeZ() != n) t2 = HostGrid<uint32_t>(n, 0u);
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    if (thin) {
        *thin = HostVoxelsGrid<T>(n, v.VoxelSize());
        thin->View().SetOrigin(origin[0], origin[1], origin[2]);
    }
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    uint32_t* tw = thin ? reinterpret_cast<uint32_t*>(thin->View().Data()) : nullptr;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::ThicknessHost(type == Types::OPENMP, words, n, rmax, thin2, t2.View().Data(), tw);
    else
        return detail::ThicknessDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveThickness" : "TiledThickness", words, n,
                                       v.VoxelSize(), origin, rmax, thin2, t2.View().Data(), tw);
}

// LabelComponents / FilterComponents: connected components of the set voxels (include/vphip.h, vp_components_*).  conn = 6 (face
// neighbours) or 26 (face, edge and corner neighbours); voxels outside the grid are empty.  No reference counterpart.
//   LabelComponents   labels(x, y, z) = 0 for an empty voxel, else 1 .. K, components numbered in increasing order of their lowest linear
//                     voxel index (scipy.ndimage.label's numbering); `labels` is resized to the grid; returns K
//   FilterComponents  in place: ComponentFilter::KEEP_LARGEST keeps the `param` (1 .. 16) largest components, ties to the lower label;
//                     MIN_VOXELS those of at least `param` voxels; returns {K, voxels kept}
//   SEQUENTIAL / OPENMP   host restatement in another formulation: one scan in index order, an explicit-stack flood per component
//   NAIVE / TILED         vp_components_label_host / vp_components_filter_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same labels and bits.
enum class ComponentFilter : int { KEEP_LARGEST = 0, MIN_VOXELS = 1 };     // = VP_COMP_*
using ComponentStats = detail::ComponentStats;

template <Types type, VGType T>
uint32_t LabelComponents(const HostVoxelsGrid<T>& grid, HostGrid<uint32_t>& labels, int conn = 26)
{
    const auto& v = grid.View();
    const size_t n = v.VoxelsPerSide();
    if (labels.View().SizeX() != n || labels.View().SizeY() != n || labels.View().SizeZ() != n) labels = HostGrid<uint32_t>(n, 0u);
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::LabelHost(type == Types::OPENMP, words, n, labels.View().Data(), conn);
    else
        return detail::LabelDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveComponents" : "TiledComponents", words, n,
                                   v.VoxelSize(), origin, labels.View().Data(), conn);
}

template <Types type, VGType T>
ComponentStats FilterComponents(HostVoxelsGrid<T>& grid, ComponentFilter mode, uint32_t param, int conn = 26)
{
    auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    uint32_t* words = reinterpret_cast<uint32_t*>(v.Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        return detail::FilterHost(type == Types::OPENMP, words, v.VoxelsPerSide(), static_cast<int>(mode), param, conn);
    else
        return detail::FilterDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveComponents" : "TiledComponents", words,
                                    v.VoxelsPerSide(), v.VoxelSize(), origin, static_cast<int>(mode), param, conn);
}

}  // namespace VOX

#endif
