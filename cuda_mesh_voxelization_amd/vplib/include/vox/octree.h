// octree.h -- VOX::BuildOctree / VOX::ExpandOctree: the sparse voxel octree of a bit grid and back, its point query, its structural check
// and its file (include/vphip.h, vp_octree*).  No reference counterpart.
//
// The tree covers the cube of side P = NextPow2(n), L = log2 P levels; a node is stored for the root and for every mixed cell of the
// levels 1 .. L - 1, breadth-first and in ascending Morton code within a level.  A record is two uint32: valid | full << 8 over the eight
// children (c = x + 2 y + 4 z) and the index of the first stored child (0: none).
//   SEQUENTIAL / OPENMP   host restatement (octree.cpp): a pyramid of state bytes over the words, then the records level by level; it does
//                         not call the library.  OPENMP works in parallel over runs of cells.  n % 32 == 0, 32 <= n <= 1024
//   NAIVE / TILED         vp_octree_host / vp_octree_expand_host with VP_ALGO_NAIVE / VP_ALGO_TILED
// Every variant produces the same bytes.
//
// File `.svo`, little-endian: the 8-byte magic "VPSVO1\0\0"; uint32 n, P, L, M; float voxel_size, origin[3]; uint32 level_offset[11],
// full_leaves[11]; then M records of 8 bytes.  ReadOctree validates before it returns: nothing from a file reaches a device unchecked.
#ifndef VPLIB_OCTREE_H
#define VPLIB_OCTREE_H

#include <cstdint>
#include <string>
#include <vector>

#include "vox/vox.h"

namespace VOX {

struct Octree {
    uint32_t n = 0, P = 0, L = 0;                                  // grid side, tree side, levels
    float voxelSize = 1.0f;
    float origin[3] = {0.0f, 0.0f, 0.0f};
    std::vector<uint32_t> nodes;                                   // two words per node
    uint32_t levelOffset[11] = {}, fullLeaves[11] = {};

    size_t NodeCount() const { return nodes.size() / 2; }
    size_t Bytes() const { return nodes.size() * sizeof(uint32_t); }
    // the voxel (x, y, z) of the grid: a descent from the root; coordinates outside the grid are unset
    bool Test(uint32_t x, uint32_t y, uint32_t z) const;
    // the structural check of vp_octree_validate_host, restated, plus the two summaries against the records; `why` receives the reason
    bool Validate(std::string* why = nullptr) const;
};

namespace detail {
void OctreeHost(bool parallel, const uint32_t* words, size_t n, Octree& tree);
void OctreeDevice(int algo, const char* label, const uint32_t* words, size_t n, float voxelSize, const float origin[3], Octree& tree);
void OctreeExpandHost(const Octree& tree, uint32_t* words);
void OctreeExpandDevice(int algo, const char* label, const Octree& tree, uint32_t* words);
}  // namespace detail

template <Types type, VGType T>
Octree BuildOctree(const HostVoxelsGrid<T>& grid)
{
    const auto& v = grid.View();
    const float origin[3] = {v.OriginX(), v.OriginY(), v.OriginZ()};
    const uint32_t* words = reinterpret_cast<const uint32_t*>(v.Data());
    Octree tree;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::OctreeHost(type == Types::OPENMP, words, v.VoxelsPerSide(), tree);
    else
        detail::OctreeDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveOctree" : "TiledOctree", words, v.VoxelsPerSide(),
                             v.VoxelSize(), origin, tree);
    tree.voxelSize = v.VoxelSize();
    for (int a = 0; a < 3; ++a) tree.origin[a] = origin[a];
    return tree;
}

// `grid` is replaced by the grid of side tree.n with the frame the tree carries.  The tree must be valid (Validate()).
template <Types type, VGType T>
void ExpandOctree(const Octree& tree, HostVoxelsGrid<T>& grid)
{
    grid = HostVoxelsGrid<T>(tree.n, tree.voxelSize);
    grid.View().SetOrigin(tree.origin[0], tree.origin[1], tree.origin[2]);
    uint32_t* words = reinterpret_cast<uint32_t*>(grid.View().Data());
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        detail::OctreeExpandHost(tree, words);
    else
        detail::OctreeExpandDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveOctreeExpand" : "TiledOctreeExpand", tree, words);
}

bool WriteOctree(const std::string& path, const Octree& tree);
// false (and `why`) for a file that cannot be read, is not an .svo or does not hold a well-formed tree; `tree` is then left empty
bool ReadOctree(const std::string& path, Octree& tree, std::string* why = nullptr);

}  // namespace VOX

#endif
