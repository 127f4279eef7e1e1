// surface_nets.cpp -- see grid_to_mesh.h.  Surface nets of a voxel grid (include/vphip.h, vp_surfnets_*; no reference counterpart): one
// vertex per boundary cell, one quad per exposed voxel face, `iterations` Jacobi relaxation steps inside the cells.
// The host variant is a straight scan over the (n+1)^3 cells in index order with an index volume -- the contract restated without any of
// the device's word tricks; it is what -t 0 / -t 3 export and what the device is compared with, bit for bit.  The device variant gets
// records, lattice positions and quads from vp_surfnets_host.  Both hand them to one emitter.
#include <array>
#include <cstdint>
#include <vector>

#include "debug_utils.h"
#include "mesh/grid_to_mesh.h"
#include "vp_runtime.h"

namespace {

constexpr uint64_t kCellMask = (1ull << 40) - 1;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// the twelve edges of the unit cell: corner pairs, grouped by axis (x, y, z)
constexpr int kEdges[12][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
// corner sets of the faces -x, +x, -y, +y, -z, +z
constexpr unsigned kFaces[6] = {0x55u, 0xAAu, 0x33u, 0xCCu, 0x0Fu, 0xF0u};

template <VGType T>
void HostLattice(const VoxelsGrid<T>& grid, uint32_t iterations, SurfaceNets& out)
{
    const int64_t n = static_cast<int64_t>(grid.VoxelsPerSide());
    const int64_t n1 = n + 1;
    auto set = [&](int64_t x, int64_t y, int64_t z) { return x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n && grid.Voxel(x, y, z); };
    out.Cells.clear(); out.Xyz.clear(); out.Quads.clear();
    std::vector<uint32_t> index(static_cast<size_t>(n1 * n1 * n1), kNone);
    for (int64_t cz = -1; cz < n; ++cz)
        for (int64_t cy = -1; cy < n; ++cy)
            for (int64_t cx = -1; cx < n; ++cx) {
                unsigned mask = 0;
                for (int c = 0; c < 8; ++c)
                    if (set(cx + (c & 1), cy + ((c >> 1) & 1), cz + (c >> 2))) mask |= 1u << c;
                if (mask == 0u || mask == 255u) continue;
                const uint64_t cell = static_cast<uint64_t>((cx + 1) + n1 * ((cy + 1) + n1 * (cz + 1)));
                index[cell] = static_cast<uint32_t>(out.Cells.size());
                out.Cells.push_back(cell | (static_cast<uint64_t>(mask) << 40));
                int m = 0, s[3] = {0, 0, 0};
                for (const auto& e : kEdges) {
                    if (((mask >> e[0]) & 1u) == ((mask >> e[1]) & 1u)) continue;
                    ++m;
                    for (int a = 0; a < 3; ++a) s[a] += ((e[0] >> a) & 1) + ((e[1] >> a) & 1);      // twice the midpoint's coordinate
                }
                const int64_t c3[3] = {cx, cy, cz};
                for (int a = 0; a < 3; ++a)
                    out.Xyz.push_back((static_cast<float>(c3[a]) + 0.5f) + static_cast<float>(s[a]) / static_cast<float>(2 * m));
            }
    SurfaceNetsFinishHost(n, iterations, index, out);
}

template <VGType T>
void DeviceLattice(const VoxelsGrid<T>& grid, uint32_t iterations, SurfaceNets& out)
{
    cpuAssert(vplib::Multi() == nullptr, "Surface nets run on one device (no -g > 1)\n");
    vp_ctx* ctx = vplib::Context();
    vp_frame f{};
    f.n = static_cast<uint32_t>(grid.VoxelsPerSide()); f.voxel_size = grid.VoxelSize();
    f.origin[0] = grid.OriginX(); f.origin[1] = grid.OriginY(); f.origin[2] = grid.OriginZ();
    f.z0 = 0; f.z1 = f.n;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(grid.Data());
    uint64_t nv = 0, nq = 0;
    gpuAssert(vp_surfnets_host(ctx, &f, words, iterations, nullptr, nullptr, nullptr, 0, 0, &nv, &nq));
    out.Cells.assign(nv, 0); out.Xyz.assign(nv * 3, 0.0f); out.Quads.assign(nq * 4, 0u);
    if (nv) gpuAssert(vp_surfnets_host(ctx, &f, words, iterations, out.Cells.data(), out.Xyz.data(), out.Quads.data(), nv, nq, &nv, &nq));
}

// lattice mesh -> world mesh: vertices origin + (p * voxel size) in float, the way the cube-face exporters map lattice points; each quad
// (a, b, c, d) becomes (a, b, c) and (a, c, d).  Faces carry the axis normal of the voxel face they came from (the quads follow the vertex
// records: owner cell by owner cell, axis by axis), so the OBJ stays readable by everything that reads the other exports.
template <VGType T>
void Emit(const VoxelsGrid<T>& grid, const SurfaceNets& sn, Mesh& mesh)
{
    mesh.Clear();
    mesh.Normals = {Normal(0, 0, 1), Normal(0, 1, 0), Normal(1, 0, 0), Normal(0, 0, -1), Normal(0, -1, 0), Normal(-1, 0, 0)};
    static const uint32_t normalIndex[3][2] = {{5, 2}, {4, 1}, {3, 0}};       // [axis][outward = + axis]
    const float vs = grid.VoxelSize();
    mesh.Coords.reserve(sn.Cells.size());
    for (size_t i = 0; i < sn.Cells.size(); ++i)
        mesh.Coords.emplace_back(grid.OriginX() + (sn.Xyz[3 * i] * vs), grid.OriginY() + (sn.Xyz[3 * i + 1] * vs), grid.OriginZ() + (sn.Xyz[3 * i + 2] * vs));
    mesh.FacesCoords.reserve(sn.Quads.size() / 4 * 6);
    mesh.FacesNormals.reserve(sn.Quads.size() / 4 * 6);
    size_t q = 0;
    for (const uint64_t rec : sn.Cells) {
        const unsigned mask = static_cast<unsigned>(rec >> 40);
        for (int axis = 0; axis < 3; ++axis) {
            if ((mask & 1u) == ((mask >> (1 << axis)) & 1u)) continue;
            const uint32_t* v = &sn.Quads[4 * q++];
            mesh.FacesCoords.insert(mesh.FacesCoords.end(), {v[0], v[1], v[2], v[0], v[2], v[3]});
            mesh.FacesNormals.insert(mesh.FacesNormals.end(), 6, normalIndex[axis][mask & 1u]);
        }
    }
    mesh.Colors.assign(mesh.VerticesSize(), Color(1.0f, 1.0f, 1.0f, 1.0f));
}

}  // namespace

// the part of the host scan that knows the inside set only through the records: quads from the index volume, then the relaxation.  Shared
// with the iso-surface nets (iso_nets.cpp), whose records come from a field.
void SurfaceNetsFinishHost(int64_t n, uint32_t iterations, const std::vector<uint32_t>& index, SurfaceNets& out)
{
    const int64_t n1 = n + 1;
    // quads, by owner cell (= vertex order), then axis
    // offsets, in the linear cell index, of the four cells around an owned x-, y- or z-edge, in the contract's order
    const int64_t s1 = n1, s2 = n1 * n1;
    const int64_t around[3][4] = {{-s1 - s2, -s2, 0, -s1}, {-1 - s2, -1, 0, -s2}, {-1 - s1, -s1, 0, -1}};
    for (const uint64_t rec : out.Cells) {
        const int64_t cell = static_cast<int64_t>(rec & kCellMask);
        const unsigned mask = static_cast<unsigned>(rec >> 40);
        for (int axis = 0; axis < 3; ++axis) {
            if ((mask & 1u) == ((mask >> (1 << axis)) & 1u)) continue;      // corner 0 against corner 1, 2, 4
            const bool lower = (mask & 1u) != 0u;                           // the lower voxel is the set one: normal along + axis
            for (int t = 0; t < 4; ++t) out.Quads.push_back(index[static_cast<size_t>(cell + around[axis][lower ? t : 3 - t])]);
        }
    }
    // relaxation
    const size_t V = out.Cells.size();
    std::vector<float> other(iterations ? out.Xyz.size() : 0);
    const int64_t nstep[6] = {-1, 1, -n1, n1, -n1 * n1, n1 * n1};
    for (uint32_t it = 0; it < iterations; ++it) {
        for (size_t i = 0; i < V; ++i) {
            const int64_t cell = static_cast<int64_t>(out.Cells[i] & kCellMask);
            const unsigned mask = static_cast<unsigned>(out.Cells[i] >> 40);
            const int64_t c3[3] = {cell % n1 - 1, (cell / n1) % n1 - 1, cell / (n1 * n1) - 1};
            float acc[3] = {0.0f, 0.0f, 0.0f};
            int deg = 0;
            for (int f = 0; f < 6; ++f) {
                const unsigned m = mask & kFaces[f];
                if (m == 0u || m == kFaces[f]) continue;
                const float* p = &out.Xyz[3 * static_cast<size_t>(index[static_cast<size_t>(cell + nstep[f])])];
                for (int a = 0; a < 3; ++a) acc[a] = deg == 0 ? p[a] : acc[a] + p[a];
                ++deg;
            }
            for (int a = 0; a < 3; ++a) {
                const float q = acc[a] / static_cast<float>(deg);
                const float lo = static_cast<float>(c3[a]) + 0.5625f, hi = static_cast<float>(c3[a]) + 1.4375f;
                other[3 * i + a] = std::min(std::max(q, lo), hi);
            }
        }
        out.Xyz.swap(other);
    }
}

template <VGType T> void SurfaceNetsLattice(const VoxelsGrid<T>& grid, uint32_t iterations, SurfaceNets& out) { HostLattice(grid, iterations, out); }
template <VGType T> void SurfaceNetsLatticeDevice(const VoxelsGrid<T>& grid, uint32_t iterations, SurfaceNets& out) { DeviceLattice(grid, iterations, out); }

template <VGType T> bool VoxelsGridToSurfaceNets(const VoxelsGrid<T>& grid, uint32_t iterations, Mesh& mesh)
{
    cpuAssert(iterations <= 64, "Surface nets: 0 .. 64 relaxation steps\n");
    SurfaceNets sn;
    HostLattice(grid, iterations, sn);
    Emit(grid, sn, mesh);
    return true;
}

template <VGType T> bool VoxelsGridToSurfaceNetsDevice(const VoxelsGrid<T>& grid, uint32_t iterations, Mesh& mesh)
{
    cpuAssert(iterations <= 64, "Surface nets: 0 .. 64 relaxation steps\n");
    SurfaceNets sn;
    DeviceLattice(grid, iterations, sn);
    Emit(grid, sn, mesh);
    return true;
}

#define VP_INSTANTIATE(T)                                                                                  \
    template void SurfaceNetsLattice<T>(const VoxelsGrid<T>&, uint32_t, SurfaceNets&);                     \
    template void SurfaceNetsLatticeDevice<T>(const VoxelsGrid<T>&, uint32_t, SurfaceNets&);               \
    template bool VoxelsGridToSurfaceNets<T>(const VoxelsGrid<T>&, uint32_t, Mesh&);                       \
    template bool VoxelsGridToSurfaceNetsDevice<T>(const VoxelsGrid<T>&, uint32_t, Mesh&);
VP_INSTANTIATE(uint32_t)
VP_INSTANTIATE(uint64_t)
#undef VP_INSTANTIATE
