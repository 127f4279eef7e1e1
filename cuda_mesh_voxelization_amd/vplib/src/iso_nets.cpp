// iso_nets.cpp -- see grid_to_mesh.h.  Surface nets of a float field at an iso level (include/vphip.h, vp_isonets*; no reference
// counterpart): the topology of the surface nets on the inside set {h >= +0}, vertices at the field's edge crossings, normals from its
// gradient.  The host variant is a straight scan over the (n+1)^3 cells in index order -- the contract restated, nothing shared with the
// kernels; it is what -t 0 / -t 3 export and what the device is compared with, bit for bit.  The device variant gets records, lattice
// positions, normals and quads from vp_isonets_host.  Both hand them to one emitter.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "debug_utils.h"
#include "mesh/grid_to_mesh.h"
#include "vp_runtime.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// +0 .. +inf; -0, negatives and every NaN are outside
bool Inside(float h)
{
    uint32_t bits;
    std::memcpy(&bits, &h, sizeof bits);
    return bits <= 0x7F800000u;
}

void HostLattice(const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, IsoNets& out)
{
    const int64_t n = static_cast<int64_t>(field.SizeX());
    const int64_t n1 = n + 1;
    auto value = [&](int64_t x, int64_t y, int64_t z) {
        if (x < 0 || y < 0 || z < 0 || x >= n || y >= n || z >= n) return std::numeric_limits<float>::quiet_NaN();
        const float v = field(static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(z));
        const float g = transform == IsoTransform::SIGNED_SQUARE ? std::copysign(std::sqrt(std::fabs(v)), v) : v;
        return g - iso;
    };
    out.Cells.clear(); out.Xyz.clear(); out.Quads.clear(); out.Normals.clear();
    std::vector<uint32_t> index(static_cast<size_t>(n1 * n1 * n1), kNone);
    for (int64_t cz = -1; cz < n; ++cz)
        for (int64_t cy = -1; cy < n; ++cy)
            for (int64_t cx = -1; cx < n; ++cx) {
                float h[8];
                unsigned mask = 0;
                for (int c = 0; c < 8; ++c) {
                    h[c] = value(cx + (c & 1), cy + ((c >> 1) & 1), cz + (c >> 2));
                    if (Inside(h[c])) mask |= 1u << c;
                }
                if (mask == 0u || mask == 255u) continue;
                const uint64_t cell = static_cast<uint64_t>((cx + 1) + n1 * ((cy + 1) + n1 * (cz + 1)));
                index[cell] = static_cast<uint32_t>(out.Cells.size());
                out.Cells.push_back(cell | (static_cast<uint64_t>(mask) << 40));
                // the crossing edges: axis x, y, z; per axis the lower corners with that axis bit clear, ascending
                float acc[3] = {0.0f, 0.0f, 0.0f};
                int m = 0;
                for (int axis = 0; axis < 3; ++axis)
                    for (int lower = 0; lower < 8; ++lower) {
                        if ((lower >> axis) & 1) continue;
                        const int upper = lower | (1 << axis);
                        if (((mask >> lower) & 1u) == ((mask >> upper) & 1u)) continue;
                        float t = h[lower] / (h[lower] - h[upper]);
                        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
                        ++m;
                        for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (a == axis ? t : static_cast<float>((lower >> a) & 1));
                    }
                const int64_t c3[3] = {cx, cy, cz};
                for (int a = 0; a < 3; ++a) {
                    const float q = acc[a] / static_cast<float>(m);
                    out.Xyz.push_back((static_cast<float>(c3[a]) + 0.5f) + q);
                }
                const float gx = ((h[1] - h[0]) + (h[3] - h[2])) + ((h[5] - h[4]) + (h[7] - h[6]));
                const float gy = ((h[2] - h[0]) + (h[3] - h[1])) + ((h[6] - h[4]) + (h[7] - h[5]));
                const float gz = ((h[4] - h[0]) + (h[5] - h[1])) + ((h[6] - h[2]) + (h[7] - h[3]));
                const float l2 = (gx * gx + gy * gy) + gz * gz;
                if (!(l2 > 0.0f) || std::isinf(l2)) {
                    out.Normals.insert(out.Normals.end(), 3, 0.0f);
                } else {
                    const float l = std::sqrt(l2);
                    out.Normals.push_back((-gx) / l); out.Normals.push_back((-gy) / l); out.Normals.push_back((-gz) / l);
                }
            }
    SurfaceNetsFinishHost(n, iterations, index, out);
}

void DeviceLattice(const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, int algo, IsoNets& out)
{
    cpuAssert(vplib::Multi() == nullptr, "Iso-surface nets run on one device (no -g > 1)\n");
    vp_ctx* ctx = vplib::Context();
    vp_frame f{};
    f.n = static_cast<uint32_t>(field.SizeX()); f.voxel_size = 1.0f;            // lattice coordinates: the frame's origin and voxel size are not applied
    f.z0 = 0; f.z1 = f.n;
    uint64_t nv = 0, nq = 0;
    const int tr = static_cast<int>(transform);
    gpuAssert(vp_isonets_host(ctx, &f, field.Data(), tr, iso, iterations, algo, nullptr, nullptr, nullptr, nullptr, 0, 0, &nv, &nq));
    out.Cells.assign(nv, 0); out.Xyz.assign(nv * 3, 0.0f); out.Normals.assign(nv * 3, 0.0f); out.Quads.assign(nq * 4, 0u);
    if (nv) gpuAssert(vp_isonets_host(ctx, &f, field.Data(), tr, iso, iterations, algo, out.Cells.data(), out.Xyz.data(), out.Normals.data(),
                                      out.Quads.data(), nv, nq, &nv, &nq));
}

// lattice mesh -> world mesh: vertices origin + (p * voxel size) in float, the way the other exporters map lattice points; each quad
// (a, b, c, d) becomes (a, b, c) and (a, c, d); one normal per vertex, so a face names the normals by its vertex indices
void Emit(const IsoFrame& fr, const IsoNets& sn, Mesh& mesh)
{
    mesh.Clear();
    const size_t V = sn.Cells.size();
    mesh.Coords.reserve(V);
    mesh.Normals.reserve(V);
    for (size_t i = 0; i < V; ++i) {
        mesh.Coords.emplace_back(fr.OriginX + (sn.Xyz[3 * i] * fr.VoxelSize), fr.OriginY + (sn.Xyz[3 * i + 1] * fr.VoxelSize),
                                 fr.OriginZ + (sn.Xyz[3 * i + 2] * fr.VoxelSize));
        mesh.Normals.emplace_back(sn.Normals[3 * i], sn.Normals[3 * i + 1], sn.Normals[3 * i + 2]);
    }
    mesh.FacesCoords.reserve(sn.Quads.size() / 4 * 6);
    for (size_t q = 0; q < sn.Quads.size() / 4; ++q) {
        const uint32_t* v = &sn.Quads[4 * q];
        mesh.FacesCoords.insert(mesh.FacesCoords.end(), {v[0], v[1], v[2], v[0], v[2], v[3]});
    }
    mesh.FacesNormals = mesh.FacesCoords;
    mesh.Colors.assign(mesh.VerticesSize(), Color(1.0f, 1.0f, 1.0f, 1.0f));
}

void Check(const Grid<float>& field, float iso, uint32_t iterations)
{
    cpuAssert(field.SizeX() == field.SizeY() && field.SizeX() == field.SizeZ(), "Iso-surface nets: the field must be a cube\n");
    cpuAssert(std::isfinite(iso), "Iso-surface nets: the iso level must be finite\n");
    cpuAssert(iterations <= 64, "Iso-surface nets: 0 .. 64 relaxation steps\n");
}

}  // namespace

void IsoSurfaceNetsLattice(const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, IsoNets& out)
{
    Check(field, iso, iterations);
    HostLattice(field, transform, iso, iterations, out);
}

void IsoSurfaceNetsLatticeDevice(const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, int algo, IsoNets& out)
{
    Check(field, iso, iterations);
    DeviceLattice(field, transform, iso, iterations, algo, out);
}

bool IsoSurfaceNets(const Grid<float>& field, const IsoFrame& frame, IsoTransform transform, float iso, uint32_t iterations, Mesh& mesh)
{
    IsoNets sn;
    IsoSurfaceNetsLattice(field, transform, iso, iterations, sn);
    Emit(frame, sn, mesh);
    return true;
}

bool IsoSurfaceNetsDevice(const Grid<float>& field, const IsoFrame& frame, IsoTransform transform, float iso, uint32_t iterations, int algo,
                          Mesh& mesh)
{
    IsoNets sn;
    IsoSurfaceNetsLatticeDevice(field, transform, iso, iterations, algo, sn);
    Emit(frame, sn, mesh);
    return true;
}
