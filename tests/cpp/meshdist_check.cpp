// VOX::MeshDistance through the C++ API: the mesh is framed as the CLI frames it, voxelized by VOX::Compute<SEQUENTIAL> for the sign, and
// every requested type writes its field and its nearest faces as raw files <prefix>.<tag>.dist.f32 / .near.u32 for the Python test to compare.
//   meshdist_check <mesh.obj> <n> <band> <signed:0|1> <gpu:0|1> <prefix>
#include <cstdio>
#include <cstdlib>
#include <span>
#include <string>

#include <bounding_box.h>
#include <mesh/mesh_io.h>
#include <vox/vox.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
    std::fclose(f);
}

template <Types TY>
static void run(const char* tag, const HostVoxelsGrid<uint32_t>& grid, const Mesh& mesh, uint32_t band, bool withSign, const std::string& prefix)
{
    const size_t n = grid.View().VoxelsPerSide();
    HostGrid<float> dist;
    HostGrid<uint32_t> near;
    VOX::MeshDistance<TY>(grid, mesh, band, dist, &near, withSign);
    dump(prefix + "." + tag + ".dist.f32", dist.View().Data(), n * n * n * 4);
    dump(prefix + "." + tag + ".near.u32", near.View().Data(), n * n * n * 4);
}

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    Mesh mesh;
    if (!ImportMesh(argv[1], mesh)) return 2;
    const size_t n = std::strtoul(argv[2], nullptr, 10);
    const uint32_t band = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
    const bool withSign = std::atoi(argv[4]) != 0;
    const std::string prefix = argv[6];
    MinMax bx, by, bz;
    const float side = CalculateBoundingBox(std::span<const Position>(mesh.Coords.data(), mesh.Coords.size()), bx, by, bz);
    HostVoxelsGrid<uint32_t> grid(n, side / n);
    grid.View().SetOrigin(bx.first, by.first, bz.first);
    VOX::Compute<Types::SEQUENTIAL>(grid, mesh);
    run<Types::SEQUENTIAL>("seq", grid, mesh, band, withSign, prefix);
    run<Types::OPENMP>("omp", grid, mesh, band, withSign, prefix);
    if (std::atoi(argv[5]) != 0) {
        run<Types::NAIVE>("naive", grid, mesh, band, withSign, prefix);
        run<Types::TILED>("tiled", grid, mesh, band, withSign, prefix);
    }
    return 0;
}
