// VOX::ComputeWinding through the C++ API: every requested type writes its field and its grid as raw files <prefix>.<tag>.w.f32 /
// .grid.u32 for the Python test to compare.  The mesh is framed as the CLI frames it unless a frame is given.
//   winding_check <mesh.obj> <n> <beta> <level> <types> <prefix> [<voxel size> <ox> <oy> <oz>]       types: letters of s(equential) o(penmp) n(aive) t(iled)
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static void run(const char* tag, HostVoxelsGrid<uint32_t>& grid, const Mesh& mesh, float level, float beta, const std::string& prefix)
{
    const size_t n = grid.View().VoxelsPerSide();
    HostGrid<float> field;
    VOX::ComputeWinding<TY>(grid, mesh, level, beta, &field);
    dump(prefix + "." + tag + ".w.f32", field.View().Data(), n * n * n * 4);
    dump(prefix + "." + tag + ".grid.u32", grid.View().Data(), n * n * n / 8);
}

int main(int argc, char** argv)
{
    if (argc != 7 && argc != 11) return 2;
    Mesh mesh;
    if (!ImportMesh(argv[1], mesh)) return 2;
    const size_t n = std::strtoul(argv[2], nullptr, 10);
    const float beta = std::strtof(argv[3], nullptr), level = std::strtof(argv[4], nullptr);
    const std::string types = argv[5], prefix = argv[6];
    float vs, o[3];
    if (argc == 11) {
        vs = std::strtof(argv[7], nullptr);
        for (int a = 0; a < 3; ++a) o[a] = std::strtof(argv[8 + a], nullptr);
    } else {
        MinMax bx, by, bz;
        const float side = CalculateBoundingBox(std::span<const Position>(mesh.Coords.data(), mesh.Coords.size()), bx, by, bz);
        vs = side / n; o[0] = bx.first; o[1] = by.first; o[2] = bz.first;
    }
    HostVoxelsGrid<uint32_t> grid(n, vs);
    grid.View().SetOrigin(o[0], o[1], o[2]);
    if (types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", grid, mesh, level, beta, prefix);
    if (types.find('o') != std::string::npos) run<Types::OPENMP>("omp", grid, mesh, level, beta, prefix);
    if (types.find('n') != std::string::npos) run<Types::NAIVE>("naive", grid, mesh, level, beta, prefix);
    if (types.find('t') != std::string::npos) run<Types::TILED>("tiled", grid, mesh, level, beta, prefix);
    return 0;
}
