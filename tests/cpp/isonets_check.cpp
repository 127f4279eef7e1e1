// IsoSurfaceNetsLattice / IsoSurfaceNets on one field file: prints, per variant, V, Q and FNV-1a-64 hashes of the records, the lattice
// positions, the normals, the quads and the world mesh (vertices, triangles, per-vertex normals), and writes the arrays of the host variant
// to <prefix>.cells / .xyz / .normals / .quads / .world for the Python test to compare with its numpy restatement.  With gpu = 1 the device
// variants (both algos) follow: they must print the hashes of the host variant.
//   isonets_check <field.f32> <n> <transform:0|1> <iso> <iterations> <gpu:0|1> <prefix>
// <iso> is the float's bit pattern in hex (no decimal round trip).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <mesh/grid_to_mesh.h>
#include <vphip.h>

static uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
    std::fclose(f);
}

static void run(const char* tag, int algo, const Grid<float>& field, IsoTransform transform, float iso, uint32_t iterations, const std::string& prefix)
{
    const IsoFrame frame{-0.25f, 0.5f, 1.75f, 0.37f / static_cast<float>(field.SizeX())};
    IsoNets sn;
    Mesh mesh;
    if (algo) { IsoSurfaceNetsLatticeDevice(field, transform, iso, iterations, algo, sn); IsoSurfaceNetsDevice(field, frame, transform, iso, iterations, algo, mesh); }
    else      { IsoSurfaceNetsLattice(field, transform, iso, iterations, sn); IsoSurfaceNets(field, frame, transform, iso, iterations, mesh); }
    uint64_t mh = fnv(mesh.Coords.data(), mesh.Coords.size() * sizeof(Position));
    mh = fnv(mesh.FacesCoords.data(), mesh.FacesCoords.size() * 4, mh);
    mh = fnv(mesh.Normals.data(), mesh.Normals.size() * sizeof(Normal), mh);
    mh = fnv(mesh.FacesNormals.data(), mesh.FacesNormals.size() * 4, mh);
    std::printf("%s %zu %zu %016lx %016lx %016lx %016lx %016lx %zu %zu\n", tag, sn.Cells.size(), sn.Quads.size() / 4, fnv(sn.Cells.data(), sn.Cells.size() * 8),
                fnv(sn.Xyz.data(), sn.Xyz.size() * 4), fnv(sn.Normals.data(), sn.Normals.size() * 4), fnv(sn.Quads.data(), sn.Quads.size() * 4), mh,
                mesh.VerticesSize(), mesh.TrianglesSize());
    if (!prefix.empty()) {
        dump(prefix + ".cells", sn.Cells.data(), sn.Cells.size() * 8);
        dump(prefix + ".xyz", sn.Xyz.data(), sn.Xyz.size() * 4);
        dump(prefix + ".normals", sn.Normals.data(), sn.Normals.size() * 4);
        dump(prefix + ".quads", sn.Quads.data(), sn.Quads.size() * 4);
        dump(prefix + ".world", mesh.Coords.data(), mesh.Coords.size() * sizeof(Position));
    }
}

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const size_t n = std::strtoul(argv[2], nullptr, 10);
    const IsoTransform transform = std::atoi(argv[3]) ? IsoTransform::SIGNED_SQUARE : IsoTransform::LINEAR;
    const uint32_t isoBits = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 16));
    float iso;
    std::memcpy(&iso, &isoBits, 4);
    const uint32_t iterations = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
    HostGrid<float> field(n, 0.0f);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(field.View().Data(), 4, n * n * n, f) != n * n * n) return 3;
    std::fclose(f);
    run("host", 0, field.View(), transform, iso, iterations, argv[7]);
    if (std::atoi(argv[6]) != 0) {
        run("tiled", VP_ALGO_TILED, field.View(), transform, iso, iterations, "");
        run("naive", VP_ALGO_NAIVE, field.View(), transform, iso, iterations, "");
    }
    return 0;
}
