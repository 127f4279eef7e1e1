// SurfaceNetsLattice / VoxelsGridToSurfaceNets on T = uint32_t and T = uint64_t grids that hold the words of one grid file: prints, per
// variant, V, Q and FNV-1a-64 hashes of the records, the lattice positions, the quads and the world mesh (vertices, triangles, face
// normals), and writes the lattice arrays of the uint32_t host variant to <prefix>.cells / .xyz / .quads for the Python test to compare
// with its numpy restatement.  With gpu = 1 the device variants follow: they must print the hashes of the host variants.
//   surfnets_check <grid.u32> <n> <iterations> <gpu:0|1> <prefix>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <mesh/grid_to_mesh.h>

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

template <typename T>
static void run(const char* tag, bool device, const std::vector<uint32_t>& words, size_t n, uint32_t iterations, const std::string& prefix)
{
    HostVoxelsGrid<T> g(n, 0.37f / static_cast<float>(n));
    g.View().SetOrigin(-0.25f, 0.5f, 1.75f);
    std::memcpy(g.View().Data(), words.data(), words.size() * 4);
    SurfaceNets sn;
    Mesh mesh;
    if (device) { SurfaceNetsLatticeDevice(g.View(), iterations, sn); VoxelsGridToSurfaceNetsDevice(g.View(), iterations, mesh); }
    else        { SurfaceNetsLattice(g.View(), iterations, sn); VoxelsGridToSurfaceNets(g.View(), iterations, mesh); }
    uint64_t mh = fnv(mesh.Coords.data(), mesh.Coords.size() * sizeof(Position));
    mh = fnv(mesh.FacesCoords.data(), mesh.FacesCoords.size() * 4, mh);
    mh = fnv(mesh.FacesNormals.data(), mesh.FacesNormals.size() * 4, mh);
    std::printf("%s %zu %zu %016lx %016lx %016lx %016lx %zu %zu\n", tag, sn.Cells.size(), sn.Quads.size() / 4, fnv(sn.Cells.data(), sn.Cells.size() * 8),
                fnv(sn.Xyz.data(), sn.Xyz.size() * 4), fnv(sn.Quads.data(), sn.Quads.size() * 4), mh, mesh.VerticesSize(), mesh.TrianglesSize());
    if (!prefix.empty()) {
        dump(prefix + ".cells", sn.Cells.data(), sn.Cells.size() * 8);
        dump(prefix + ".xyz", sn.Xyz.data(), sn.Xyz.size() * 4);
        dump(prefix + ".quads", sn.Quads.data(), sn.Quads.size() * 4);
        dump(prefix + ".world", mesh.Coords.data(), mesh.Coords.size() * sizeof(Position));
    }
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const size_t n = std::strtoul(argv[2], nullptr, 10);
    const uint32_t iterations = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
    std::vector<uint32_t> words(n * n * n / 32);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(words.data(), 4, words.size(), f) != words.size()) return 3;
    std::fclose(f);
    run<uint32_t>("seq32", false, words, n, iterations, argv[5]);
    run<uint64_t>("seq64", false, words, n, iterations, "");
    if (std::atoi(argv[4]) != 0) {
        run<uint32_t>("dev32", true, words, n, iterations, "");
        run<uint64_t>("dev64", true, words, n, iterations, "");
    }
    return 0;
}
