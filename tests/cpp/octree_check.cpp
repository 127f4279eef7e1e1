// VOX::BuildOctree / ExpandOctree / ReadOctree through the C++ API, for the Python tests to compare.
//   octree_check build <grid.u32> <n> <word bits: 32 | 64> <types> <prefix>     types: letters of s(equential) o(penmp) n(aive) t(iled)
//       every type builds the tree of the grid (a raw file of n^3 / 8 bytes in the library's layout), checks it, writes <prefix>.<tag>.svo,
//       expands it with the same type into <prefix>.<tag>.grid.u32 and prints "<tag> <M>"
//   octree_check read <file.svo> <type> <prefix> [<points.u32>]
//       reads and validates the file (exit 4 and "rejected: <why>" if it is refused), expands it with the type into <prefix>.grid.u32,
//       prints "n <n> nodes <M>"; with a file of uint32 (x, y, z) triples, Octree::Test of every point goes to <prefix>.test.u8; with the
//       word "all" in its place, Test of every voxel goes to <prefix>.test.u32 as a grid
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/octree.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
    std::fclose(f);
}

static std::vector<char> slurp(const char* path)
{
    std::vector<char> bytes;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    char buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    std::fclose(f);
    return bytes;
}

template <Types TY, typename W>
static void build_one(const char* tag, const HostVoxelsGrid<W>& grid, const std::string& prefix)
{
    const VOX::Octree tree = VOX::BuildOctree<TY>(grid);
    std::string why;
    if (!tree.Validate(&why)) { std::printf("%s invalid: %s\n", tag, why.c_str()); std::exit(5); }
    if (!VOX::WriteOctree(prefix + "." + tag + ".svo", tree)) std::exit(3);
    HostVoxelsGrid<W> back;
    VOX::ExpandOctree<TY>(tree, back);
    dump(prefix + "." + tag + ".grid.u32", back.View().Data(), back.View().StorageSize() * sizeof(W));
    std::printf("%s %zu\n", tag, tree.NodeCount());
}

template <typename W>
static int build_all(const std::vector<char>& bytes, size_t n, const std::string& types, const std::string& prefix)
{
    HostVoxelsGrid<W> grid(n, 0.5f);
    grid.View().SetOrigin(1.0f, -2.0f, 3.0f);
    std::memcpy(grid.View().Data(), bytes.data(), bytes.size());
    if (types.find('s') != std::string::npos) build_one<Types::SEQUENTIAL>("seq", grid, prefix);
    if (types.find('o') != std::string::npos) build_one<Types::OPENMP>("omp", grid, prefix);
    if (types.find('n') != std::string::npos) build_one<Types::NAIVE>("naive", grid, prefix);
    if (types.find('t') != std::string::npos) build_one<Types::TILED>("tiled", grid, prefix);
    return 0;
}

static int read_one(const char* path, char type, const std::string& prefix, const char* points)
{
    VOX::Octree tree;
    std::string why;
    if (!VOX::ReadOctree(path, tree, &why)) { std::printf("rejected: %s\n", why.c_str()); return 4; }
    HostVoxelsGrid<uint32_t> grid;
    if (type == 's') VOX::ExpandOctree<Types::SEQUENTIAL>(tree, grid);
    else if (type == 'n') VOX::ExpandOctree<Types::NAIVE>(tree, grid);
    else if (type == 't') VOX::ExpandOctree<Types::TILED>(tree, grid);
    else return 2;
    dump(prefix + ".grid.u32", grid.View().Data(), grid.View().StorageSize() * 4);
    std::printf("n %u nodes %zu\n", tree.n, tree.NodeCount());
    if (points && std::strcmp(points, "all") == 0) {
        const size_t n = tree.n;
        std::vector<uint32_t> words(n * n * n / 32, 0u);
        for (size_t z = 0; z < n; ++z)
            for (size_t y = 0; y < n; ++y)
                for (size_t x = 0; x < n; ++x)
                    if (tree.Test(static_cast<uint32_t>(x), static_cast<uint32_t>(y), static_cast<uint32_t>(z)))
                        words[(x >> 5) + (n / 32) * (y + n * z)] |= 1u << (x & 31);
        dump(prefix + ".test.u32", words.data(), words.size() * 4);
    } else if (points) {
        const std::vector<char> raw = slurp(points);
        const size_t count = raw.size() / 12;
        std::vector<uint32_t> p(3 * count);
        std::memcpy(p.data(), raw.data(), count * 12);
        std::vector<uint8_t> out(count);
        for (size_t i = 0; i < count; ++i) out[i] = tree.Test(p[3 * i], p[3 * i + 1], p[3 * i + 2]) ? 1 : 0;
        dump(prefix + ".test.u8", out.data(), out.size());
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 7 && std::strcmp(argv[1], "build") == 0) {
        const size_t n = std::strtoul(argv[3], nullptr, 10);
        const int bits = std::atoi(argv[4]);
        const std::vector<char> bytes = slurp(argv[2]);
        if (n == 0 || bytes.size() != n * n * n / 8) return 2;
        if (bits == 32) return build_all<uint32_t>(bytes, n, argv[5], argv[6]);
        if (bits == 64) return build_all<uint64_t>(bytes, n, argv[5], argv[6]);
        return 2;
    }
    if ((argc == 5 || argc == 6) && std::strcmp(argv[1], "read") == 0) return read_one(argv[2], argv[3][0], argv[4], argc == 6 ? argv[5] : nullptr);
    return 2;
}
