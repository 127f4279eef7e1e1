// VOX::LocalThickness through the C++ API: every requested type writes T2 and the thin grid as raw files <prefix>.<tag>.t2.u32 / .thin.u32
// for the Python test to compare, and prints "<tag> <thin count>".  The grid comes from a raw file of n^3 / 8 bytes in the library's layout.
//   thickness_check <grid.u32> <n> <rmax> <thin2> <word bits: 32 | 64> <types> <prefix>       types: letters of s(equential) o(penmp) n(aive) t(iled)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/vox.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
    std::fclose(f);
}

template <Types TY, typename W>
static void run(const char* tag, const HostVoxelsGrid<W>& grid, uint32_t rmax, uint32_t thin2, const std::string& prefix)
{
    const size_t n = grid.View().VoxelsPerSide();
    HostGrid<uint32_t> t2;
    HostVoxelsGrid<W> thin;
    const uint64_t count = VOX::LocalThickness<TY>(grid, rmax, t2, thin2, &thin);
    dump(prefix + "." + tag + ".t2.u32", t2.View().Data(), n * n * n * 4);
    dump(prefix + "." + tag + ".thin.u32", thin.View().Data(), n * n * n / 8);
    std::printf("%s %llu\n", tag, static_cast<unsigned long long>(count));
}

template <typename W>
static int all(const std::vector<char>& bytes, size_t n, uint32_t rmax, uint32_t thin2, const std::string& types, const std::string& prefix)
{
    HostVoxelsGrid<W> grid(n, 1.0f);
    std::memcpy(grid.View().Data(), bytes.data(), bytes.size());
    if (types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", grid, rmax, thin2, prefix);
    if (types.find('o') != std::string::npos) run<Types::OPENMP>("omp", grid, rmax, thin2, prefix);
    if (types.find('n') != std::string::npos) run<Types::NAIVE>("naive", grid, rmax, thin2, prefix);
    if (types.find('t') != std::string::npos) run<Types::TILED>("tiled", grid, rmax, thin2, prefix);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const size_t n = std::strtoul(argv[2], nullptr, 10);
    const uint32_t rmax = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10)), thin2 = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
    const int bits = std::atoi(argv[5]);
    std::vector<char> bytes(n * n * n / 8);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 2;
    std::fclose(f);
    if (bits == 32) return all<uint32_t>(bytes, n, rmax, thin2, argv[6], argv[7]);
    if (bits == 64) return all<uint64_t>(bytes, n, rmax, thin2, argv[6], argv[7]);
    return 2;
}
