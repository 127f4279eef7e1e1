// VOX::GeodesicDistance checked from C++, a stand-alone program.
//   geodesic_check <mask.u32> <seeds.u32> <n> <metric> <word bits: 32 | 64> <types> <prefix>
//       types: letters of s(equential) o(penmp) n(aive) t(iled); every requested type writes <prefix>.<tag>.geo.u32 (n^3 values) and
//       <prefix>.<tag>.reach.u32 (a grid) for the Python test to compare and prints "<tag> <seeds> <reached> <max> <index>".  The grids are
//       raw files of n^3 / 8 bytes in the library's layout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/geodesic.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
    std::fclose(f);
}

static bool slurp(const char* path, std::vector<char>& bytes)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
    std::fclose(f);
    return ok;
}

template <Types TY, typename W>
static void run(const char* tag, const HostVoxelsGrid<W>& mask, const HostVoxelsGrid<W>& seeds, int metric, const std::string& prefix)
{
    const size_t n = mask.View().VoxelsPerSide();
    HostGrid<uint32_t> dist;
    HostVoxelsGrid<W> reach;
    const VOX::GeodesicStats st = VOX::GeodesicDistance<TY>(mask, seeds, static_cast<VOX::GeodesicMetric>(metric), dist, &reach);
    dump(prefix + "." + tag + ".geo.u32", dist.View().Data(), n * n * n * 4);
    dump(prefix + "." + tag + ".reach.u32", reach.View().Data(), n * n * n / 8);
    std::printf("%s %llu %llu %llu %llu\n", tag, static_cast<unsigned long long>(st.seeds), static_cast<unsigned long long>(st.reached),
                static_cast<unsigned long long>(st.maxDist), static_cast<unsigned long long>(st.maxIndex));
}

template <typename W>
static int all(const std::vector<char>& maskBytes, const std::vector<char>& seedBytes, size_t n, int metric, const std::string& types,
               const std::string& prefix)
{
    HostVoxelsGrid<W> mask(n, 1.0f), seeds(n, 1.0f);
    std::memcpy(mask.View().Data(), maskBytes.data(), maskBytes.size());
    std::memcpy(seeds.View().Data(), seedBytes.data(), seedBytes.size());
    if (types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", mask, seeds, metric, prefix);
    if (types.find('o') != std::string::npos) run<Types::OPENMP>("omp", mask, seeds, metric, prefix);
    if (types.find('n') != std::string::npos) run<Types::NAIVE>("naive", mask, seeds, metric, prefix);
    if (types.find('t') != std::string::npos) run<Types::TILED>("tiled", mask, seeds, metric, prefix);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const size_t n = std::strtoul(argv[3], nullptr, 10);
    const int metric = std::atoi(argv[4]);
    const int bits = std::atoi(argv[5]);
    std::vector<char> mask(n * n * n / 8), seeds(n * n * n / 8);
    if (!slurp(argv[1], mask) || !slurp(argv[2], seeds)) return 2;
    if (bits == 32) return all<uint32_t>(mask, seeds, n, metric, argv[6], argv[7]);
    if (bits == 64) return all<uint64_t>(mask, seeds, n, metric, argv[6], argv[7]);
    return 2;
}
