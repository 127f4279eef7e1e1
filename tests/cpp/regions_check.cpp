// VOX::AnalyzeRegions checked from C++, a stand-alone program.
//   regions_check <labels.u32> <values.u32 | -> <n> <count> <types> <prefix>
//       types: letters of s(equential) o(penmp) n(aive) t(iled); every requested type writes <prefix>.<tag>.table.u64 (count x 26 values) for
//       the Python test to compare and prints "<tag> <voxels> <labels> <ignored> <interfaces> <sum of the Euler numbers>".  labels and values
//       are raw files of n^3 uint32; "-" = no value field.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/regions.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) std::exit(3);
    std::fclose(f);
}

static bool slurp(const char* path, void* data, size_t bytes)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(data, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

template <Types TY>
static void run(const char* tag, const HostGrid<uint32_t>& labels, uint32_t count, const HostGrid<uint32_t>* values, const std::string& prefix)
{
    VOX::RegionTotals t{};
    const std::vector<VOX::RegionStats> table = VOX::AnalyzeRegions<TY>(labels, count, values, &t);
    long long chi = 0;
    for (const VOX::RegionStats& r : table) chi += r.EulerNumber();
    dump(prefix + "." + tag + ".table.u64", table.data(), table.size() * sizeof(VOX::RegionStats));
    std::printf("%s %llu %llu %llu %llu %lld\n", tag, static_cast<unsigned long long>(t.voxels), static_cast<unsigned long long>(t.labels),
                static_cast<unsigned long long>(t.ignored), static_cast<unsigned long long>(t.interfaces), chi);
}

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const size_t n = std::strtoul(argv[3], nullptr, 10);
    const uint32_t count = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
    const std::string types = argv[5], prefix = argv[6];
    HostGrid<uint32_t> labels(n, 0u), values(n, 0u);
    const bool field = std::strcmp(argv[2], "-") != 0;
    if (!slurp(argv[1], labels.View().Data(), n * n * n * 4)) return 2;
    if (field && !slurp(argv[2], values.View().Data(), n * n * n * 4)) return 2;
    const HostGrid<uint32_t>* v = field ? &values : nullptr;
    if (types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", labels, count, v, prefix);
    if (types.find('o') != std::string::npos) run<Types::OPENMP>("omp", labels, count, v, prefix);
    if (types.find('n') != std::string::npos) run<Types::NAIVE>("naive", labels, count, v, prefix);
    if (types.find('t') != std::string::npos) run<Types::TILED>("tiled", labels, count, v, prefix);
    return 0;
}
