// VOX::Watershed checked from C++, a stand-alone program.
//   watershed_check <mask.u32> <markers.u32> <priority.u32 | -> <n> <order> <quantum> <connectivity> <word bits: 32 | 64> <types> <prefix>
//       types: letters of s(equential) o(penmp) n(aive) t(iled); every requested type writes <prefix>.<tag>.labels.u32 (n^3 values) and
//       <prefix>.<tag>.cut.u32 (a grid) for the Python test to compare and prints "<tag> <markers> <labelled> <levels> <cut>".  The mask is
//       a raw file of n^3 / 8 bytes in the library's layout, markers and priority raw files of n^3 uint32; "-" = no priority field.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/watershed.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
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

struct Job {
    const HostGrid<uint32_t>* markers;
    const HostGrid<uint32_t>* priority;
    int order;
    uint32_t quantum;
    int connectivity;
    std::string prefix;
};

template <Types TY, typename W>
static void run(const char* tag, const HostVoxelsGrid<W>& mask, const Job& job)
{
    const size_t n = mask.View().VoxelsPerSide();
    HostGrid<uint32_t> labels;
    HostVoxelsGrid<W> cut;
    const VOX::WatershedStats st = VOX::Watershed<TY>(mask, *job.markers, job.priority, static_cast<VOX::WatershedOrder>(job.order), job.quantum,
                                                      job.connectivity, labels, &cut);
    dump(job.prefix + "." + tag + ".labels.u32", labels.View().Data(), n * n * n * 4);
    dump(job.prefix + "." + tag + ".cut.u32", cut.View().Data(), n * n * n / 8);
    std::printf("%s %llu %llu %llu %llu\n", tag, static_cast<unsigned long long>(st.markers), static_cast<unsigned long long>(st.labelled),
                static_cast<unsigned long long>(st.levels), static_cast<unsigned long long>(st.cutVoxels));
}

template <typename W>
static int all(const std::vector<char>& maskBytes, size_t n, const Job& job, const std::string& types)
{
    HostVoxelsGrid<W> mask(n, 1.0f);
    std::memcpy(mask.View().Data(), maskBytes.data(), maskBytes.size());
    if (types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", mask, job);
    if (types.find('o') != std::string::npos) run<Types::OPENMP>("omp", mask, job);
    if (types.find('n') != std::string::npos) run<Types::NAIVE>("naive", mask, job);
    if (types.find('t') != std::string::npos) run<Types::TILED>("tiled", mask, job);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 11) return 2;
    const size_t n = std::strtoul(argv[4], nullptr, 10);
    const int bits = std::atoi(argv[8]);
    std::vector<char> mask(n * n * n / 8);
    HostGrid<uint32_t> markers(n, 0u), priority(n, 0u);
    const bool flood = std::strcmp(argv[3], "-") != 0;
    if (!slurp(argv[1], mask.data(), mask.size()) || !slurp(argv[2], markers.View().Data(), n * n * n * 4)) return 2;
    if (flood && !slurp(argv[3], priority.View().Data(), n * n * n * 4)) return 2;
    const Job job{&markers, flood ? &priority : nullptr, std::atoi(argv[5]), static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10)), std::atoi(argv[7]),
                  argv[10]};
    if (bits == 32) return all<uint32_t>(mask, n, job, argv[9]);
    if (bits == 64) return all<uint64_t>(mask, n, job, argv[9]);
    return 2;
}
