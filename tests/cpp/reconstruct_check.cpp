// VOX::Reconstruct and VOX::Extrema checked from C++, a stand-alone program.
//   reconstruct_check rec <domain.u32 | -> <marker.u32> <mask.u32> <n> <mode> <connectivity> <word bits: 32 | 64> <types> <prefix>
//   reconstruct_check ext <domain.u32 | -> <values.u32> <n> <kind> <scale> <h> <connectivity> <word bits: 32 | 64> <types> <prefix>
//       types: letters of s(equential) o(penmp) n(aive) t(iled).  rec: every requested type writes <prefix>.<tag>.rec.u32 (n^3 values) and
//       prints "<tag> <domain> <changed> <sum> <top>"; ext: <prefix>.<tag>.scaled.u32, .flat.u32 (n^3 values), .ext.u32 (a grid) and
//       "<tag> <domain> <extrema> <top> <flattened>".  The fields are raw files of n^3 uint32, x fastest; the grids raw files of n^3 / 8
//       bytes in the library's layout; "-" for the domain means every voxel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/reconstruct.h>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) std::exit(3);
    std::fclose(f);
}

static bool slurp(const char* path, void* to, size_t bytes)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(to, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

struct Args {
    bool ext = false, everyVoxel = false;
    size_t n = 0;
    int a = 0, b = 0, conn = 6;                                     // rec: mode, -; ext: kind, scale
    uint32_t h = 0;
    std::string types, prefix;
    HostGrid<uint32_t> first, second;                              // rec: marker, mask; ext: values, -
};

template <Types TY, typename W>
static void run(const char* tag, const Args& g, const HostVoxelsGrid<W>& domain)
{
    const size_t n = g.n, vb = n * n * n * 4;
    const std::string stem = g.prefix + "." + tag;
    if (!g.ext) {
        HostGrid<uint32_t> field;
        const VOX::ReconstructStats st = VOX::Reconstruct<TY>(g.everyVoxel ? nullptr : &domain, g.first, g.second, static_cast<VOX::ReconstructMode>(g.a),
                                                               g.conn, field);
        dump(stem + ".rec.u32", field.View().Data(), vb);
        std::printf("%s %llu %llu %llu %llu\n", tag, static_cast<unsigned long long>(st.domain), static_cast<unsigned long long>(st.changed),
                    static_cast<unsigned long long>(st.sum), static_cast<unsigned long long>(st.top));
    } else {
        HostGrid<uint32_t> scaled, flat;
        HostVoxelsGrid<W> extrema;
        const VOX::ExtremaStats st = VOX::Extrema<TY>(domain, g.everyVoxel, g.first, static_cast<VOX::ExtremaKind>(g.a), static_cast<VOX::ExtremaScale>(g.b),
                                                       g.h, g.conn, scaled, flat, extrema);
        dump(stem + ".scaled.u32", scaled.View().Data(), vb);
        dump(stem + ".flat.u32", flat.View().Data(), vb);
        dump(stem + ".ext.u32", extrema.View().Data(), n * n * n / 8);
        std::printf("%s %llu %llu %llu %llu\n", tag, static_cast<unsigned long long>(st.domain), static_cast<unsigned long long>(st.extrema),
                    static_cast<unsigned long long>(st.top), static_cast<unsigned long long>(st.flattened));
    }
}

template <typename W>
static int all(const Args& g, const char* domainPath)
{
    HostVoxelsGrid<W> domain(g.n, 1.0f);
    if (!g.everyVoxel && !slurp(domainPath, domain.View().Data(), g.n * g.n * g.n / 8)) return 2;
    if (g.types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", g, domain);
    if (g.types.find('o') != std::string::npos) run<Types::OPENMP>("omp", g, domain);
    if (g.types.find('n') != std::string::npos) run<Types::NAIVE>("naive", g, domain);
    if (g.types.find('t') != std::string::npos) run<Types::TILED>("tiled", g, domain);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    Args g;
    g.ext = std::strcmp(argv[1], "ext") == 0;
    if ((!g.ext && std::strcmp(argv[1], "rec") != 0) || argc != (g.ext ? 12 : 11)) return 2;
    g.everyVoxel = std::strcmp(argv[2], "-") == 0;
    int bits = 0;
    if (!g.ext) {
        g.n = std::strtoul(argv[5], nullptr, 10);
        g.a = std::atoi(argv[6]);
        g.conn = std::atoi(argv[7]);
        bits = std::atoi(argv[8]);
    } else {
        g.n = std::strtoul(argv[4], nullptr, 10);
        g.a = std::atoi(argv[5]);
        g.b = std::atoi(argv[6]);
        g.h = static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10));
        g.conn = std::atoi(argv[8]);
        bits = std::atoi(argv[9]);
    }
    g.types = argv[g.ext ? 10 : 9];
    g.prefix = argv[g.ext ? 11 : 10];
    const size_t vb = g.n * g.n * g.n * 4;
    g.first = HostGrid<uint32_t>(g.n, 0u);
    if (!slurp(argv[3], g.first.View().Data(), vb)) return 2;
    if (!g.ext) {
        g.second = HostGrid<uint32_t>(g.n, 0u);
        if (!slurp(argv[4], g.second.View().Data(), vb)) return 2;
    }
    if (bits == 32) return all<uint32_t>(g, argv[2]);
    if (bits == 64) return all<uint64_t>(g, argv[2]);
    return 2;
}
