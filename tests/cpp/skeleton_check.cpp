// The simple-point test and VOX::Skeletonize checked from C++, a stand-alone program.
//   skeleton_check exhaustive
//       every one of the 2^26 neighbourhoods through the plain and the shift form of csrc/skeleton_simple.h: prints
//       "simple <count> mismatches <count> steps <a> <b>" -- the dilations the flood fills needed at most for (a) and (b), one less than the
//       fixed step counts of the shift form -- and fails on a mismatch, a wrong count or a step count the constants do not cover
//   skeleton_check run <grid.u32> <anchor.u32 | -> <n> <mode> <max iters> <word bits: 32 | 64> <types> <prefix>
//       types: letters of s(equential) o(penmp) n(aive) t(iled); every requested type writes <prefix>.<tag>.skel.u32 for the Python test to
//       compare and prints "<tag> <voxels> <iterations> <deleted>".  The grids are raw files of n^3 / 8 bytes in the library's layout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vox/skeleton.h>

#include "../../cuda_mesh_voxelization_amd/csrc/skeleton_simple.h"

static int exhaustive()
{
    unsigned long long simple = 0, mismatches = 0;
    int stepsA = 0, stepsB = 0;
#pragma omp parallel for schedule(static) reduction(+ : simple, mismatches) reduction(max : stepsA, stepsB)
    for (long long c = 0; c < (1ll << 26); ++c) {
        const uint32_t m = vp::sk_mask_of_index(static_cast<uint32_t>(c));
        int a = 0, b = 0;
        const bool plain = vp::sk_simple_plain(m, &a, &b);
        simple += plain;
        mismatches += plain != vp::sk_simple_shift(m);
        // the centre bit is ignored
        mismatches += plain != vp::sk_simple_shift(m | vp::kSkCentre);
        if (a > stepsA) stepsA = a;
        if (b > stepsB) stepsB = b;
    }
    std::printf("simple %llu mismatches %llu steps %d %d\n", simple, mismatches, stepsA, stepsB);
    return (simple == 25985144ull && mismatches == 0 && stepsA + 1 <= vp::kSkStepsA && stepsB + 1 <= vp::kSkStepsB) ? 0 : 1;
}

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
static void run(const char* tag, const HostVoxelsGrid<W>& grid, const HostVoxelsGrid<W>* anchor, int mode, uint32_t iters, const std::string& prefix)
{
    const size_t n = grid.View().VoxelsPerSide();
    HostVoxelsGrid<W> skel;
    const VOX::SkeletonStats st = VOX::Skeletonize<TY>(grid, skel, static_cast<VOX::SkeletonMode>(mode), iters, anchor);
    dump(prefix + "." + tag + ".skel.u32", skel.View().Data(), n * n * n / 8);
    std::printf("%s %llu %llu %llu\n", tag, static_cast<unsigned long long>(st.voxels), static_cast<unsigned long long>(st.iterations),
                static_cast<unsigned long long>(st.deleted));
}

template <typename W>
static int all(const std::vector<char>& bytes, const std::vector<char>* anchorBytes, size_t n, int mode, uint32_t iters, const std::string& types,
               const std::string& prefix)
{
    HostVoxelsGrid<W> grid(n, 1.0f), anchor(n, 1.0f);
    std::memcpy(grid.View().Data(), bytes.data(), bytes.size());
    if (anchorBytes) std::memcpy(anchor.View().Data(), anchorBytes->data(), anchorBytes->size());
    const HostVoxelsGrid<W>* a = anchorBytes ? &anchor : nullptr;
    if (types.find('s') != std::string::npos) run<Types::SEQUENTIAL>("seq", grid, a, mode, iters, prefix);
    if (types.find('o') != std::string::npos) run<Types::OPENMP>("omp", grid, a, mode, iters, prefix);
    if (types.find('n') != std::string::npos) run<Types::NAIVE>("naive", grid, a, mode, iters, prefix);
    if (types.find('t') != std::string::npos) run<Types::TILED>("tiled", grid, a, mode, iters, prefix);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "exhaustive") == 0) return exhaustive();
    if (argc != 10 || std::strcmp(argv[1], "run") != 0) return 2;
    const size_t n = std::strtoul(argv[4], nullptr, 10);
    const int mode = std::atoi(argv[5]);
    const uint32_t iters = static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10));
    const int bits = std::atoi(argv[7]);
    std::vector<char> bytes(n * n * n / 8), anchor(n * n * n / 8);
    if (!slurp(argv[2], bytes)) return 2;
    const bool hasAnchor = std::strcmp(argv[3], "-") != 0;
    if (hasAnchor && !slurp(argv[3], anchor)) return 2;
    if (bits == 32) return all<uint32_t>(bytes, hasAnchor ? &anchor : nullptr, n, mode, iters, argv[8], argv[9]);
    if (bits == 64) return all<uint64_t>(bytes, hasAnchor ? &anchor : nullptr, n, mode, iters, argv[8], argv[9]);
    return 2;
}
