// VOX::Morph on T = uint32_t and T = uint64_t grids with the same voxels: prints one FNV-1a-64 hash of the grid bytes per (type, op,
// T) for the Python test to compare (the two T must agree, and so must SEQUENTIAL and OPENMP).
//   morph_check <n> <radius> <gpu:0|1>
#include <cstdio>
#include <cstdlib>

#include <vox/vox.h>

static uint64_t fnv(const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

template <Types TY, typename T>
static void run(const char* tag, size_t n, uint32_t radius)
{
    for (int op = 0; op < 4; ++op) {
        HostVoxelsGrid<T> g(n, 1.0f / static_cast<float>(n));
        uint32_t s = 12345u;
        for (size_t z = 0; z < n; ++z) for (size_t y = 0; y < n; ++y) for (size_t x = 0; x < n; ++x) {
            s = s * 1664525u + 1013904223u;
            const uint32_t keep = (op == 0 || op == 3) ? 3u : 200u;          // sparse for dilate / close, dense for erode / open
            if ((s >> 24) < keep) g.View().Voxel(x, y, z) = true;
        }
        VOX::Morph<TY>(g, static_cast<VOX::MorphOp>(op), radius);
        std::printf("%s op%d %016lx\n", tag, op, fnv(g.View().Data(), n * n * n / 8));
    }
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const size_t n = std::strtoul(argv[1], nullptr, 10);
    const uint32_t radius = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10));
    run<Types::SEQUENTIAL, uint32_t>("seq32", n, radius);
    run<Types::SEQUENTIAL, uint64_t>("seq64", n, radius);
    run<Types::OPENMP, uint32_t>("omp32", n, radius);
    run<Types::OPENMP, uint64_t>("omp64", n, radius);
    if (std::atoi(argv[3]) != 0) {
        run<Types::NAIVE, uint32_t>("naive32", n, radius);
        run<Types::NAIVE, uint64_t>("naive64", n, radius);
        run<Types::TILED, uint32_t>("tiled32", n, radius);
        run<Types::TILED, uint64_t>("tiled64", n, radius);
    }
    return 0;
}
