// VOX::DistanceTransform, VOX::MorphExact and JFA::ComputeExact on T = uint32_t and T = uint64_t grids with the same voxels: prints one
// FNV-1a-64 hash per (type, call, T) for the Python test to compare (the two T must agree, and so must every type).
//   edt_check <n> <radius> <gpu:0|1>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <jfa/jfa.h>
#include <vox/vox.h>

static uint64_t fnv(const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

// keep = the chance in 256 of a set voxel
template <typename T>
static void fill(HostVoxelsGrid<T>& g, size_t n, uint32_t keep)
{
    uint32_t s = 12345u;
    for (size_t z = 0; z < n; ++z) for (size_t y = 0; y < n; ++y) for (size_t x = 0; x < n; ++x) {
        s = s * 1664525u + 1013904223u;
        if ((s >> 24) < keep) g.View().Voxel(x, y, z) = true;
    }
}

template <Types TY, typename T>
static void run(const char* tag, size_t n, uint32_t radius)
{
    const float vs = 0.75f / static_cast<float>(n);
    for (int seeds = 0; seeds < 3; ++seeds) {
        HostVoxelsGrid<T> g(n, vs);
        fill(g, n, seeds == 0 ? 2u : 220u);                                  // few seeds for SET, few for UNSET, a dense solid for BORDER
        HostGrid<uint32_t> d;
        VOX::DistanceTransform<TY>(g, d, static_cast<VOX::EdtSeeds>(seeds));
        std::printf("%s edt%d %016lx\n", tag, seeds, fnv(d.View().Data(), n * n * n * 4));
    }
    for (int op = 0; op < 4; ++op) {
        HostVoxelsGrid<T> g(n, vs);
        fill(g, n, (op == 0 || op == 3) ? 3u : 254u);                        // sparse for dilate / close, dense for erode / open
        VOX::MorphExact<TY>(g, static_cast<VOX::MorphOp>(op), radius);
        std::printf("%s op%d %016lx\n", tag, op, fnv(g.View().Data(), n * n * n / 8));
    }
    {
        HostVoxelsGrid<T> g(n, vs);
        fill(g, n, 220u);
        HostGrid<float> sdf(n, -INFINITY);
        JFA::ComputeExact<TY>(g, sdf);
        std::printf("%s sdf %016lx\n", tag, fnv(sdf.View().Data(), n * n * n * 4));
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
