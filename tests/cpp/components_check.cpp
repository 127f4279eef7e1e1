// VOX::LabelComponents / VOX::FilterComponents on T = uint32_t and T = uint64_t grids with the same voxels: prints, per (type, T,
// connectivity), K and one FNV-1a-64 hash of the label volume, then K, the kept voxels and the hash of the grid after KEEP_LARGEST 2
// and after MIN_VOXELS 3, for the Python test to compare (the two T must agree, and so must SEQUENTIAL and OPENMP).
//   components_check <n> <density 0..255> <gpu:0|1>
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

template <typename T>
static HostVoxelsGrid<T> make(size_t n, uint32_t density)
{
    HostVoxelsGrid<T> g(n, 1.0f / static_cast<float>(n));
    for (size_t z = 0; z < n; ++z) for (size_t y = 0; y < n; ++y) for (size_t x = 0; x < n; ++x) {
        uint32_t h = static_cast<uint32_t>(x + n * (y + n * z)) * 2654435761u;      // the test rebuilds the voxels from this hash
        h ^= h >> 15;
        h *= 2246822519u;
        if ((h >> 24) < density) g.View().Voxel(x, y, z) = true;
    }
    return g;
}

template <Types TY, typename T>
static void run(const char* tag, size_t n, uint32_t density)
{
    for (int conn : {6, 26}) {
        HostVoxelsGrid<T> g = make<T>(n, density);
        HostGrid<uint32_t> labels;
        const uint32_t k = VOX::LabelComponents<TY>(g, labels, conn);
        std::printf("%s %d label %u 0 %016lx\n", tag, conn, k, fnv(labels.View().Data(), n * n * n * 4));
        VOX::ComponentStats st = VOX::FilterComponents<TY>(g, VOX::ComponentFilter::KEEP_LARGEST, 2u, conn);
        std::printf("%s %d largest2 %u %llu %016lx\n", tag, conn, st.count, static_cast<unsigned long long>(st.kept), fnv(g.View().Data(), n * n * n / 8));
        g = make<T>(n, density);
        st = VOX::FilterComponents<TY>(g, VOX::ComponentFilter::MIN_VOXELS, 3u, conn);
        std::printf("%s %d min3 %u %llu %016lx\n", tag, conn, st.count, static_cast<unsigned long long>(st.kept), fnv(g.View().Data(), n * n * n / 8));
    }
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const size_t n = std::strtoul(argv[1], nullptr, 10);
    const uint32_t density = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10));
    run<Types::SEQUENTIAL, uint32_t>("seq32", n, density);
    run<Types::SEQUENTIAL, uint64_t>("seq64", n, density);
    run<Types::OPENMP, uint32_t>("omp32", n, density);
    run<Types::OPENMP, uint64_t>("omp64", n, density);
    if (std::atoi(argv[3]) != 0) {
        run<Types::NAIVE, uint32_t>("naive32", n, density);
        run<Types::NAIVE, uint64_t>("naive64", n, density);
        run<Types::TILED, uint32_t>("tiled32", n, density);
        run<Types::TILED, uint64_t>("tiled64", n, density);
    }
    return 0;
}
