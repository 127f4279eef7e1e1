// octree.cpp -- VOX::BuildOctree / ExpandOctree back ends: the host restatement of vp_octree (include/vphip.h), the marshalling of the GPU
// variants onto the C ABI, the point query, the structural check and the .svo file.
//
// The host build is a pyramid over the words: one state byte (0 empty, 1 mixed, 2 full) per cell of the levels 0 .. L - 1, in Morton
// order, so that the children of cell m are the cells 8 m .. 8 m + 7 one level down; level L - 1 reads its eight voxels from the words.
// The records of a level are then written in runs of cells: a first sweep counts the stored cells and their mixed children per run, a
// serial prefix turns the counts into positions, a second sweep writes.  OPENMP runs the sweeps in parallel over the runs; the bytes are
// the same.  It does not call the library.
#include <algorithm>
#include <bit>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "debug_utils.h"
#include "profiling.h"
#include "vox/octree.h"
#include "vp_runtime.h"

namespace VOX {

namespace {

constexpr char kMagic[8] = {'V', 'P', 'S', 'V', 'O', '1', '\0', '\0'};
constexpr size_t kRun = 4096;                                     // cells per run of the record sweeps

uint32_t Compact3(uint32_t m)                                     // every third bit of a Morton code, from bit 0
{
    uint32_t x = m & 0x09249249u;
    x = (x ^ (x >> 2)) & 0x030C30C3u;
    x = (x ^ (x >> 4)) & 0x0300F00Fu;
    x = (x ^ (x >> 8)) & 0x030000FFu;
    x = (x ^ (x >> 16)) & 0x000003FFu;
    return x;
}

uint32_t LevelsOf(size_t n)
{
    uint32_t L = 5;
    while ((size_t{1} << L) < n) ++L;
    return L;
}

bool SideServed(size_t n) { return n >= 32 && n <= 1024 && n % 32 == 0; }

// the eight voxels of the side-2 cell with Morton code m, bit c = x + 2 y + 4 z; outside the grid: unset
uint32_t CellBits(const uint32_t* words, size_t n, size_t m)
{
    const size_t x = 2 * size_t{Compact3(static_cast<uint32_t>(m))}, y = 2 * size_t{Compact3(static_cast<uint32_t>(m >> 1))},
                 z = 2 * size_t{Compact3(static_cast<uint32_t>(m >> 2))};
    if (x >= n || y >= n || z >= n) return 0;
    const size_t w = n / 32;
    uint32_t v = 0;
    for (size_t dz = 0; dz < 2; ++dz)
        for (size_t dy = 0; dy < 2; ++dy)
            v |= ((words[(x >> 5) + w * ((y + dy) + n * (z + dz))] >> (x & 31)) & 3u) << (2 * dy + 4 * dz);
    return v;
}

void ChildMasks(const uint8_t* child, size_t m, uint32_t& valid, uint32_t& full)
{
    valid = full = 0;
    for (uint32_t c = 0; c < 8; ++c) {
        const uint8_t s = child[8 * m + c];
        valid |= (s != 0 ? 1u : 0u) << c;
        full |= (s == 2 ? 1u : 0u) << c;
    }
}

uint8_t StateOf(uint32_t valid, uint32_t full) { return valid == 0 ? 0 : (full == 0xFFu ? 2 : 1); }

void SetBox(uint32_t* words, size_t n, size_t x0, size_t y0, size_t z0, size_t side)
{
    const size_t w = n / 32;
    for (size_t z = z0; z < z0 + side; ++z)
        for (size_t y = y0; y < y0 + side; ++y) {
            uint32_t* row = words + w * (y + n * z);
            if (side >= 32) std::fill(row + x0 / 32, row + (x0 + side) / 32, 0xFFFFFFFFu);
            else row[x0 >> 5] |= ((1u << side) - 1u) << (x0 & 31);
        }
}

void ExpandNode(const Octree& t, uint32_t node, uint32_t level, size_t x, size_t y, size_t z, uint32_t* words)
{
    const uint32_t masks = t.nodes[2 * size_t{node}], first = t.nodes[2 * size_t{node} + 1];
    const uint32_t valid = masks & 0xFFu, full = (masks >> 8) & 0xFFu;
    const size_t side = size_t{t.P} >> (level + 1);
    uint32_t rank = 0;
    for (uint32_t c = 0; c < 8; ++c) {
        const size_t cx = x + (c & 1u) * side, cy = y + ((c >> 1) & 1u) * side, cz = z + (c >> 2) * side;
        if ((full >> c) & 1u) SetBox(words, t.n, cx, cy, cz, side);
        else if ((valid >> c) & 1u) ExpandNode(t, first + rank++, level + 1, cx, cy, cz, words);
    }
}

bool Fail(std::string* why, const std::string& what)
{
    if (why) *why = what;
    return false;
}

}  // namespace

bool Octree::Test(uint32_t x, uint32_t y, uint32_t z) const
{
    if (x >= n || y >= n || z >= n || nodes.empty()) return false;
    size_t node = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t sh = L - 1 - l, c = ((x >> sh) & 1u) | (((y >> sh) & 1u) << 1) | (((z >> sh) & 1u) << 2);
        const uint32_t masks = nodes[2 * node], valid = masks & 0xFFu, full = (masks >> 8) & 0xFFu;
        if (!((valid >> c) & 1u)) return false;
        if ((full >> c) & 1u) return true;
        node = size_t{nodes[2 * node + 1]} + static_cast<size_t>(std::popcount(valid & ~full & ((1u << c) - 1u)));
        if (node == 0 || node >= NodeCount()) return false;
    }
    return false;
}

bool Octree::Validate(std::string* why) const
{
    if (!SideServed(n)) return Fail(why, "the side is not a multiple of 32 in 32 .. 1024");
    if (L != LevelsOf(n) || P != (1u << L)) return Fail(why, "P and L do not belong to n");
    const uint64_t M = NodeCount();
    if (nodes.size() % 2 || M < 1 || M >= (uint64_t{1} << 28)) return Fail(why, "the node count is outside 1 .. 2^28 - 1");
    struct Cell { uint16_t x, y, z; };
    std::vector<Cell> level{Cell{0, 0, 0}}, next;
    uint32_t offsets[11], fulls[11] = {};
    uint64_t begin = 0, running = 1;
    for (uint32_t l = 0; l < 11; ++l) {
        offsets[l] = static_cast<uint32_t>(begin);
        if (l >= L || level.empty()) continue;
        const uint32_t side = P >> (l + 1);
        next.clear();
        for (size_t k = 0; k < level.size(); ++k) {
            const uint64_t i = begin + k;
            const std::string at = "node " + std::to_string(i) + ": ";
            const uint32_t masks = nodes[2 * i], child = nodes[2 * i + 1], valid = masks & 0xFFu, full = (masks >> 8) & 0xFFu, mixed = valid & ~full;
            if (masks >> 16) return Fail(why, at + "upper mask bits set");
            if (full & ~valid) return Fail(why, at + "full is not a subset of valid");
            if (l > 0 && (valid == 0 || full == 0xFFu)) return Fail(why, at + "a stored cell that is not mixed");
            if (l == L - 1 && mixed) return Fail(why, at + "a voxel that is neither set nor unset");
            if (child != (mixed ? running : 0)) return Fail(why, at + "child is not the running sum");
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t cx = 2u * level[k].x + (c & 1u), cy = 2u * level[k].y + ((c >> 1) & 1u), cz = 2u * level[k].z + (c >> 2);
                const uint32_t far = std::max({cx, cy, cz}) * side;
                if (((full >> c) & 1u) && far + side > n) return Fail(why, at + "a full child pokes out of the grid");
                if (((valid >> c) & 1u) && far >= n) return Fail(why, at + "a child outside the grid");
                if ((mixed >> c) & 1u) next.push_back(Cell{static_cast<uint16_t>(cx), static_cast<uint16_t>(cy), static_cast<uint16_t>(cz)});
            }
            fulls[l] += static_cast<uint32_t>(std::popcount(full));
            running += static_cast<uint64_t>(std::popcount(mixed));
            if (running > M) return Fail(why, at + "children beyond the last node");
        }
        begin += level.size();
        level.swap(next);
    }
    if (running != M) return Fail(why, "the levels do not end at the node count");
    for (uint32_t l = 0; l < 11; ++l)
        if (levelOffset[l] != offsets[l] || fullLeaves[l] != fulls[l]) return Fail(why, "a summary does not belong to the records");
    return true;
}

namespace detail {

void OctreeHost(bool parallel, const uint32_t* words, size_t n, Octree& t)
{
    PROFILING_SCOPE(parallel ? "OpenMPOctree" : "SequentialOctree");
    cpuAssert(SideServed(n), "Octree: the grid side must be a multiple of 32 in 32..1024\n");
    const uint32_t L = LevelsOf(n);
    t = Octree{};
    t.n = static_cast<uint32_t>(n); t.L = L; t.P = 1u << L;
    std::vector<std::vector<uint8_t>> st(L);
    for (uint32_t l = 0; l < L; ++l) st[l].resize(size_t{1} << (3 * l));
    {
        uint8_t* leaf = st[L - 1].data();
        const int64_t cells = static_cast<int64_t>(st[L - 1].size());
#pragma omp parallel for schedule(static) if (parallel)
        for (int64_t m = 0; m < cells; ++m) {
            const uint32_t v = CellBits(words, n, static_cast<size_t>(m));
            leaf[m] = StateOf(v, v);
        }
    }
    for (int l = static_cast<int>(L) - 2; l >= 0; --l) {
        const uint8_t* child = st[l + 1].data();
        uint8_t* mine = st[l].data();
        const int64_t cells = static_cast<int64_t>(st[l].size());
#pragma omp parallel for schedule(static) if (parallel)
        for (int64_t m = 0; m < cells; ++m) {
            uint32_t valid, full;
            ChildMasks(child, static_cast<size_t>(m), valid, full);
            mine[m] = StateOf(valid, full);
        }
    }
    // per level and run of cells: the stored cells, their mixed children and their full children
    struct Run { uint64_t stored = 0, kids = 0, fulls = 0; };
    std::vector<std::vector<Run>> runs(L);
    auto masks_of = [&](uint32_t l, size_t m, uint32_t& valid, uint32_t& full) {
        if (l == L - 1) valid = full = CellBits(words, n, m);
        else ChildMasks(st[l + 1].data(), m, valid, full);
    };
    for (uint32_t l = 0; l < L; ++l) {
        const size_t cells = st[l].size();
        runs[l].resize((cells + kRun - 1) / kRun);
        const int64_t count = static_cast<int64_t>(runs[l].size());
#pragma omp parallel for schedule(dynamic) if (parallel)
        for (int64_t r = 0; r < count; ++r) {
            Run run;
            for (size_t m = static_cast<size_t>(r) * kRun; m < std::min(cells, (static_cast<size_t>(r) + 1) * kRun); ++m) {
                if (!(st[l][m] == 1 || l == 0)) continue;
                uint32_t valid, full;
                masks_of(l, m, valid, full);
                ++run.stored;
                run.kids += static_cast<uint64_t>(std::popcount(valid & ~full));
                run.fulls += static_cast<uint64_t>(std::popcount(full));
            }
            runs[l][static_cast<size_t>(r)] = run;
        }
    }
    uint64_t total = 0;
    for (uint32_t l = 0; l < 11; ++l) {
        t.levelOffset[l] = static_cast<uint32_t>(total);
        if (l >= L) continue;
        uint64_t fulls = 0;
        for (const Run& r : runs[l]) { total += r.stored; fulls += r.fulls; }
        t.fullLeaves[l] = static_cast<uint32_t>(fulls);
    }
    t.nodes.assign(2 * total, 0u);
    for (uint32_t l = 0; l < L; ++l) {
        const size_t cells = st[l].size();
        std::vector<uint64_t> at(runs[l].size()), kid(runs[l].size());
        uint64_t a = t.levelOffset[l], k = t.levelOffset[l + 1];
        for (size_t r = 0; r < runs[l].size(); ++r) { at[r] = a; kid[r] = k; a += runs[l][r].stored; k += runs[l][r].kids; }
        const int64_t count = static_cast<int64_t>(runs[l].size());
#pragma omp parallel for schedule(dynamic) if (parallel)
        for (int64_t r = 0; r < count; ++r) {
            uint64_t node = at[static_cast<size_t>(r)], first = kid[static_cast<size_t>(r)];
            if (runs[l][static_cast<size_t>(r)].stored == 0) continue;
            for (size_t m = static_cast<size_t>(r) * kRun; m < std::min(cells, (static_cast<size_t>(r) + 1) * kRun); ++m) {
                if (!(st[l][m] == 1 || l == 0)) continue;
                uint32_t valid, full;
                masks_of(l, m, valid, full);
                const uint32_t mixed = valid & ~full;
                t.nodes[2 * node] = valid | (full << 8);
                t.nodes[2 * node + 1] = mixed ? static_cast<uint32_t>(first) : 0u;
                ++node;
                first += static_cast<uint64_t>(std::popcount(mixed));
            }
        }
    }
}

void OctreeExpandHost(const Octree& t, uint32_t* words)
{
    PROFILING_SCOPE("HostOctreeExpand");
    std::string why;
    cpuAssert(t.Validate(&why), "Octree: not a well-formed tree: " + why + "\n");
    std::fill(words, words + size_t{t.n} * t.n * t.n / 32, 0u);
    ExpandNode(t, 0, 0, 0, 0, 0, words);
}

static vp_frame FrameOf(size_t n, float vs, const float origin[3])
{
    vp_frame f{};
    f.n = static_cast<uint32_t>(n); f.voxel_size = vs;
    f.origin[0] = origin[0]; f.origin[1] = origin[1]; f.origin[2] = origin[2];
    f.z0 = 0; f.z1 = f.n;
    return f;
}

void OctreeDevice(int algo, const char* label, const uint32_t* words, size_t n, float vs, const float origin[3], Octree& t)
{
    const std::string name(label);
    PROFILING_SCOPE(name);
    cpuAssert(vplib::Multi() == nullptr, "The octree is built on one device (no -g > 1)\n");
    cpuAssert(SideServed(n), "Octree: the grid side must be a multiple of 32 in 32..1024\n");
    const vp_frame f = FrameOf(n, vs, origin);
    vp_ctx* ctx = vplib::Context();
    t = Octree{};
    t.n = f.n; t.L = LevelsOf(n); t.P = 1u << t.L;
#if PROFILING
    gpuAssert(vp_prof_reset(ctx));
    gpuAssert(vp_prof_enable(ctx, 1));
#endif
    {
        PROFILING_SCOPE(name + "::Processing");
        uint64_t count = 0;
        // the first call learns the count (a capacity of 0 is refused with the count stored), the second one has the room
        const int rc = vp_octree_host(ctx, &f, words, algo, nullptr, 0, &count, nullptr, nullptr);
        cpuAssert(rc == VP_ERR_INVALID && count > 0, std::string("vp_octree_host: ") + vp_last_error() + "\n");
        t.nodes.assign(2 * count, 0u);
        gpuAssert(vp_octree_host(ctx, &f, words, algo, t.nodes.data(), count, &count, t.levelOffset, t.fullLeaves));
    }
#if PROFILING
    gpuAssert(vp_prof_enable(ctx, 0));
#endif
}

void OctreeExpandDevice(int algo, const char* label, const Octree& t, uint32_t* words)
{
    const std::string name(label);
    PROFILING_SCOPE(name);
    cpuAssert(vplib::Multi() == nullptr, "The octree is expanded on one device (no -g > 1)\n");
    std::string why;
    cpuAssert(t.Validate(&why), "Octree: not a well-formed tree: " + why + "\n");
    const vp_frame f = FrameOf(t.n, t.voxelSize, t.origin);
    gpuAssert(vp_octree_expand_host(vplib::Context(), &f, t.nodes.data(), t.NodeCount(), algo, words));
}

}  // namespace detail

bool WriteOctree(const std::string& path, const Octree& t)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const uint32_t head[4] = {t.n, t.P, t.L, static_cast<uint32_t>(t.NodeCount())};
    const float frame[4] = {t.voxelSize, t.origin[0], t.origin[1], t.origin[2]};
    bool ok = std::fwrite(kMagic, 1, 8, f) == 8 && std::fwrite(head, 4, 4, f) == 4 && std::fwrite(frame, 4, 4, f) == 4 &&
              std::fwrite(t.levelOffset, 4, 11, f) == 11 && std::fwrite(t.fullLeaves, 4, 11, f) == 11 &&
              std::fwrite(t.nodes.data(), 4, t.nodes.size(), f) == t.nodes.size();
    ok = std::fclose(f) == 0 && ok;
    return ok;
}

bool ReadOctree(const std::string& path, Octree& t, std::string* why)
{
    t = Octree{};
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return Fail(why, "cannot open " + path);
    char magic[8];
    uint32_t head[4];
    float frame[4];
    Octree r;
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, kMagic, 8) == 0 && std::fread(head, 4, 4, f) == 4 &&
              std::fread(frame, 4, 4, f) == 4 && std::fread(r.levelOffset, 4, 11, f) == 11 && std::fread(r.fullLeaves, 4, 11, f) == 11;
    if (ok) {
        // the size of the rest of the file decides how much is read, never the header alone
        const long at = std::ftell(f);
        ok = at >= 0 && std::fseek(f, 0, SEEK_END) == 0;
        const long end = ok ? std::ftell(f) : -1;
        ok = ok && end >= at && std::fseek(f, at, SEEK_SET) == 0 && head[3] >= 1 && head[3] < (1u << 28) &&
             static_cast<uint64_t>(end - at) == uint64_t{head[3]} * 8;
        if (ok) {
            r.nodes.resize(2 * size_t{head[3]});
            ok = std::fread(r.nodes.data(), 4, r.nodes.size(), f) == r.nodes.size();
        }
    }
    std::fclose(f);
    if (!ok) return Fail(why, path + " is not an .svo file of the size its header states");
    r.n = head[0]; r.P = head[1]; r.L = head[2];
    r.voxelSize = frame[0]; r.origin[0] = frame[1]; r.origin[1] = frame[2]; r.origin[2] = frame[3];
    if (!r.Validate(why)) return false;
    t = std::move(r);
    return true;
}

}  // namespace VOX
