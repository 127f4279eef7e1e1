// regions.h -- VOX::AnalyzeRegions: per-label volume, bounding box, moments, surface, contact, Euler number and value statistics of a label
// volume (include/vphip.h, vp_regions).  No reference counterpart.
//
// `labels` holds one uint32 per voxel, x fastest, as VOX::LabelComponents and VOX::Watershed write it; the effective label of a voxel is its
// label where that is 1 .. count, else 0 (labels above `count` are ignored, outside the grid the label is 0).  `values` is an optional field
// of one uint32 per voxel (a squared distance, a thickness, a geodesic distance).  Record k - 1 of the result belongs to label k and holds
// the 26 integer words of include/vphip.h; a label without a voxel has an all-zero record.
//   SEQUENTIAL / OPENMP   host restatement (regions.cpp): one pass over a volume padded by one layer, run by run along x; it does not call
//                         the library.  OPENMP deals the z planes to threads, which merge their runs into the table under a lock per label
//                         group: every word is an integer sum, minimum or maximum, so the order does not show.  Any grid side
//   NAIVE / TILED         vp_regions_host with VP_ALGO_NAIVE / VP_ALGO_TILED (n % 32 == 0, n <= 1024)
// Every variant produces the same bytes and the same totals.
#ifndef VPLIB_REGIONS_H
#define VPLIB_REGIONS_H

#include <array>
#include <cmath>
#include <cstdint>
#include <vector>

#include "vox/vox.h"

namespace VOX {

constexpr uint32_t REGION_WORDS = 26;                                                     // VP_REGION_WORDS
constexpr uint32_t REGIONS_MAX = 0xFFFFFu;                                                // VP_REGIONS_MAX

// sum of V, labels with V > 0, voxels whose label lies above `count` (ignored), interfaces = sum of the contact faces / 2
struct RegionTotals { uint64_t voxels, labels, ignored, interfaces; };

// The record of one label: the 26 words, and what follows from them.  Coordinates of the words are voxel indices; the accessors that take a
// voxel size (and an origin) answer in world units.
struct RegionStats {
    uint64_t w[REGION_WORDS];

    uint64_t Voxels() const { return w[0]; }
    bool Empty() const { return w[0] == 0; }
    std::array<uint64_t, 3> BoxMin() const { return {w[1], w[2], w[3]}; }                // the lowest and highest voxel per axis, inclusive
    std::array<uint64_t, 3> BoxMax() const { return {w[4], w[5], w[6]}; }
    uint64_t ExposedFaces() const { return w[16] + w[17] + w[18]; }
    uint64_t ContactFaces() const { return w[19]; }
    uint64_t FirstIndex() const { return w[25]; }                                         // x + n (y + n z)
    double Volume(double vs) const { return static_cast<double>(w[0]) * vs * vs * vs; }
    std::array<double, 3> Centroid(double vs, const float origin[3]) const
    {
        const double v = Empty() ? 1.0 : static_cast<double>(w[0]);
        return {(static_cast<double>(w[7]) / v + 0.5) * vs + origin[0], (static_cast<double>(w[8]) / v + 0.5) * vs + origin[1],
                (static_cast<double>(w[9]) / v + 0.5) * vs + origin[2]};
    }
    // covariance of the voxel centres plus 1/12 per axis for the voxel's own extent, times vs^2: xx, yy, zz, xy, xz, yz.  The second
    // moments are taken about an integer point near the middle of the box in exact integer arithmetic first
    std::array<double, 6> Covariance(double vs) const
    {
        if (Empty()) return {0, 0, 0, 0, 0, 0};
        const int64_t v = static_cast<int64_t>(w[0]);
        int64_t c[3], s1[3];
        for (int a = 0; a < 3; ++a) {
            c[a] = static_cast<int64_t>((w[1 + a] + w[4 + a]) / 2);
            s1[a] = static_cast<int64_t>(w[7 + a]) - c[a] * v;
        }
        const int pairs[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
        std::array<double, 6> out{};
        for (int k = 0; k < 6; ++k) {
            const int a = pairs[k][0], b = pairs[k][1];
            const int64_t s2 = static_cast<int64_t>(w[10 + k]) - c[a] * static_cast<int64_t>(w[7 + b]) - c[b] * static_cast<int64_t>(w[7 + a]) + c[a] * c[b] * v;
            const double d = static_cast<double>(v);
            out[k] = (static_cast<double>(s2) / d - (static_cast<double>(s1[a]) / d) * (static_cast<double>(s1[b]) / d) + (a == b ? 1.0 / 12.0 : 0.0)) * vs * vs;
        }
        return out;
    }
    // the three-direction Crofton estimate S = (2 / 3) F vs^2: anisotropic, a few per cent on round shapes
    double SurfaceArea(double vs) const { return 2.0 / 3.0 * static_cast<double>(ExposedFaces()) * vs * vs; }
    double ContactArea(double vs) const { return static_cast<double>(w[19]) * vs * vs; }
    double Sphericity() const
    {
        const double s = SurfaceArea(1.0);
        return s > 0 ? std::cbrt(3.14159265358979323846) * std::pow(6.0 * static_cast<double>(w[0]), 2.0 / 3.0) / s : 0.0;
    }
    // of the closed-cube complex (26-connected foreground): n0 - n1 + n2 - V with n2 = (6 V + F) / 2
    int64_t EulerNumber() const
    {
        return static_cast<int64_t>(w[20]) - static_cast<int64_t>(w[21]) + static_cast<int64_t>((6 * w[0] + ExposedFaces()) / 2) - static_cast<int64_t>(w[0]);
    }
    double ValueMean() const { return Empty() ? 0.0 : static_cast<double>(w[22]) / static_cast<double>(w[0]); }
    uint64_t ValueMin() const { return w[23]; }
    uint64_t ValueMax() const { return w[24]; }
};
static_assert(sizeof(RegionStats) == REGION_WORDS * sizeof(uint64_t), "a vector of RegionStats is the table of vp_regions");

namespace detail {
// the host form refuses a count above REGIONS_MAX with cpuAssert, as the library refuses it
RegionTotals RegionsHost(bool parallel, const uint32_t* labels, uint32_t count, const uint32_t* values, size_t n, RegionStats* table);
RegionTotals RegionsDevice(int algo, const char* label, const uint32_t* labels, uint32_t count, const uint32_t* values, size_t n, RegionStats* table);
}  // namespace detail

// `values` (may be nullptr) has the side of `labels`; `totals`, when given, gets the four totals
template <Types type>
std::vector<RegionStats> AnalyzeRegions(const HostGrid<uint32_t>& labels, uint32_t count, const HostGrid<uint32_t>* values = nullptr,
                                        RegionTotals* totals = nullptr)
{
    const size_t n = labels.View().SizeX();
    std::vector<RegionStats> table(count);
    const uint32_t* vw = values ? values->View().Data() : nullptr;
    RegionTotals t;
    if constexpr (type == Types::SEQUENTIAL || type == Types::OPENMP)
        t = detail::RegionsHost(type == Types::OPENMP, labels.View().Data(), count, vw, n, table.data());
    else
        t = detail::RegionsDevice(type == Types::NAIVE ? 1 : 2, type == Types::NAIVE ? "NaiveRegions" : "TiledRegions", labels.View().Data(), count, vw,
                                  n, table.data());
    if (totals) *totals = t;
    return table;
}

}  // namespace VOX

#endif
