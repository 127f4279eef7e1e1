// skeleton_simple.h -- the simple-point test of topological thinning (include/vphip.h, vp_skeleton), shared by the
// kernels of skeleton.hip, the host form of vplib and the check program.  Plain C++: every function is host and device code alike.
//
// A neighbourhood is a 27-bit mask, bit i = (dx+1) + 3 (dy+1) + 9 (dz+1); bit 13 is the centre and is ignored.  simple(m) is Bertrand and
// Malandain's characterisation for (26, 6): (a) the object bits m & N26 are non-empty and one 26-component; (b) the background bits
// ~m & N18 hold a face bit, and all face bits among them lie in one 6-component of ~m & N18.
//   plain form   a flood fill over per-bit adjacency masks, one frontier at a time: the check
//   shift form   in the x + 3 y + 9 z packing a 26-dilation is three masked shift pairs applied separably (+-1, +-3, +-9), a 6-dilation the
//                OR of six masked shifts; a component is grown from its lowest bit for a FIXED number of steps, no data-dependent loop.
//                An exhaustive run over the 2^26 neighbourhoods (tests/cpp/skeleton_check.cpp repeats it) needs at most kSkStepsA - 1
//                dilations until (a)'s component stops growing and kSkStepsB - 1 for (b)'s; the constants include the step that finds
//                the fixed point.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <cstdint>

#if defined(__HIPCC__)
#define VP_SK_HD __host__ __device__ __forceinline__
#else
#define VP_SK_HD inline
#endif

namespace vp {

constexpr uint32_t kSkAll = 0x07FFFFFFu;
constexpr uint32_t kSkCentre = 1u << 13;
constexpr uint32_t kSkN26 = kSkAll & ~kSkCentre;
constexpr uint32_t kSkN6 = (1u << 12) | (1u << 14) | (1u << 10) | (1u << 16) | (1u << 4) | (1u << 22);
constexpr uint32_t kSkCorners = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
constexpr uint32_t kSkN18 = kSkN26 & ~kSkCorners;
constexpr uint32_t kSkXLo = 0x01249249u, kSkXHi = kSkXLo << 2;     // the bits with dx = -1 / +1
constexpr uint32_t kSkYLo = 0x001C0E07u, kSkYHi = kSkYLo << 6;
constexpr uint32_t kSkZLo = 0x000001FFu, kSkZHi = kSkZLo << 18;
constexpr int kSkStepsA = 9;                                       // 26-dilations of (a), the one that finds the fixed point included
constexpr int kSkStepsB = 11;                                      // 6-dilations of (b), likewise
constexpr int kSkModeKernel = 0, kSkModeCurve = 1;                 // VP_SKEL_KERNEL, VP_SKEL_CURVE

// the 27-bit mask of table index c: the 26 non-centre bits, the centre left out
VP_SK_HD uint32_t sk_mask_of_index(uint32_t c) { return (c & 0x1FFFu) | ((c >> 13) << 14); }

VP_SK_HD uint32_t sk_lowest(uint32_t v) { return v & (0u - v); }

VP_SK_HD uint32_t sk_popcount(uint32_t v)
{
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

// ---- shift form ------------------------------------------------------------------------------------------------------------------------
// r and its 26-neighbours inside the cube (bits above 26 may be set: callers mask)
VP_SK_HD uint32_t sk_dilate26(uint32_t r)
{
    r |= ((r & ~kSkXHi) << 1) | ((r & ~kSkXLo) >> 1);
    r |= ((r & ~kSkYHi) << 3) | ((r & ~kSkYLo) >> 3);
    return r | (r << 9) | (r >> 9);
}

// r and its 6-neighbours inside the cube
VP_SK_HD uint32_t sk_dilate6(uint32_t r)
{
    return r | ((r & ~kSkXHi) << 1) | ((r & ~kSkXLo) >> 1) | ((r & ~kSkYHi) << 3) | ((r & ~kSkYLo) >> 3) | (r << 9) | (r >> 9);
}

// the component of `seed` in `allowed` after STEPS dilations
template <int STEPS, bool FACES>
VP_SK_HD uint32_t sk_grow(uint32_t seed, uint32_t allowed)
{
    uint32_t r = seed;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) r = (FACES ? sk_dilate6(r) : sk_dilate26(r)) & allowed;
    return r;
}

VP_SK_HD bool sk_simple_shift(uint32_t m)
{
    const uint32_t obj = m & kSkN26, bg = ~m & kSkN18, faces = bg & kSkN6;
    if (obj == 0u || faces == 0u) return false;
    const uint32_t a = sk_grow<kSkStepsA, false>(sk_lowest(obj), obj);
    const uint32_t b = sk_grow<kSkStepsB, true>(sk_lowest(faces), bg);
    return a == obj && (faces & ~b) == 0u;
}

// ---- plain form ------------------------------------------------------------------------------------------------------------------------
// the 26- (FACES: 6-) neighbours of bit i inside the cube, from its coordinates; evaluated at compile time into SkAdj
template <bool FACES>
constexpr uint32_t sk_adjacent(int i)
{
    const int x = i % 3, y = (i / 3) % 3, z = i / 9;
    uint32_t a = 0u;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int d = (dx != 0) + (dy != 0) + (dz != 0);
                const int u = x + dx, v = y + dy, w = z + dz;
                if (d == 0 || (FACES && d != 1) || u < 0 || u > 2 || v < 0 || v > 2 || w < 0 || w > 2) continue;
                a |= 1u << (u + 3 * v + 9 * w);
            }
    return a;
}

template <bool FACES>
struct SkAdj {
    uint32_t v[27];
    constexpr SkAdj() : v{}
    {
        for (int i = 0; i < 27; ++i) v[i] = sk_adjacent<FACES>(i);
    }
};

// the component of `seed` in `allowed`: one frontier after the other, at most 26 of them; *steps = the frontiers that added a bit
template <bool FACES>
VP_SK_HD uint32_t sk_flood(uint32_t seed, uint32_t allowed, int* steps = nullptr)
{
    constexpr SkAdj<FACES> adj;
    uint32_t reach = seed, frontier = seed;
    int count = 0;
    for (int round = 0; round < 27 && frontier != 0u; ++round) {
        uint32_t next = 0u, rest = frontier;
        for (int k = 0; k < 27 && rest != 0u; ++k) {
            next |= adj.v[__builtin_ctz(rest)];
            rest &= rest - 1u;
        }
        next &= allowed & ~reach;
        reach |= next;
        frontier = next;
        count += next != 0u;
    }
    if (steps) *steps = count;
    return reach;
}

VP_SK_HD bool sk_simple_plain(uint32_t m, int* steps_a = nullptr, int* steps_b = nullptr)
{
    const uint32_t obj = m & kSkN26, bg = ~m & kSkN18, faces = bg & kSkN6;
    if (steps_a) *steps_a = 0;
    if (steps_b) *steps_b = 0;
    if (obj == 0u || faces == 0u) return false;
    const uint32_t a = sk_flood<false>(sk_lowest(obj), obj, steps_a);
    const uint32_t b = sk_flood<true>(sk_lowest(faces), bg, steps_b);
    return a == obj && (faces & ~b) == 0u;
}

// the deletion rule of one examined voxel: simple, and in curve mode not a line end
template <bool SHIFT>
VP_SK_HD bool sk_deletable(uint32_t m, int mode)
{
    if (mode == kSkModeCurve && sk_popcount(m & kSkN26) == 1u) return false;
    return SHIFT ? sk_simple_shift(m) : sk_simple_plain(m);
}

}  // namespace vp
