// fill.hip -- interior fill of a whole-grid bit grid for gfx950 (MI355X): vp_fill_interior (include/vphip.h).
//
// A voxel is EXTERIOR if it is not set and lies on the grid boundary or is face-adjacent (6-connectivity) to an exterior voxel; the
// result is the complement of the exterior set E (= scipy.ndimage.binary_fill_holes with its default structure).  d_out holds E while
// the fill runs; fill_final writes NOT E over it.  The only other memory is the context's flag ring (2 kFillBatch words, round_ring.h).
//
// A ROUND is three sweeps, each of which carries E through the runs of empty voxels (p = NOT W) along one axis, over the whole length of
// the axis, in both directions, in one launch:
//   fill_x   one wave segment of L = pow2 >= n/32 lanes per x row (several rows per wave below n = 2048).  In a word the run fill toward
//            higher x is the add-carry trick (((p + s) ^ p) & p) | s, toward lower x the same on __builtin_bitreverse32 of both; across
//            the words of a row a segmented generate / propagate scan over the lanes forwards the carry (a word that is entirely empty
//            propagates it).  Round 0's fill_x also seeds E: NOT W on the six faces (it is the only write of every word of E).
//   fill_y,  columns along y or z, bitwise over the 32 voxels of a word: the recurrence e[k] |= p[k] & e[k - 1] and its mirror is an
//   fill_z   associative generate / propagate scan.  A workgroup owns C columns x S segments (512 lanes; C = 32, 64 from n = 1024): each lane walks its
//            segment once for the summaries (carry out with no carry in, AND of p), the segments' carries are combined through LDS,
//            then the lane walks its segment up and down again with its carry in and stores the words that changed.  Every step also
//            runs the two-direction in-word x fill, which costs a few VALU operations and saves rounds.  Lanes map to consecutive words
//            of a plane (z sweep) or of a row x several z (y sweep).
//   fill_final  out = NOT E, 16 B per lane.
//
// Convergence without a sync per round: the flag ring and the batched host loop of round_ring.h, kFillBatch rounds per read-back; every
// kernel of a round is handed the previous round's flag and its own.
//
// Order-free: within one launch every word of E has exactly one writer (its row lane / its column segment) and is stored only when it
// changed; a sweep only adds bits of NOT W that a 6-path inside NOT W connects to bits already in E.  E therefore only grows and stays a
// subset of the exterior; the carries combined from other segments are lower bounds, so anything missed in one round is found by a
// later one, and a round that changes nothing proves E closed under the 6-neighbour step, i.e. E is the exterior.
#include "round_ring.h"
#include "vp_internal.h"

#include <algorithm>

namespace vp {

namespace {

constexpr uint32_t kFillBatch = 4;  // rounds enqueued between two read-backs of their flags (tests/test_fill_gpu.py reads this line)
constexpr int kYZThreads = 512;     // fill_y / fill_z workgroup: C columns x (512 / C) segments

// the run of p toward higher bits from every seed of s (s subset of p), within one word
__device__ __forceinline__ uint32_t run_up(uint32_t p, uint32_t s) { return (((p + s) ^ p) & p) | s; }

// both directions within one word: every run of p that holds a bit of s
__device__ __forceinline__ uint32_t fill_word(uint32_t s, uint32_t p)
{
    return run_up(p, s) | __builtin_bitreverse32(run_up(__builtin_bitreverse32(p), __builtin_bitreverse32(s)));
}

// Row sweep (x).  Lane `sub` of a segment of L = 1 << lshift lanes holds word `sub` of a row (lanes >= w hold p = e = 0).
__global__ void __launch_bounds__(256)
fill_x(const uint32_t* __restrict__ W, uint32_t* __restrict__ E, uint32_t n, uint32_t w, uint32_t lshift, int seed,
       const uint32_t* prev, uint32_t* cur)
{
    if (round_skip(prev)) return;
    const uint32_t L = 1u << lshift;
    const uint32_t sub = threadIdx.x & (L - 1);
    const uint64_t rows = (uint64_t)n * n;
    const uint32_t perBlock = 256u >> lshift;
    bool changed = false;
    for (uint64_t r0 = (uint64_t)blockIdx.x * perBlock; r0 < rows; r0 += (uint64_t)gridDim.x * perBlock) {
        const uint64_t row = r0 + (threadIdx.x >> lshift);
        const bool valid = row < rows && sub < w;
        const size_t idx = (size_t)row * w + sub;
        uint32_t p = 0u, e = 0u;
        if (valid) {
            p = ~W[idx];
            if (seed) {
                const uint32_t y = (uint32_t)(row % n), z = (uint32_t)(row / n);
                const uint32_t face = (y == 0 || y == n - 1 || z == 0 || z == n - 1) ? ~0u
                                    : ((sub == 0 ? 1u : 0u) | (sub == w - 1 ? 0x80000000u : 0u));
                e = p & face;
            } else {
                e = E[idx];
            }
        }
        // toward higher x: carry out of the word with no carry in (g) and "the word passes a carry through" (t), scanned upward
        uint32_t g = (uint32_t)(((uint64_t)p + e) >> 32), t = p == ~0u ? 1u : 0u;
        // toward lower x: the same on the bit-reversed word, scanned downward
        const uint32_t pr = __builtin_bitreverse32(p), er = __builtin_bitreverse32(e);
        uint32_t gd = (uint32_t)(((uint64_t)pr + er) >> 32), td = t;
        for (uint32_t d = 1; d < L; d <<= 1) {
            const uint32_t gu_ = __shfl_up(g, d, (int)L), tu_ = __shfl_up(t, d, (int)L);
            const uint32_t gd_ = __shfl_down(gd, d, (int)L), td_ = __shfl_down(td, d, (int)L);
            if (sub >= d) { g |= t & gu_; t &= tu_; }
            if (sub + d < L) { gd |= td & gd_; td &= td_; }
        }
        uint32_t cin = __shfl_up(g, 1, (int)L), cind = __shfl_down(gd, 1, (int)L);
        if (sub == 0) cin = 0u;
        if (sub == L - 1) cind = 0u;
        const uint32_t up = run_up(p, e | (p & cin));
        const uint32_t dn = __builtin_bitreverse32(run_up(pr, er | (pr & cind)));
        const uint32_t res = up | dn;
        if (valid && (seed || res != e)) {
            E[idx] = res;
            changed |= res != 0u;
        }
    }
    round_mark(changed, cur);
}

// Column sweep along y (AXIS 1) or z (AXIS 2).  Column c in [0, n w): z sweep -- word c of a plane, stride n w; y sweep -- word c % w of
// the rows of plane c / w, stride w.  Lane = (segment, column of the workgroup's group of C columns).
template <int AXIS>
__global__ void __launch_bounds__(kYZThreads)
fill_yz(const uint32_t* __restrict__ W, uint32_t* __restrict__ E, uint32_t n, uint32_t w, uint32_t C,
        const uint32_t* prev, uint32_t* cur)
{
    if (round_skip(prev)) return;
    __shared__ uint32_t s_gu[kYZThreads], s_gd[kYZThreads], s_p[kYZThreads];
    const uint32_t S = kYZThreads / C;
    const uint32_t Ls = n / S;
    const uint32_t col = threadIdx.x % C, seg = threadIdx.x / C;
    const size_t ncols = (size_t)n * w;
    const size_t stride = AXIS == 2 ? ncols : (size_t)w;
    const uint32_t k0 = seg * Ls, k1 = k0 + Ls;
    bool changed = false;
    for (size_t gidx = blockIdx.x; gidx * C < ncols; gidx += gridDim.x) {
        const size_t c = gidx * C + col;
        const bool valid = c < ncols;
        const size_t base = AXIS == 2 ? c : (c / w) * ncols + (c % w);
        // walk 1: summaries of the segment -- carry out upward (in-word fill folded in), carry out downward, AND of p
        uint32_t gu = 0u, gd = 0u, allp = valid ? ~0u : 0u;
        if (valid) {
            for (uint32_t k = k0; k < k1; k += 8) {
                uint32_t pp[8], ee[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (k + i < k1) { pp[i] = ~W[base + (size_t)(k + i) * stride]; ee[i] = E[base + (size_t)(k + i) * stride]; }
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (k + i < k1) {
                        gu = fill_word(ee[i] | (pp[i] & gu), pp[i]);
                        gd |= ee[i] & allp;
                        allp &= pp[i];
                    }
            }
        }
        s_gu[threadIdx.x] = gu; s_gd[threadIdx.x] = gd; s_p[threadIdx.x] = allp;
        __syncthreads();
        uint32_t cu = 0u, cd = 0u;
        for (uint32_t s = 0; s < seg; ++s) cu = s_gu[s * C + col] | (s_p[s * C + col] & cu);
        for (uint32_t s = S - 1; s > seg; --s) cd = s_gd[s * C + col] | (s_p[s * C + col] & cd);
        __syncthreads();
        if (valid) {
            // walk 2: upward with the carry from the segments below
            uint32_t a = cu;
            for (uint32_t k = k0; k < k1; k += 8) {
                uint32_t pp[8], ee[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (k + i < k1) { pp[i] = ~W[base + (size_t)(k + i) * stride]; ee[i] = E[base + (size_t)(k + i) * stride]; }
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (k + i < k1) {
                        a = fill_word(ee[i] | (pp[i] & a), pp[i]);
                        if (a != ee[i]) { E[base + (size_t)(k + i) * stride] = a; changed = true; }
                    }
            }
            // walk 3: downward with the carry from the segments above, over what walk 2 left
            uint32_t d = cd;
            for (uint32_t j = 0; j < Ls; j += 8) {
                uint32_t pp[8], ee[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (j + i < Ls) {
                        const size_t a_ = base + (size_t)(k1 - 1 - j - i) * stride;
                        pp[i] = ~W[a_]; ee[i] = E[a_];
                    }
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (j + i < Ls) {
                        d = fill_word(ee[i] | (pp[i] & d), pp[i]);
                        if (d != ee[i]) { E[base + (size_t)(k1 - 1 - j - i) * stride] = d; changed = true; }
                    }
            }
        }
    }
    round_mark(changed, cur);
}

__global__ void __launch_bounds__(256)
fill_final(uint4* __restrict__ E, size_t nvec)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const uint4 v = E[i];
        E[i] = make_uint4(~v.x, ~v.y, ~v.z, ~v.w);
    }
}

}  // namespace

int launch_fill_interior(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_out, uint32_t* h_rounds)
{
    hipStream_t st = ctx->stream;
    const uint32_t w = n / 32;
    const size_t nwords = (size_t)n * n * w;
    VP_TRY(reserve(ctx, ctx->fill.flags, 2 * kFillBatch * sizeof(uint32_t), false));
    VP_TRY(ctx->fill.host.need(kFillBatch));
    const RoundRing ring{(uint32_t*)ctx->fill.flags.ptr, kFillBatch, ctx->fill.host.p};

    uint32_t lshift = 0;
    while ((1u << lshift) < w) ++lshift;
    const uint64_t xrows = (uint64_t)n * n, xper = 256u >> lshift;
    const unsigned xblocks = (unsigned)std::min<uint64_t>((xrows + xper - 1) / xper, (uint64_t)ctx->cus * 16);
    const uint32_t C = n >= 1024 ? 64 : 32;
    const unsigned yzblocks = (unsigned)std::min<size_t>((nwords / n + C - 1) / C, (size_t)ctx->cus * 4);

    uint32_t rounds = 0;
    VP_TRY(run_rounds(st, ring, &rounds, nullptr, [&](uint32_t r, const uint32_t* prev, uint32_t* cur) {
        {
            ProfScope p(ctx, VP_K_FILL_X);
            hipLaunchKernelGGL(fill_x, dim3(xblocks), dim3(256), 0, st, d_words, d_out, n, w, lshift, r == 0 ? 1 : 0, prev, cur);
        }
        {
            ProfScope p(ctx, VP_K_FILL_Y);
            hipLaunchKernelGGL(fill_yz<1>, dim3(yzblocks), dim3(kYZThreads), 0, st, d_words, d_out, n, w, C, prev, cur);
        }
        {
            ProfScope p(ctx, VP_K_FILL_Z);
            hipLaunchKernelGGL(fill_yz<2>, dim3(yzblocks), dim3(kYZThreads), 0, st, d_words, d_out, n, w, C, prev, cur);
        }
    }));
    {
        const size_t nvec = nwords / 4;      // n % 32 == 0: whole uint4s; d_out is 16-byte aligned (checked at the ABI)
        const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, (size_t)ctx->cus * 16));
        ProfScope p(ctx, VP_K_FILL_FINAL);
        hipLaunchKernelGGL(fill_final, dim3(blocks), dim3(256), 0, st, (uint4*)d_out, nvec);
    }
    VP_HIP(hipGetLastError());
    VP_HIP(hipStreamSynchronize(st));
    if (h_rounds) *h_rounds = rounds;
    return 0;
}

}  // namespace vp
