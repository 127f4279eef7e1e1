// edt.hip -- exact Euclidean distance transform of a whole-grid bit grid for gfx950 (MI355X): vp_edt, vp_edt_sdf, vp_edt_morph
// (include/vphip.h).
//
// D(p) = min over the seed voxels q of |p - q|^2, integer voxel coordinates, uint32; kNone where there is no seed.  The minimum separates:
//   x pass      g(x, y, z) = min over the seeds (x', y, z) of the row of (x - x')^2
//   y / z pass  out(i) = min over j of in(j) + (i - j)^2 along a column
// Everything is integer arithmetic, so both algos, the host restatements and numpy agree bit for bit.  kNone never enters an addition:
// a column entry that is kNone is no candidate.
//   edt_x          both algos.  A workgroup owns 256 / w whole rows (w = n / 32 words).  The seed words of its rows go to LDS (complemented on
//                  load for SEEDS_UNSET); one lane per word finds the nearest non-zero word strictly left and right of its own (at most
//                  31 LDS reads each way); then one lane per voxel: the nearest seed bit at or below x is in the own word (clz of the bits
//                  0 .. b) or the top bit of the left word found, the nearest at or above x likewise (ctz).  Stores are coalesced along x.
//                  SEEDS_BORDER runs on the border mask jfa_border_march (jfa_seed.hip) leaves in a buffer of the context.
//   edt_col_naive  one thread per voxel from global memory into a second volume: candidates at distance d = 1, 2, ... on both sides while
//                  d^2 is below the best so far (a candidate at distance d costs at least d^2).
//   edt_col_tiled  a workgroup stages the whole columns of BX adjacent x (a bundle: 32, or 16 above n = 512, so that n * BX * 4 bytes <= 64 KiB:
//                  two workgroups per CU) as 16-byte loads, runs the same bounded search on LDS -- lanes of a wave read 32 consecutive words
//                  of a row: no bank conflicts -- and writes back IN PLACE: the bundle's columns are read by nobody else.  A bundle
//                  without any seed is left as it is (no search, no store), and an entry the pass does not lower is not stored.
//   edt_to_sdf     D -> +-((float)D * vs^2) in place, the sign from the bit words; kNone -> +inf on set voxels / the caller's fill.
//   edt_thresh     D -> bit words: one lane per voxel, a wave's ballot is two words, stored by its first lane.
// No atomics: every output has one writer.
#include "vp_internal.h"

namespace vp {

namespace {

constexpr uint32_t kNone = VP_EDT_NONE;
constexpr uint32_t kFar = 0x7FFFFFFFu;          // "no seed on this side of the row" (a distance, not a squared one)

__global__ void __launch_bounds__(256)
edt_x(const uint32_t* __restrict__ seeds, uint32_t inv, uint32_t* __restrict__ dist, uint32_t n, uint32_t w, uint32_t rows, uint32_t RB)
{
    __shared__ uint32_t s_word[256];
    __shared__ int s_left[256], s_right[256];
    const uint32_t t = threadIdx.x, row0 = blockIdx.x * RB, nw = RB * w;     // nw <= 256
    const uint32_t r = t / w, xw = t - r * w;
    if (t < nw) s_word[t] = (row0 + r < rows) ? seeds[(size_t)(row0 + r) * w + xw] ^ inv : 0u;
    __syncthreads();
    if (t < nw) {
        const uint32_t* rw = s_word + r * w;
        int l = -1, rr = -1;
        for (int j = (int)xw - 1; j >= 0; --j) if (rw[j]) { l = j; break; }
        for (int j = (int)xw + 1; j < (int)w; ++j) if (rw[j]) { rr = j; break; }
        s_left[t] = l; s_right[t] = rr;
    }
    __syncthreads();
    const uint32_t total = RB * n;
    for (uint32_t i = t; i < total; i += 256) {
        const uint32_t ri = i / n, x = i - ri * n;
        if (row0 + ri >= rows) break;
        const uint32_t wi = ri * w + (x >> 5), b = x & 31u;
        const uint32_t wd = s_word[wi];
        uint32_t dl = kFar, dr = kFar;
        const uint32_t lo = wd & (0xFFFFFFFFu >> (31u - b));             // seed bits at or below b
        if (lo) dl = b - (31u - (uint32_t)__clz((int)lo));
        else if (s_left[wi] >= 0) {
            const uint32_t j = (uint32_t)s_left[wi];
            dl = x - (j * 32u + 31u - (uint32_t)__clz((int)s_word[ri * w + j]));
        }
        const uint32_t hi = wd & (0xFFFFFFFFu << b);                     // seed bits at or above b
        if (hi) dr = (uint32_t)(__ffs((int)hi) - 1) - b;
        else if (s_right[wi] >= 0) {
            const uint32_t j = (uint32_t)s_right[wi];
            dr = j * 32u + (uint32_t)(__ffs((int)s_word[ri * w + j]) - 1) - x;
        }
        const uint32_t d = dl < dr ? dl : dr;
        dist[(size_t)row0 * n + i] = d == kFar ? kNone : d * d;
    }
}

// out(i) of one column: `at(j)` reads entry j.  Candidates at distance d on both sides while d^2 < best.
template <class At>
__device__ __forceinline__ uint32_t column_min(At at, int i, int n)
{
    uint32_t best = at(i);
    for (int d = 1; ; ++d) {
        const uint32_t dd = (uint32_t)(d * d);
        const int lo = i - d, hi = i + d;
        if (dd >= best || (lo < 0 && hi >= n)) break;
        if (lo >= 0) { const uint32_t v = at(lo); if (v != kNone && v + dd < best) best = v + dd; }
        if (hi < n) { const uint32_t v = at(hi); if (v != kNone && v + dd < best) best = v + dd; }
    }
    return best;
}

// One thread per voxel.  axis = 1: columns along y (stride n), 2: along z (stride n^2).
__global__ void __launch_bounds__(256)
edt_col_naive(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, int axis, size_t nvox)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nvox) return;
    const size_t stride = axis == 1 ? (size_t)n : (size_t)n * n;
    const int i = (int)((idx / stride) % n);
    const uint32_t* col = in + (idx - (size_t)i * stride);
    out[idx] = column_min([&](int j) { return col[(size_t)j * stride]; }, i, (int)n);
}

// Workgroup (blockIdx.x, blockIdx.y) = the columns of the BX voxels from x = blockIdx.x * BX of the row / plane blockIdx.y:
// entry j of the column of x at dist[blockIdx.y * strideO + j * strideJ + x] (y pass: strideJ = n, strideO = n^2; z pass: n^2 and n).
template <int BX>
__global__ void __launch_bounds__(256)
edt_col_tiled(uint32_t* __restrict__ dist, uint32_t n, size_t strideJ, size_t strideO)
{
    extern __shared__ uint32_t s_col[];                              // n rows of BX entries
    constexpr uint32_t Q = BX / 4;                                     // 16-byte loads per row
    uint32_t* base = dist + (size_t)blockIdx.y * strideO + (size_t)blockIdx.x * BX;
    const uint32_t q = threadIdx.x % Q;
    int any = 0;
    for (uint32_t j = threadIdx.x / Q; j < n; j += 256 / Q) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + (size_t)j * strideJ + q * 4);
        *reinterpret_cast<uint4*>(s_col + j * BX + q * 4) = v;
        any |= (v.x & v.y & v.z & v.w) != kNone;
    }
    if (!__syncthreads_or(any)) return;                               // no seed in the whole bundle: it stays kNone
    const uint32_t xx = threadIdx.x % BX;
    for (uint32_t i = threadIdx.x / BX; i < n; i += 256 / BX) {
        const uint32_t best = column_min([&](int j) { return s_col[(uint32_t)j * BX + xx]; }, (int)i, (int)n);
        if (best != s_col[i * BX + xx]) base[(size_t)i * strideJ + xx] = best;
    }
}

__global__ void __launch_bounds__(256)
edt_to_sdf(uint32_t* dist, const uint32_t* __restrict__ words, float vs2, float fill, size_t total4)
{
    const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i4 >= total4) return;
    const size_t v = i4 * 4;
    const uint32_t bits = (words[v >> 5] >> (v & 31)) & 0xFu;
    const uint4 d4 = reinterpret_cast<const uint4*>(dist)[i4];
    const uint32_t d[4] = {d4.x, d4.y, d4.z, d4.w};
    float o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float init = ((bits >> b) & 1u) ? INFINITY : fill;
        o[b] = d[b] == kNone ? init : copysignf((float)d[b] * vs2, init);
    }
    reinterpret_cast<float4*>(dist)[i4] = make_float4(o[0], o[1], o[2], o[3]);
}

// bit = D <= r2 (greater == 0) or D > r2; the voxel count is a multiple of 256, so every wave is whole
__global__ void __launch_bounds__(256)
edt_thresh(const uint32_t* __restrict__ dist, uint32_t* __restrict__ out, uint32_t r2, int greater)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = dist[idx];
    const unsigned long long m = __ballot(greater ? v > r2 : v <= r2);
    if ((threadIdx.x & 63u) == 0u) reinterpret_cast<uint2*>(out)[idx >> 6] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
}

int column_pass(vp_ctx* ctx, uint32_t n, uint32_t* d_dist, int axis)
{
    const size_t sJ = axis == 1 ? (size_t)n : (size_t)n * n, sO = axis == 1 ? (size_t)n * n : (size_t)n;
    ProfScope p(ctx, axis == 1 ? VP_K_EDT_Y : VP_K_EDT_Z);
    if (n <= 512) hipLaunchKernelGGL((edt_col_tiled<32>), dim3(n / 32, n), dim3(256), (size_t)n * 32 * 4, ctx->stream, d_dist, n, sJ, sO);
    else {
        // 64 KiB of dynamic LDS at n = 1024: the whole default allowance
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&edt_col_tiled<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        hipLaunchKernelGGL((edt_col_tiled<16>), dim3(n / 16, n), dim3(256), (size_t)n * 16 * 4, ctx->stream, d_dist, n, sJ, sO);
    }
    VP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_edt(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, int seeds, uint32_t* d_dist, int algo)
{
    const uint32_t n = f.n, w = f.w;
    const size_t nvox = (size_t)n * n * n;
    uint32_t* vol2 = nullptr;
    if (algo == VP_ALGO_NAIVE) {
        VP_TRY(reserve(ctx, ctx->edt.vol2, nvox * 4, false));
        vol2 = (uint32_t*)ctx->edt.vol2.ptr;
    }
    const uint32_t* sw = d_words;
    if (seeds == VP_EDT_SEEDS_BORDER) {
        VP_TRY(reserve(ctx, ctx->edt.mask, nvox / 8, false));
        VP_TRY(launch_jfa_init(ctx, f, d_words, nullptr, nullptr, nullptr, (uint32_t*)ctx->edt.mask.ptr));
        sw = (const uint32_t*)ctx->edt.mask.ptr;
    }
    {
        const uint32_t rows = n * n, RB = 256u / w;
        ProfScope p(ctx, VP_K_EDT_X);
        hipLaunchKernelGGL(edt_x, dim3((rows + RB - 1) / RB), dim3(256), 0, ctx->stream, sw, seeds == VP_EDT_SEEDS_UNSET ? ~0u : 0u, d_dist, n, w,
                           rows, RB);
        VP_HIP(hipGetLastError());
    }
    if (algo == VP_ALGO_NAIVE) {
        const unsigned blocks = (unsigned)(nvox / 256);
        {
            ProfScope p(ctx, VP_K_EDT_Y_NAIVE);
            hipLaunchKernelGGL(edt_col_naive, dim3(blocks), dim3(256), 0, ctx->stream, (const uint32_t*)d_dist, vol2, n, 1, nvox);
            VP_HIP(hipGetLastError());
        }
        ProfScope p(ctx, VP_K_EDT_Z_NAIVE);
        hipLaunchKernelGGL(edt_col_naive, dim3(blocks), dim3(256), 0, ctx->stream, (const uint32_t*)vol2, d_dist, n, 2, nvox);
        VP_HIP(hipGetLastError());
        return 0;
    }
    VP_TRY(column_pass(ctx, n, d_dist, 1));
    return column_pass(ctx, n, d_dist, 2);
}

int launch_edt_thresh(vp_ctx* ctx, uint32_t n, const uint32_t* d_dist, uint32_t* d_out, uint32_t r2, int greater)
{
    ProfScope p(ctx, VP_K_EDT_THRESH);
    hipLaunchKernelGGL(edt_thresh, dim3((unsigned)((size_t)n * n * n / 256)), dim3(256), 0, ctx->stream, d_dist, d_out, r2, greater);
    VP_HIP(hipGetLastError());
    return 0;
}

int launch_edt_sdf(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, float fill, float* d_sdf, int algo)
{
    VP_TRY(launch_edt(ctx, f, d_words, VP_EDT_SEEDS_BORDER, reinterpret_cast<uint32_t*>(d_sdf), algo));
    const float vs2 = f.vs * f.vs;
    const size_t total4 = (size_t)f.n * f.n * f.n / 4;
    ProfScope p(ctx, VP_K_EDT_SDF);
    hipLaunchKernelGGL(edt_to_sdf, dim3((unsigned)(total4 / 256)), dim3(256), 0, ctx->stream, reinterpret_cast<uint32_t*>(d_sdf), d_words, vs2, fill,
                       total4);
    VP_HIP(hipGetLastError());
    return 0;
}

int launch_edt_morph(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo)
{
    const size_t nvox = (size_t)f.n * f.n * f.n, bytes = nvox / 8;
    if (radius == 0) return launch_stream_copy(ctx, d_out, d_words, bytes);
    const bool two = op == VP_MORPH_OPEN || op == VP_MORPH_CLOSE;
    VP_TRY(reserve(ctx, ctx->edt.vol, nvox * 4, false));
    if (algo == VP_ALGO_NAIVE) VP_TRY(reserve(ctx, ctx->edt.vol2, nvox * 4, false));
    if (two) VP_TRY(reserve(ctx, ctx->edt.tmp, bytes, false));
    uint32_t* vol = (uint32_t*)ctx->edt.vol.ptr;
    const uint32_t r2 = radius * radius;                             // radius <= 65535
    auto one = [&](const uint32_t* in, uint32_t* out, bool erode) -> int {
        VP_TRY(launch_edt(ctx, f, in, erode ? VP_EDT_SEEDS_UNSET : VP_EDT_SEEDS_SET, vol, algo));
        ProfScope p(ctx, VP_K_EDT_THRESH);
        hipLaunchKernelGGL(edt_thresh, dim3((unsigned)(nvox / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)vol, out, r2, erode ? 1 : 0);
        VP_HIP(hipGetLastError());
        return 0;
    };
    if (!two) return one(d_words, d_out, op == VP_MORPH_ERODE);
    uint32_t* tmp = (uint32_t*)ctx->edt.tmp.ptr;
    VP_TRY(one(d_words, tmp, op == VP_MORPH_OPEN));                  // open = dilate(erode), close = erode(dilate)
    return one(tmp, d_out, op == VP_MORPH_CLOSE);
}

}  // namespace vp
