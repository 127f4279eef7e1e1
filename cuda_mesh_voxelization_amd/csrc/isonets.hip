// isonets.hip -- surface nets of a scalar field at an iso level (include/vphip.h, vp_isonets*).  The topology is that
// of surfnets.hip, run on the INSIDE grid of the field: this file classifies the field into that grid, then places the vertices by the
// field's edge crossings and takes the normals from its gradient.  Count, records, quads and relaxation are the launches of surfnets.hip.
//
//   VP_ALGO_TILED  iso_classify: a wave streams 512 consecutive voxels, eight independent loads per lane, one ballot per load = 64
//                  consecutive inside bits, written by the lane that has the load's number.  iso_place: one lane per vertex, in record
//                  order; it decodes the record, gathers the eight corner values and recomputes h (no n^3 float volume is kept).
//   VP_ALGO_NAIVE  iso_classify_naive: one thread per word, 32 voxels one by one.  iso_place_naive: one thread per CELL finds its vertex in
//                  the index volume of the NAIVE path, reads its eight field values and takes the inside bits from them, not from the record.
// Both place kernels walk the twelve edges through the same device function: every operation in it is one IEEE operation of the contract.
#include "vp_internal.h"

namespace vp {

namespace {

constexpr int kBlock = 256;
constexpr int kLoads = 8;                           // independent loads per lane of iso_classify
constexpr uint32_t kNoVertex = 0xFFFFFFFFu;

struct Field {
    const float* v;
    uint32_t n;
    int transform;
    float iso;
};

__device__ __forceinline__ float field_h(const Field& f, float v)
{
    const float g = f.transform == VP_ISO_SIGNED_SQUARE ? copysignf(sqrtf(fabsf(v)), v) : v;
    return g - f.iso;
}

// +0 .. +inf; -0, negatives and every NaN are outside
__device__ __forceinline__ bool is_inside(float h) { return __float_as_uint(h) <= 0x7F800000u; }

// h at the eight corners of cell (cx, cy, cz), each in -1 .. n-1; a voxel outside the grid has h = NaN
__device__ __forceinline__ void corner_values(const Field& f, int cx, int cy, int cz, float (&h)[8])
{
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int x = cx + (c & 1), y = cy + ((c >> 1) & 1), z = cz + (c >> 2);
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < (int)f.n && y < (int)f.n && z < (int)f.n;
        h[c] = in ? field_h(f, f.v[((size_t)z * f.n + y) * f.n + x]) : __uint_as_float(0x7FC00000u);
    }
}

// position (and normal, if asked for) of the vertex of cell (cx, cy, cz) with corner values h and inside bits mask (active: 3 .. 12 crossings)
__device__ __forceinline__ void place(const float (&h)[8], uint32_t mask, int cx, int cy, int cz, float* __restrict__ xyz,
                                      float* __restrict__ normals, size_t v)
{
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int m = 0;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if ((c >> axis) & 1) continue;
            const int d = c | (1 << axis);
            if ((((mask >> c) ^ (mask >> d)) & 1u) == 0u) continue;
            float t = h[c] / (h[c] - h[d]);
            if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
            ++m;
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a] += a == axis ? t : (float)((c >> a) & 1);
        }
    const int cell[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) xyz[3 * v + a] = ((float)cell[a] + 0.5f) + acc[a] / (float)m;
    if (normals) {
        const float g[3] = {((h[1] - h[0]) + (h[3] - h[2])) + ((h[5] - h[4]) + (h[7] - h[6])),
                            ((h[2] - h[0]) + (h[3] - h[1])) + ((h[6] - h[4]) + (h[7] - h[5])),
                            ((h[4] - h[0]) + (h[5] - h[1])) + ((h[6] - h[2]) + (h[7] - h[3]))};
        const float l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        const bool ok = l2 > 0.0f && l2 <= 3.402823466e38f;        // neither zero, NaN nor infinite
        const float l = sqrtf(l2);
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[3 * v + a] = ok ? (-g[a]) / l : 0.0f;
    }
}

// ---- classification: the field into its inside grid, n^3 / 32 words, x fastest (the grid layout of the library) ----------------------
__global__ void __launch_bounds__(kBlock)
iso_classify(Field f, size_t nvox, unsigned long long* __restrict__ words64)
{
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = (size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const size_t base = wave * (64 * kLoads);                     // nvox is a multiple of 64: a load is inside or outside as a whole
    float v[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
        const size_t at = base + (size_t)u * 64 + lane;
        v[u] = at < nvox ? f.v[at] : __uint_as_float(0x7FC00000u);
    }
    unsigned long long mine = 0ull;
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
        const unsigned long long b = __ballot(is_inside(field_h(f, v[u])));
        if (lane == (uint32_t)u) mine = b;
    }
    const size_t at = base + (size_t)lane * 64;
    if (lane < (uint32_t)kLoads && at < nvox) words64[at / 64] = mine;
}

__global__ void __launch_bounds__(kBlock)
iso_classify_naive(Field f, size_t nwords, uint32_t* __restrict__ words)
{
    const size_t w = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= nwords) return;
    uint32_t bits = 0u;
    for (int b = 0; b < 32; ++b) bits |= (is_inside(field_h(f, f.v[w * 32 + b])) ? 1u : 0u) << b;
    words[w] = bits;
}

// ---- placement ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
iso_place(Field f, const unsigned long long* __restrict__ cells, uint32_t nverts, float* __restrict__ xyz, float* __restrict__ normals)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nverts) return;
    const unsigned long long rec = cells[v];
    const uint32_t c = (uint32_t)(rec & ((1ull << 40) - 1ull)), mask = (uint32_t)(rec >> 40) & 255u, n1 = f.n + 1;
    const int cx = (int)(c % n1) - 1, cy = (int)((c / n1) % n1) - 1, cz = (int)(c / (n1 * n1)) - 1;
    float h[8];
    corner_values(f, cx, cy, cz, h);
    place(h, mask, cx, cy, cz, xyz, normals, v);
}

__global__ void __launch_bounds__(kBlock)
iso_place_naive(Field f, uint32_t ncells, const uint32_t* __restrict__ index, uint32_t nverts, float* __restrict__ xyz,
                float* __restrict__ normals)
{
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncells) return;
    const uint32_t v = index[c];
    if (v == kNoVertex || v >= nverts) return;
    const uint32_t n1 = f.n + 1;
    const int cx = (int)(c % n1) - 1, cy = (int)((c / n1) % n1) - 1, cz = (int)(c / (n1 * n1)) - 1;
    float h[8];
    corner_values(f, cx, cy, cz, h);
    uint32_t mask = 0u;
#pragma unroll
    for (int t = 0; t < 8; ++t) mask |= (is_inside(h[t]) ? 1u : 0u) << t;
    place(h, mask, cx, cy, cz, xyz, normals, v);
}

}  // namespace

// Called by launch_surfnets_write between its vertex pass and the relaxation: overwrites the starting positions in d_xyz with those of the
// field and writes the normals.  `index` is the vertex-index volume of the NAIVE path.
int launch_iso_place(vp_ctx* ctx, uint32_t n, int algo, const IsoField& iso, const uint64_t* d_cells, const uint32_t* index, float* d_xyz,
                     size_t nverts)
{
    const Field f{iso.d_field, n, iso.transform, iso.iso};
    ProfScope p(ctx, algo == VP_ALGO_NAIVE ? VP_K_SN_VERTS_NAIVE : VP_K_SN_VERTS);
    if (algo == VP_ALGO_NAIVE) {
        const size_t ncells = (size_t)(n + 1) * (n + 1) * (n + 1);
        hipLaunchKernelGGL(iso_place_naive, dim3((unsigned)((ncells + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, f, (uint32_t)ncells,
                           index, (uint32_t)nverts, d_xyz, iso.d_normals);
    } else {
        hipLaunchKernelGGL(iso_place, dim3((unsigned)((nverts + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, f,
                           (const unsigned long long*)d_cells, (uint32_t)nverts, d_xyz, iso.d_normals);
    }
    VP_HIP(hipGetLastError());
    return 0;
}

// The whole build into the context's own buffers (blocking: V and Q are read back by the count).  The caller has validated everything; from
// here on the previous result is gone, so a failure leaves V = Q = 0.
int launch_isonets(vp_ctx* ctx, uint32_t n, const float* d_field, int transform, float iso, uint32_t iterations, bool want_normals, int algo)
{
    const size_t nvox = (size_t)n * n * n;
    ctx->iso.vertices = ctx->iso.quad_count = 0;
    ctx->iso.has_normals = false;
    VP_TRY(reserve(ctx, ctx->iso.words, nvox / 8));
    const Field f{d_field, n, transform, iso};
    {
        ProfScope p(ctx, algo == VP_ALGO_NAIVE ? VP_K_SN_CELLS_NAIVE : VP_K_SN_CELLS);
        if (algo == VP_ALGO_NAIVE) {
            const size_t nwords = nvox / 32;
            hipLaunchKernelGGL(iso_classify_naive, dim3((unsigned)((nwords + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, f, nwords,
                               (uint32_t*)ctx->iso.words.ptr);
        } else {
            const size_t per_block = (size_t)64 * kLoads * (kBlock / 64);
            hipLaunchKernelGGL(iso_classify, dim3((unsigned)((nvox + per_block - 1) / per_block)), dim3(kBlock), 0, ctx->stream, f, nvox,
                               (unsigned long long*)ctx->iso.words.ptr);
        }
    }
    VP_HIP(hipGetLastError());
    const uint32_t* words = (const uint32_t*)ctx->iso.words.ptr;
    uint64_t nv = 0, nq = 0;
    const int rc = launch_surfnets_count(ctx, n, words, algo, &nv, &nq);
    ctx->sn.words = nullptr;                                      // the scratch now belongs to this build: no vp_surfnets may be served from it
    VP_TRY(rc);
    VP_TRY(reserve(ctx, ctx->iso.cells, nv ? nv * 8 : 8));
    VP_TRY(reserve(ctx, ctx->iso.xyz, nv ? nv * 12 : 8));
    if (want_normals) VP_TRY(reserve(ctx, ctx->iso.normals, nv ? nv * 12 : 8));
    VP_TRY(reserve(ctx, ctx->iso.quads, nq ? nq * 16 : 8));
    IsoField field{d_field, transform, iso, want_normals ? (float*)ctx->iso.normals.ptr : nullptr};
    VP_TRY(launch_surfnets_write(ctx, n, words, algo, iterations, (uint64_t*)ctx->iso.cells.ptr, (float*)ctx->iso.xyz.ptr,
                                 (uint32_t*)ctx->iso.quads.ptr, &field));
    ctx->iso.vertices = nv; ctx->iso.quad_count = nq; ctx->iso.has_normals = want_normals;
    return 0;
}

}  // namespace vp
