// morph.hip -- ball morphology of a whole-grid bit grid for gfx950 (MI355X): vp_morph (include/vphip.h).
//
// B_r = {(dx, dy, dz) in Z^3 : dx^2 + dy^2 + dz^2 <= r^2}.  dilate(W, r): voxel p is set iff some d in B_r has p - d in the grid and set
// (outside reads as empty).  erode(W, r) = NOT dilate(NOT W, r) (outside reads as set).  Erosion is the dilation kernel with the words
// complemented on load and on store: a word or a row outside the grid is 0 AFTER the complement, in both cases.
//
// The ball is a stack of x segments: the row offset (dy, dz) carries the half-width hw = isqrt(r^2 - dy^2 - dz^2), and the output row
// (y, z) is the OR over the disc dy^2 + dz^2 <= r^2 of the x-dilation by hw of row (y + dy, z + dz).
//   morph_naive   one thread per output word, from global memory: every row's three-word window (left, own, right) is x-dilated by its
//                 own hw (two 64-bit smears) and ORed in.  The plain form the tiled kernel is tested against.
//   morph_tiled   the x-dilations nest, so the rows are folded in by Horner from the widest down: acc = row(y, z); for hw = r-1 .. 0:
//                 acc = xdil1(acc) | OR of the rows whose half-width is hw.  r one-voxel dilations and one word OR per row, 32 voxels
//                 each.  A thread owns G consecutive words of a row (4 where n % 128 == 0, else 1) and carries G + 2 accumulators: the
//                 two outer words receive no carry from beyond, which is exact for r <= 32 -- the error enters at their far bit and
//                 moves one bit per step, so it has not reached the owned words when the last step reads their near bit.
//                 A workgroup owns a tile of T x T rows by XW words.  LDS form: tile plus r halo rows all around plus one word left
//                 and right, staged once (already complemented, 0 outside the grid); every row read is then an LDS read without a
//                 bounds test.  Where no tile with T >= 16 fits the LDS budget (the halo grows with r^2) the same body reads the rows
//                 from global memory instead -- through L1 / L2, where neighbouring lanes and tiles share them -- bounds-tested.
// The rows of the disc, sorted by half-width from r down, are a table per radius: built once on the host for r = 1 .. 32 and kept in a
// context buffer (36 k entries).  Every lane reads the same entry, so the walk over the table is scalar.
// No atomics: every output word has one writer.  Open and close are two launches through the context's intermediate grid.
#include "vp_internal.h"

#include <algorithm>
#include <vector>

namespace vp {

namespace {

constexpr uint32_t kMaxRadius = 32;
constexpr uint32_t kLdsBudgetWords = 16 * 1024;   // 64 KiB per workgroup: two workgroups per CU (160 KiB)

// table entry: dy + 64 in bits 0-7, dz + 64 in bits 8-15, half-width in bits 16-23
__host__ __device__ __forceinline__ int ent_dy(uint32_t e) { return (int)(e & 255u) - 64; }
__host__ __device__ __forceinline__ int ent_dz(uint32_t e) { return (int)((e >> 8) & 255u) - 64; }
__host__ __device__ __forceinline__ uint32_t ent_hw(uint32_t e) { return e >> 16; }

inline uint32_t isqrt_u32(uint32_t v)
{
    uint32_t s = 0;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// the tables of all radii, one after the other: start[r] .. start[r + 1]
struct Tables {
    std::vector<uint32_t> entries;
    uint32_t start[kMaxRadius + 2];
    Tables()
    {
        start[0] = start[1] = 0;
        for (uint32_t r = 1; r <= kMaxRadius; ++r) {
            const int R = (int)r;
            for (int hw = R; hw >= 0; --hw)
                for (int dz = -R; dz <= R; ++dz)
                    for (int dy = -R; dy <= R; ++dy) {
                        const int d2 = dy * dy + dz * dz;
                        if (d2 <= R * R && (int)isqrt_u32((uint32_t)(R * R - d2)) == hw)
                            entries.push_back((uint32_t)(dy + 64) | ((uint32_t)(dz + 64) << 8) | ((uint32_t)hw << 16));
                    }
            start[r + 1] = (uint32_t)entries.size();
        }
    }
};

const Tables& tables()
{
    static const Tables t;
    return t;
}

// OR of v << s for s = 0 .. h (h <= 32), by doubling
__device__ __forceinline__ uint64_t smear_up(uint64_t v, uint32_t h)
{
    uint32_t cover = 1;                       // v holds the shifts 0 .. cover - 1
    while (2 * cover <= h + 1) { v |= v << cover; cover *= 2; }
    return v | (v << (h + 1 - cover));
}
__device__ __forceinline__ uint64_t smear_down(uint64_t v, uint32_t h)
{
    uint32_t cover = 1;
    while (2 * cover <= h + 1) { v |= v >> cover; cover *= 2; }
    return v | (v >> (h + 1 - cover));
}

// One thread per output word.  inv = 0 (dilate) or ~0 (erode).
__global__ void __launch_bounds__(256)
morph_naive(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, uint32_t w, int r, uint32_t inv, size_t nwords)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nwords) return;
    const int xw = (int)(idx % w);
    const int y = (int)((idx / w) % n), z = (int)(idx / ((size_t)w * n));
    const int N = (int)n, W = (int)w;
    uint32_t acc = 0u;
    for (int dz = -r; dz <= r; ++dz) {
        const int zz = z + dz;
        if (zz < 0 || zz >= N) continue;
        for (int dy = -r; dy <= r; ++dy) {
            const int yy = y + dy;
            const int rest = r * r - dy * dy - dz * dz;
            if (rest < 0 || yy < 0 || yy >= N) continue;
            uint32_t hw = 0;
            while ((int)((hw + 1) * (hw + 1)) <= rest) ++hw;
            const uint32_t* row = in + ((size_t)zz * n + (size_t)yy) * w;
            const uint32_t c = row[xw] ^ inv;
            const uint32_t l = xw > 0 ? row[xw - 1] ^ inv : 0u;
            const uint32_t rr = xw + 1 < W ? row[xw + 1] ^ inv : 0u;
            // toward higher x: the high word of (c : l) smeared up; toward lower x: the low word of (rr : c) smeared down
            acc |= (uint32_t)(smear_up(((uint64_t)c << 32) | l, hw) >> 32) | (uint32_t)smear_down(((uint64_t)rr << 32) | c, hw);
        }
    }
    out[idx] = acc ^ inv;
}

// Tile kernel (see the head of the file).  Workgroup (blockIdx.x, .y, .z) = tile of XW words x T rows x T planes; 256 lanes walk the
// tile's T * T * XW / G positions, x fastest.  LDS image: (T + 2 r)^2 rows of XW + 2 words, row (yy, zz) at (zz * (T + 2 r) + yy).
template <int G, bool LDS>
__global__ void __launch_bounds__(256)
morph_tiled(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, uint32_t w, int r, uint32_t inv,
            const uint32_t* __restrict__ tab, uint32_t ntab, uint32_t T, uint32_t XW)
{
    extern __shared__ uint32_t s_img[];
    const int N = (int)n, W = (int)w;
    const int x0 = (int)(blockIdx.x * XW), y0 = (int)(blockIdx.y * T), z0 = (int)(blockIdx.z * T);
    const int TH = (int)T + 2 * r, XP = (int)XW + 2;
    if (LDS) {
        const uint32_t rows = (uint32_t)(TH * TH);
        auto stage = [&](uint32_t row, int yy, int zz, uint32_t xx) {
            const int gx = x0 - 1 + (int)xx, gy = y0 - r + yy, gz = z0 - r + zz;
            uint32_t v = 0u;
            if (gx >= 0 && gx < W && gy >= 0 && gy < N && gz >= 0 && gz < N) v = in[((size_t)gz * n + (size_t)gy) * w + (size_t)gx] ^ inv;
            s_img[row * (uint32_t)XP + xx] = v;
        };
        if (XP <= 32) {
            // 16 or 32 lanes per row (the first XP of them load), 16 or 8 rows per step; (yy, zz) advance without a division
            const uint32_t shift = XP <= 16 ? 4u : 5u;
            const uint32_t xx = threadIdx.x & ((1u << shift) - 1u), step = 256u >> shift;
            uint32_t row = threadIdx.x >> shift;
            int zz = (int)(row / (uint32_t)TH), yy = (int)(row % (uint32_t)TH);
            for (; row < rows; row += step) {
                if (xx < (uint32_t)XP) stage(row, yy, zz, xx);
                yy += (int)step;
                while (yy >= TH) { yy -= TH; ++zz; }
            }
        } else {
            for (uint32_t i = threadIdx.x; i < rows * (uint32_t)XP; i += 256) {
                const uint32_t row = i / (uint32_t)XP;
                stage(row, (int)(row % (uint32_t)TH), (int)(row / (uint32_t)TH), i - row * (uint32_t)XP);
            }
        }
        __syncthreads();
    }
    const uint32_t XG = XW / G;
    const uint32_t positions = XG * T * T;
    const uint32_t xgs = XG >= 4 ? 2u : XG >> 1;
    for (uint32_t p = threadIdx.x; p < positions; p += 256) {
        const uint32_t rowp = G == 4 ? p >> xgs : p / XG;                 // G == 4: XG is 1, 2 or 4 (XW = 4, 8 or 16)
        const uint32_t xg = p - rowp * XG, tz = rowp / T, ty = rowp - tz * T;
        const int xw = x0 + (int)(xg * G), y = y0 + (int)ty, z = z0 + (int)tz;
        if (xw >= W || y >= N || z >= N) continue;
        uint32_t a[G + 2];
#pragma unroll
        for (int j = 0; j < G + 2; ++j) a[j] = 0u;
        const uint32_t* sp = s_img + ((int)(tz + r) * TH + (int)(ty + r)) * XP + (int)(xg * G);
        int level = r;
        for (uint32_t i = 0; i < ntab; ++i) {
            const uint32_t e = tab[i];
            const int dy = ent_dy(e), dz = ent_dz(e), hw = (int)ent_hw(e);
            while (level > hw) {
                uint32_t b[G + 2];
#pragma unroll
                for (int j = 0; j < G + 2; ++j) {
                    b[j] = a[j] | (a[j] << 1) | (a[j] >> 1);
                    if (j > 0) b[j] |= a[j - 1] >> 31;
                    if (j < G + 1) b[j] |= a[j + 1] << 31;
                }
#pragma unroll
                for (int j = 0; j < G + 2; ++j) a[j] = b[j];
                --level;
            }
            if (LDS) {
                const uint32_t* q = sp + (dz * TH + dy) * XP;
#pragma unroll
                for (int j = 0; j < G + 2; ++j) a[j] |= q[j];
            } else {
                const int yy = y + dy, zz = z + dz;
                if (yy >= 0 && yy < N && zz >= 0 && zz < N) {
                    const uint32_t* q = in + ((size_t)zz * n + (size_t)yy) * w + xw;
                    if (xw > 0) a[0] |= q[-1] ^ inv;
#pragma unroll
                    for (int j = 0; j < G; ++j) a[j + 1] |= q[j] ^ inv;          // xw + G <= w: w % G == 0
                    if (xw + G < W) a[G + 1] |= q[G] ^ inv;
                }
            }
        }
        // the last row of the table has half-width 0, so level is 0 here
        uint32_t* o = out + ((size_t)z * n + (size_t)y) * w + xw;
#pragma unroll
        for (int j = 0; j < G; ++j) o[j] = a[j + 1] ^ inv;
    }
}

struct TileShape { uint32_t T, XW; bool lds; };

// Tile shape per radius: of the candidates that fit the LDS budget, the one with the smallest halo factor
// ((T + 2 r) / T)^2 (XW + 2) / XW; none with T >= 16 fits: rows through L1 / L2 on a 16 x 16 x XW tile.
TileShape tile_shape(uint32_t w, uint32_t G, uint32_t r)
{
    // G == 4: XW is 16, 8 or 4 words (a power of two not above w; the last tile in x may be partial); G == 1: the whole row
    auto width = [&](uint32_t X) { if (G != 4) return w; while (X > w) X /= 2; return X; };
    TileShape best{16u, width(16u), false};
    double bestf = 0.0;
    static const uint32_t Ts[] = {32u, 24u, 16u};
    static const uint32_t Xs[] = {16u, 8u};
    for (uint32_t T : Ts)
        for (uint32_t X : Xs) {
            const uint32_t XW = width(X);
            const uint64_t words = (uint64_t)(T + 2 * r) * (T + 2 * r) * (XW + 2);
            if (words > kLdsBudgetWords) continue;
            const double f = (double)(T + 2 * r) * (T + 2 * r) / ((double)T * T) * (double)(XW + 2) / (double)XW;
            if (!best.lds || f < bestf) { best = TileShape{T, XW, true}; bestf = f; }
        }
    return best;
}

int one_pass(vp_ctx* ctx, uint32_t n, const uint32_t* d_in, uint32_t* d_out, bool erode, uint32_t r, int algo)
{
    hipStream_t st = ctx->stream;
    const uint32_t w = n / 32;
    const size_t nwords = (size_t)n * n * w;
    const uint32_t inv = erode ? ~0u : 0u;
    if (algo == VP_ALGO_NAIVE) {
        ProfScope p(ctx, VP_K_MORPH_NAIVE);
        hipLaunchKernelGGL(morph_naive, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, d_in, d_out, n, w, (int)r, inv, nwords);
    } else {
        const Tables& t = tables();
        const uint32_t* tab = (const uint32_t*)ctx->morph.tab.ptr + t.start[r];
        const uint32_t ntab = t.start[r + 1] - t.start[r];
        const uint32_t G = (w % 4 == 0) ? 4u : 1u;
        const TileShape s = tile_shape(w, G, r);
        const dim3 grid((w + s.XW - 1) / s.XW, (n + s.T - 1) / s.T, (n + s.T - 1) / s.T);
        const size_t lds = s.lds ? (size_t)(s.T + 2 * r) * (s.T + 2 * r) * (s.XW + 2) * sizeof(uint32_t) : 0;
        ProfScope p(ctx, VP_K_MORPH);
        if (G == 4) {
            if (s.lds) hipLaunchKernelGGL((morph_tiled<4, true>), grid, dim3(256), lds, st, d_in, d_out, n, w, (int)r, inv, tab, ntab, s.T, s.XW);
            else hipLaunchKernelGGL((morph_tiled<4, false>), grid, dim3(256), 0, st, d_in, d_out, n, w, (int)r, inv, tab, ntab, s.T, s.XW);
        } else {
            if (s.lds) hipLaunchKernelGGL((morph_tiled<1, true>), grid, dim3(256), lds, st, d_in, d_out, n, w, (int)r, inv, tab, ntab, s.T, s.XW);
            else hipLaunchKernelGGL((morph_tiled<1, false>), grid, dim3(256), 0, st, d_in, d_out, n, w, (int)r, inv, tab, ntab, s.T, s.XW);
        }
    }
    VP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_morph(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo)
{
    const size_t bytes = (size_t)n * n * n / 8;
    if (radius == 0) return launch_stream_copy(ctx, d_out, d_words, bytes);
    if (algo == VP_ALGO_TILED && !ctx->morph.tab.ptr) {
        // first tiled call on this context: the row tables of every radius (the only synchronising step besides growing morph_tmp)
        const Tables& t = tables();
        VP_TRY(reserve(ctx, ctx->morph.tab, t.entries.size() * sizeof(uint32_t), false));
        VP_HIP(hipMemcpy(ctx->morph.tab.ptr, t.entries.data(), t.entries.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (op == VP_MORPH_DILATE || op == VP_MORPH_ERODE) return one_pass(ctx, n, d_words, d_out, op == VP_MORPH_ERODE, radius, algo);
    VP_TRY(reserve(ctx, ctx->morph.tmp, bytes, false));
    uint32_t* tmp = (uint32_t*)ctx->morph.tmp.ptr;
    VP_TRY(one_pass(ctx, n, d_words, tmp, op == VP_MORPH_OPEN, radius, algo));      // open = dilate(erode), close = erode(dilate)
    return one_pass(ctx, n, tmp, d_out, op == VP_MORPH_CLOSE, radius, algo);
}

}  // namespace vp
