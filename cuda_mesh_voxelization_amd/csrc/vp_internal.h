// vp_internal.h -- shared declarations of libvphip.so (not part of the public ABI): the context, whose state is one small struct per
// feature (each names its device buffers once), the error macros and the stage launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/vphip.h"

namespace vp {

// JFA state "no seed yet" of the two 32-bit id formats (jfa_common.h, IdU<9> / IdU<10>): y and z fields all ones, x = 2^BITS
constexpr uint32_t kNone9 = 0xFF9FF200u;    // n <= 512
constexpr uint32_t kNone10 = 0xFFDFFC00u;   // 512 < n <= 1024
constexpr int kTile = 8;                  // voxelizer tile: 8x8 (y,z) columns = one wave64
constexpr int kRecDwords = 20;            // per-triangle record, see vox.hip

// Device-side copy of vp_frame plus derived constants.
struct Frame {
    uint32_t n;        // voxels per side (global)
    uint32_t w;        // words per x-row = n / 32
    uint32_t z0, z1;   // slab
    float vs, ox, oy, oz;
};

inline Frame make_frame(const vp_frame* f)
{
    Frame r;
    r.n = f->n; r.w = f->n / 32; r.z0 = f->z0; r.z1 = f->z1;
    r.vs = f->voxel_size; r.ox = f->origin[0]; r.oy = f->origin[1]; r.oz = f->origin[2];
    return r;
}

int set_error(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define VP_HIP(call)                                                          \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) return vp::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

#define VP_TRY(call)                 \
    do {                             \
        int rc_ = (call);            \
        if (rc_ != 0) return rc_;    \
    } while (0)

struct ProfSpan { int kernel; hipEvent_t a, b; };

struct Buffer {
    void* ptr = nullptr;
    size_t bytes = 0;
};

// Pinned host words that device counts are copied back through: allocated by the first need(), used like the pointer, freed with the
// context.  The only place that allocates or frees pinned host memory.
template <typename T>
struct HostWords {
    T* p = nullptr;
    HostWords() = default;
    HostWords(const HostWords&) = delete;
    HostWords& operator=(const HostWords&) = delete;
    ~HostWords() { if (p) (void)hipHostFree(p); }
    int need(size_t count, bool zeroed = false)
    {
        if (p) return 0;
        VP_HIP(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault));
        if (zeroed) std::fill(p, p + count, T(0));
        return 0;
    }
    operator T*() const { return p; }
};

// What the state of one feature offers the context.  A feature names each of its device buffers ONCE, in VP_BUFFERS(released, ...) --
// freed by vp_ctx_release and by vp_ctx_destroy -- or VP_BUFFERS(kept, ...) -- freed by vp_ctx_destroy alone: the macro declares them
// and the member released(f) / kept(f) that enumerates them.  forget() puts the feature back into its "no result, no record" state
// (vp_ctx_release).  A new feature adds its struct to vp_ctx and its name to each_feature: nothing else frees, releases or resets it.
struct Feature {
    template <typename F> void released(F) {}
    template <typename F> void kept(F) {}
    void forget() {}
};
#define VP_BUFFERS(WHEN, ...) vp::Buffer __VA_ARGS__; template <typename F> void WHEN(F f) { vp::each(f, __VA_ARGS__); }
template <typename F, typename... B> void each(F& f, B&... b) { (f(b), ...); }
// the result of a feature that the context owns: n = the side of the grid it is for, 0: none
struct OwnedResult : Feature {
    uint32_t n = 0;
    void forget() { n = 0; }
};

}  // namespace vp

struct vp_ctx {
    using Buffer = vp::Buffer;
    int device = 0;
    int cus = 256;                             // compute units of the device (workgroup slots = cus x workgroups per CU)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // the tile-kernel launches of the most recent pass call (jfa_dense.hip, launch_tile; vp_jfa_last_shapes): a pass whose chains are
    // split makes two, so four is room enough; a host-side note, no device work
    vp_jfa_shape dense_shapes[4];
    int dense_shape_count = 0;
    // profiling
    bool prof_on = false;
    uint64_t prof_mask = ~0ull;                                    // timing keys that get events (vp_prof_select)
    std::vector<vp::ProfSpan> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[VP_K_ALL] = {};
    uint64_t prof_n[VP_K_ALL] = {};

    // vp_ctx_workspace: the slots
    struct Workspace : vp::Feature {
        Buffer slots[VP_WORKSPACE_SLOTS];
        template <typename F> void released(F f) { for (Buffer& b : slots) f(b); }
    } ws;
    // the job (triangle buffer, count, grid side, slab) whose large-triangle count last came back as ZERO: only that very job leaves the
    // list kernels out (a coarse mesh that follows a fine one on the same context must not be walked triangle by triangle)
    struct VoxJob { const void* tri = nullptr; size_t ntris = 0; uint32_t n = 0, z0 = 0, z1 = 0;
                    bool operator==(const VoxJob& o) const { return tri == o.tri && ntris == o.ntris && n == o.n && z0 == o.z0 && z1 == o.z1; } };
    // voxelizer (vox.hip): its grow-only workspaces; the work-queue size of an earlier call, copied back lazily (never waited for) to size
    // the next call's queue
    struct Vox : vp::Feature {
        VP_BUFFERS(kept, rec, tile_cnt, tile_off, tile_cur, pairs, scratch)
        vp::HostWords<uint32_t> total_host;
        hipEvent_t total_event = nullptr;
        bool total_pending = false;
        uint64_t total_seen = 0;
        uint64_t nbig_seen = 0;                // large triangles an earlier call counted (sizes the record list)
        bool counts_known = false;             // at least one such count has come back
        VoxJob pending_job, nolist_job;
    } vox;
    // conservative voxelizer (cvox.hip): its own large-triangle counter, record list and row scan, and its own lazily copied count
    struct Cvox : vp::Feature {
        VP_BUFFERS(kept, cnt, rec, base)
        vp::HostWords<uint32_t> host;
        hipEvent_t event = nullptr;
        bool pending = false;
        uint64_t nbig_seen = 0;
    } cvox;
    // interior fill (fill.hip): the ring of round flags (two batches) and its pinned host copy of one batch
    struct Fill : vp::Feature {
        VP_BUFFERS(kept, flags)
        vp::HostWords<uint32_t> host;
    } fill;
    // ball morphology (morph.hip): the row tables of every radius (uploaded by the first tiled call) and the intermediate grid of open / close
    struct Morph : vp::Feature {
        VP_BUFFERS(kept, tab, tmp)
    } morph;
    // connected components (components.hip): root counts per block of voxels and their scan; for vp_components_filter the label volume
    // (4 n^3 bytes, the one buffer vp_ctx_release frees), the sizes and keep flags of the K components, the arg-max winners and the kept
    // count; the pinned host words K and kept are read back through
    struct Comp : vp::Feature {
        VP_BUFFERS(released, labels)
        VP_BUFFERS(kept, cnt, off, sizes, keep, small)
        vp::HostWords<uint64_t> host;
    } comp;
    // surface nets (surfnets.hip): block counts of vertices and quads and their scans; the rank lookup -- NAIVE: the vertex-index volume,
    // 4 (n+1)^3 bytes; TILED: active-cell bits + one exclusive count per word, about n^3/4 bytes -- and the second position buffer of the
    // relaxation (rank and xyz are freed by vp_ctx_release); what the last vp_surfnets_count was for (words = nullptr: nothing)
    struct Sn : vp::Feature {
        VP_BUFFERS(released, rank, xyz)
        VP_BUFFERS(kept, cnt, off)
        const uint32_t* words = nullptr;
        uint32_t n = 0;
        int algo = 0;
        uint64_t vertices = 0, quads = 0;
        void forget() { words = nullptr; }
    } sn;
    // exact distance transform (edt.hip): the border mask of SEEDS_BORDER, the distance volume of vp_edt_morph, the second volume of the NAIVE
    // column passes (4 n^3 bytes each) and the intermediate grid of open / close; all four are freed by vp_ctx_release
    struct Edt : vp::Feature {
        VP_BUFFERS(released, mask, vol, vol2, tmp)
    } edt;
    // mesh distance (meshdist.hip): NAIVE's key volume (8 n^3 bytes), the triangle records and their row scan, the brick counts (+ write
    // cursors and plane sums) and offsets, the brick lists; the pinned host words the plane sums are read back through and the list
    // length of the last TILED call (vp_mesh_distance_stats); the six buffers are freed by vp_ctx_release
    struct Md : vp::Feature {
        VP_BUFFERS(released, keys, rec, base, cnt, off, list)
        vp::HostWords<uint64_t> host;
        uint64_t last_total = 0;
    } md;
    // iso-surface nets (isonets.hip): the inside grid of the field (n^3 / 8 bytes) and the mesh of the last vp_isonets, which the context
    // owns and vp_isonets_result hands out -- records, positions, normals (if asked for), quads; all five are freed by vp_ctx_release
    struct Iso : vp::Feature {
        VP_BUFFERS(released, words, cells, xyz, normals, quads)
        uint64_t vertices = 0, quad_count = 0;
        bool has_normals = false;
        void forget() { vertices = quad_count = 0; has_normals = false; }
    } iso;
    // generalized winding number (winding.hip): the result of the last vp_winding, which the context owns and vp_winding_result hands out
    // -- the field w (4 n^3 bytes) and its inside grid (n^3 / 8 bytes) -- the triangle records sorted by leaf (48 B each) and the pyramid
    // (counts, boxes, area sums, node records, leaf offsets, leaf keys); the pinned host word the inside count comes back through
    struct Wn : vp::OwnedResult {
        VP_BUFFERS(released, w, inside, rec, tree)
        vp::HostWords<uint64_t> host;
    } wn;
    // local thickness (thickness.hip): the result of the last vp_thickness, which the context owns and vp_thickness_result hands out -- T2
    // (4 n^3 bytes) and the thin grid (n^3 / 8 bytes) -- TILED's capped radii as uint16 (2 n^3 bytes), the grids of the saturated centres and
    // of the saturated region (n^3 / 8 bytes each) and the thin count with the per-brick summaries; the pinned host word the count comes
    // back through (the distance volumes are edt.vol / edt.vol2)
    struct Th : vp::OwnedResult {
        VP_BUFFERS(released, t2, thin, d16, sat, sum)
        vp::HostWords<uint64_t> host;
    } th;
    // sparse voxel octree (octree.hip): the nodes of the last vp_octree (8 bytes each, sized from the count), which the context owns and
    // vp_octree_result hands out; the device summary (level_offset | full_leaves | nodes per level), the state bytes and ranks of the levels
    // (NAIVE: all of them; TILED: those above the 32^3 blocks) and TILED's per-block counts and offsets; the pinned host words the summary
    // comes back through and its copy
    struct Oc : vp::OwnedResult {
        VP_BUFFERS(released, nodes, sum, state, rank, cnt)
        vp::HostWords<uint32_t> host;
        uint64_t count = 0;
        uint32_t level_offset[11] = {}, full_leaves[11] = {};
        void forget() { OwnedResult::forget(); count = 0; }
    } oc;
    // the grid of the last vp_octree_expand (n^3 / 8 bytes), which the context owns and vp_octree_expand_result hands out
    struct OcExpand : vp::OwnedResult {
        VP_BUFFERS(released, grid)
    } ocx;
    // topological thinning (skeleton.hip): the grid of the last vp_skeleton (n^3 / 8 bytes), which the context owns and vp_skeleton_result
    // hands out, and its three statistics; NAIVE's second grid, the border words of the current iteration (n^3 / 8 bytes each) and the
    // counters with TILED's block flags and list of active blocks (block_list.h); the pinned host words the counters come back through
    struct Sk : vp::OwnedResult {
        VP_BUFFERS(released, grid, tmp, border, aux)
        vp::HostWords<uint64_t> host;
        uint64_t stats[3] = {};
    } sk;
    // geodesic distance (geodesic.hip): D (4 n^3 bytes) and the reach grid (n^3 / 8 bytes) of the last vp_geodesic, which the context owns
    // and vp_geodesic_result hands out, and its four statistics; the counters with TILED's block flags and list of active blocks
    // (block_list.h) or NAIVE's ring of round flags; the pinned host words they come back through
    struct Gd : vp::OwnedResult {
        VP_BUFFERS(released, dist, reach, aux)
        vp::HostWords<uint64_t> host;
        uint64_t stats[4] = {};
    } gd;
    // seeded watershed (watershed.hip): W (4 n^3 bytes) and the cut grid (n^3 / 8 bytes) of the last vp_watershed, which the context owns and
    // vp_watershed_result hands out, and its four statistics; the key volume (8 n^3 bytes) and the counters with the presence bitmap of the
    // levels, the range of P per block and TILED's block flags and list (block_list.h) or NAIVE's ring of round flags; the pinned host
    // words they come back through
    struct Wsd : vp::OwnedResult {
        VP_BUFFERS(released, labels, cut, keys, aux)
        vp::HostWords<uint32_t> host;
        uint64_t stats[4] = {};
    } wsd;
    // region analysis (regions.hip): the table of the last vp_regions (26 x 8 bytes per label), which the context owns and
    // vp_regions_result hands out, its label count and four statistics; the four device totals and the pinned host words they come back through
    struct Rg : vp::OwnedResult {
        VP_BUFFERS(released, table, aux)
        vp::HostWords<uint64_t> host;
        uint32_t count = 0;
        uint64_t stats[4] = {};
        void forget() { OwnedResult::forget(); count = 0; }
    } rg;
    // grayscale reconstruction (reconstruct.hip): R (4 n^3 bytes) of the last vp_reconstruct, which the context owns and
    // vp_reconstruct_result hands out, and its four statistics; the counters with TILED's block flags and list of active blocks
    // (block_list.h) or NAIVE's ring of round flags; the pinned host words they come back through
    struct Rc : vp::OwnedResult {
        VP_BUFFERS(released, field, aux)
        vp::HostWords<uint64_t> host;
        uint64_t stats[4] = {};
    } rc;
    // h-extrema (reconstruct.hip): the scaled field V, the flattened field H (4 n^3 bytes each) and the grid E of the extended extrema
    // (n^3 / 8 bytes) of the last vp_extrema, which the context owns and vp_extrema_result hands out, and its four statistics; the field of
    // the second reconstruction (4 n^3 bytes of scratch) and counters, flags and host words of its own, like Rc's
    struct Ex : vp::OwnedResult {
        VP_BUFFERS(released, scaled, flat, extrema, tmp, aux)
        vp::HostWords<uint64_t> host;
        uint64_t stats[4] = {};
    } ex;
    // vp_extract_*: block counts / offsets of the last count call and what it was for (words = nullptr: nothing)
    struct Ext : vp::Feature {
        VP_BUFFERS(kept, cnt, off)
        const uint32_t* words = nullptr;
        int mode = -1;
        uint32_t n = 0;
        uint64_t total = 0;
        void forget() { words = nullptr; }
    } ext;
    // JFA: the row of "no seed" ids (jfa_seed.hip) and the workspace of vp_jfa* with d_work = NULL -- two id volumes + border mask, freed
    // by vp_ctx_release -- with the record of what the last vp_jfa_start left in its workspace, so that vp_jfa_run can refuse anything
    // else (a run on a workspace that holds init ids where it expects a border mask, or nothing at all, would produce an sdf from stale
    // memory)
    struct Jfa : vp::Feature {
        VP_BUFFERS(released, work)
        VP_BUFFERS(kept, none_row)
        struct Started {
            bool valid = false;
            bool mask = false;                     // border mask behind the two id volumes (fast sequence) / init ids in the first volume
            uint32_t n = 0;
            int algo = 0;
            const void* work = nullptr;
            size_t work_bytes = 0;
            const uint32_t* words = nullptr;
        } started;
        void forget() { started.valid = false; }
    } jfa;

    // f(feature) for every feature of the context: how vp_ctx_release and vp_ctx_destroy find every buffer
    template <typename F> void each_feature(F f)
    {
        f(ws); f(vox); f(cvox); f(fill); f(morph); f(comp); f(sn); f(edt); f(md); f(iso); f(wn); f(th); f(oc); f(ocx); f(sk); f(gd); f(wsd); f(rg); f(rc); f(ex); f(ext); f(jfa);
    }
};

namespace vp {

int reserve(vp_ctx* ctx, Buffer& b, size_t bytes, bool headroom = true);
void release(Buffer& b);

// RAII profiling bracket: the constructor records the start event on the stream, the destructor the end event (scope = the launches timed).
struct ProfScope {
    vp_ctx* ctx; int kernel; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(vp_ctx* c, int k);
    ~ProfScope();
};

// ---- id windows (include/vphip.h, vp_jfa_window_*) ----
// A buffer of `planes` id planes in the library's layout -- 4-byte ids (jfa_common.h: IdU<9> / IdU<10>) up to n = 1024; above that `planes`
// planes of 32-bit words followed by `planes` planes of bytes (IdC: 5 bytes per voxel).  `at` = index, inside the buffer, of plane z0 of
// the frame a call is made with.
struct IdWin {
    char* base = nullptr;
    uint32_t planes = 0, at = 0;
};
constexpr uint32_t kTileMinN = 96;   // VP_ALGO_TILED runs the tile kernels from this side on (n % 32 == 0: 96, 128, ...); the table kernel below it
                                     // (64 / 32: 0.063 / 0.061 ms per step against 0.117 / 0.102: launch-bound, profiles/r04/ab_tilemin.txt)
inline bool win_compact(uint32_t n) { return n > 1024; }
inline size_t win_plane_bytes(uint32_t n) { return (size_t)n * n * 4; }                     // of the (word) plane
inline size_t win_bytes(uint32_t n, uint32_t planes) { return (size_t)n * n * planes * (win_compact(n) ? 5 : 4); }
inline char* win_words(const IdWin& w, uint32_t n, int64_t plane)
{
    return reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(w.base) + (uintptr_t)(plane * (int64_t)win_plane_bytes(n)));
}
inline char* win_bytes_plane(const IdWin& w, uint32_t n, int64_t plane)
{
    return reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(w.base) + (uintptr_t)((int64_t)w.planes * (int64_t)win_plane_bytes(n) + plane * (int64_t)n * n));
}

// ---- stage launchers (each enqueues on ctx->stream) ----
int launch_voxelize(vp_ctx* ctx, const Frame& f, uint32_t* d_words, const float* d_xyz, size_t nverts,
                    const uint32_t* d_tri, size_t ntris, int algo, int accumulate);
// cvox.hip: conservative (26-separating) surface voxelization, OR into d_words (accumulate) or overwrite
int launch_voxelize_conservative(vp_ctx* ctx, const Frame& f, uint32_t* d_words, const float* d_xyz, size_t nverts,
                                 const uint32_t* d_tri, size_t ntris, int algo, int accumulate);
// fill.hip: interior fill of a whole grid, d_out = NOT exterior(d_words); blocking (reads the round flags back once per batch)
int launch_fill_interior(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_out, uint32_t* h_rounds);
// morph.hip: ball dilate / erode / open / close of a whole grid (enqueues only, once the context's buffers have grown)
int launch_morph(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo);
// edt.hip: exact squared distances to the seeds of a whole grid, the exact sdf and ball morphology through the transform (enqueue only, once
// the context's buffers have grown)
int launch_edt(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, int seeds, uint32_t* d_dist, int algo);
int launch_edt_sdf(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, float fill, float* d_sdf, int algo);
int launch_edt_morph(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo);
// the threshold pass of vp_edt_morph on its own: bit = D <= r2 (greater == 0) or D > r2, booked under VP_K_EDT_THRESH
int launch_edt_thresh(vp_ctx* ctx, uint32_t n, const uint32_t* d_dist, uint32_t* d_out, uint32_t r2, int greater);
// thickness.hip: local thickness of a whole grid -- T2 and the thin grid -- into the context's own buffers (enqueues only once they have
// grown, unless h_thin_count asks for the count)
int launch_thickness(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, uint32_t rmax, uint32_t thin2, int algo, uint64_t* h_thin_count);
// octree.hip: the sparse voxel octree of a whole grid into the context's own buffers (blocks once: the node count is read back), a tree back
// into a grid (enqueues only) and the structural check of a tree on the host
int launch_octree(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, int algo, uint64_t* h_nodes);
int launch_octree_expand(vp_ctx* ctx, const Frame& f, const uint32_t* d_nodes, uint64_t nodes, uint32_t* d_words, int algo);
int octree_validate(const uint32_t* h_nodes, uint64_t nodes, uint32_t n);
// skeleton.hip: topological thinning of a whole grid into the context's own grid (blocks: the deleted count of every iteration is read back),
// the table of the simple neighbourhoods on the device (2^21 words, enqueues only) and on the CPU
int launch_skeleton(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, const uint32_t* d_anchor, int mode, uint32_t max_iters, int algo,
                    uint64_t* h_stats);
int launch_skeleton_table(vp_ctx* ctx, int algo, uint32_t* d_table);
void skeleton_table_cpu(int algo, uint32_t* h_table);
// geodesic.hip: geodesic distances inside a mask from seed voxels and the reach grid, into the context's own buffers (blocks: the round
// flags or the length of the block list are read back)
int launch_geodesic(vp_ctx* ctx, const Frame& f, const uint32_t* d_mask, const uint32_t* d_seeds, int metric, int algo, uint64_t* h_stats);
// watershed.hip: seeded watershed / influence zones of a mask from a marker volume, labels and the cut grid into the context's own buffers
// (blocks: a pre-pass, then the round flags or the length of the block list per level, are read back); d_priority may be null
int launch_watershed(vp_ctx* ctx, const Frame& f, const uint32_t* d_mask, const uint32_t* d_markers, const uint32_t* d_priority, int order,
                     uint32_t quantum, int conn, int algo, uint64_t* h_stats);
// regions.hip: the per-label records of a label volume (volume, box, moments, faces, lattice points and edges, values) into the context's own
// table (blocks once: the four totals are read back); d_values may be null
int launch_regions(vp_ctx* ctx, const Frame& f, const uint32_t* d_labels, uint32_t count, const uint32_t* d_values, int algo, uint64_t* h_stats);
// reconstruct.hip: grayscale reconstruction of a marker field under a mask field, and the scaled field, the flattened field and the grid of
// the extended extrema of a value field, into the context's own buffers (block: the round flags or the length of the block list are
// read back); d_domain may be null
int launch_reconstruct(vp_ctx* ctx, const Frame& f, const uint32_t* d_domain, const uint32_t* d_marker, const uint32_t* d_mask, int mode, int conn,
                       int algo, uint64_t* h_stats);
int launch_extrema(vp_ctx* ctx, const Frame& f, const uint32_t* d_domain, const uint32_t* d_values, int kind, int scale, uint32_t h, int conn,
                   int algo, uint64_t* h_stats);
// meshdist.hip: narrow-band squared distance to the triangles of a mesh and the nearest face of a whole grid (TILED blocks once: it reads
// the list lengths back)
int launch_mesh_distance(vp_ctx* ctx, const Frame& f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris,
                         const uint32_t* d_sign, uint32_t band, float* d_dist, uint32_t* d_nearest, int algo);
// winding.hip: generalized winding number of a mesh at the centres of a whole grid and its inside grid, into the context's own buffers
// (enqueues only once they have grown, unless h_inside_count asks for the count)
int launch_winding(vp_ctx* ctx, const Frame& f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris, float beta, float level,
                   int algo, uint64_t* h_inside_count);
// components.hip: labels, sizes and size filters of the connected components of a whole grid; all three are blocking (counts go to the host)
int launch_components_label(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_labels, int conn, int algo, uint32_t* h_count);
int launch_components_sizes(vp_ctx* ctx, uint32_t n, const uint32_t* d_labels, uint32_t count, uint32_t* d_sizes);
int launch_components_filter(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, uint32_t* d_out, int conn, int mode, uint32_t param, int algo,
                             uint32_t* h_count, uint64_t* h_kept);
// surfnets.hip: count (blocking: V and Q go to the host) and write (vertices, quads, `iterations` relaxation steps; enqueues only, once the
// context's buffers have grown) of the surface-nets mesh of a whole grid
int launch_surfnets_count(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, int algo, uint64_t* h_vertices, uint64_t* h_quads);
// iso != nullptr: d_words is the inside grid of that field; launch_iso_place replaces the starting positions before the relaxation
struct IsoField { const float* d_field; int transform; float iso; float* d_normals; };
int launch_surfnets_write(vp_ctx* ctx, uint32_t n, const uint32_t* d_words, int algo, uint32_t iterations, uint64_t* d_cells, float* d_xyz,
                          uint32_t* d_quads, const IsoField* iso = nullptr);
// isonets.hip: surface nets of a scalar field at an iso level into the context's own buffers (blocking), and its placement pass
int launch_isonets(vp_ctx* ctx, uint32_t n, const float* d_field, int transform, float iso, uint32_t iterations, bool want_normals, int algo);
int launch_iso_place(vp_ctx* ctx, uint32_t n, int algo, const IsoField& iso, const uint64_t* d_cells, const uint32_t* index, float* d_xyz,
                     size_t nverts);
int launch_csg(vp_ctx* ctx, uint32_t* d_a, const uint32_t* d_b, size_t nwords, int op);
int launch_stream_copy(vp_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);   // 16 B per lane: the measured HBM copy rate
// jfa_seed.hip
size_t jfa_id_bytes(const Frame& f);                              // plain ids: 4 (n <= 1024) or 8 bytes
int launch_jfa_init(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, const uint32_t* below,
                    const uint32_t* above, void* d_ids, uint32_t* d_border_words);
int launch_jfa_pass(vp_ctx* ctx, const Frame& f, uint32_t k, const void* d_in, const void* d_minus,
                    const void* d_plus, void* d_out, int algo);
bool jfa_pass_can_fuse_final(const Frame& f, uint32_t k, int algo);
int launch_jfa_pass_ex(vp_ctx* ctx, const Frame& f, uint32_t k, const void* d_in, const void* d_minus,
                       const void* d_plus, void* d_out, int algo, const uint32_t* d_words, float fill, float* d_sdf);
int launch_jfa_final(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, const void* d_ids,
                     float fill, float* d_sdf);
bool jfa_can_start_from_mask(const Frame& f, int algo);         // n % 128 == 0: the pass k = n/2 straight from the border mask
bool jfa_can_fuse_first_two(const Frame& f, int algo);          // passes n/2 and n/4 in one launch from the border mask (whole grids)
int launch_win_init(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, const uint32_t* below, const uint32_t* above, const IdWin& out);
int launch_win_first_pass(vp_ctx* ctx, const Frame& f, const uint32_t* d_border, const IdWin& out);
int launch_win_clear(vp_ctx* ctx, uint32_t n, const IdWin& w);
// One pass with step k over the planes of f (tile kernel, jfa_dense.hip); the planes z -+ k of a plane z are found `stride` planes below /
// above it in the window (stride = k for a window of consecutive planes).  d_sdf != nullptr: the last pass, fused with the id -> sdf conversion.
int launch_win_pass(vp_ctx* ctx, const Frame& f, uint32_t k, const IdWin& in, const IdWin& out, uint32_t stride,
                    const uint32_t* d_words, float fill, float* d_sdf);
#define VP_DENSE_DECL(NAME) int NAME(vp_ctx* ctx, const Frame& f, uint32_t k, const IdWin& in, const IdWin& out, uint32_t stride, const uint32_t* d_words, float fill, float* d_sdf)
VP_DENSE_DECL(launch_dense_id9_pass);  VP_DENSE_DECL(launch_dense_id9_last);      // per id format; _last = fused with the id -> sdf conversion
VP_DENSE_DECL(launch_dense_id10_pass); VP_DENSE_DECL(launch_dense_id10_last);
VP_DENSE_DECL(launch_dense_idc_pass);  VP_DENSE_DECL(launch_dense_idc_last);
#undef VP_DENSE_DECL
// jfa_first_two.hip: passes n/2 and n/4 of a whole grid from its border mask into a window of n planes
// ranks > 1: the planes of rank `rank` of a cyclic distribution of the grid over `ranks` ranks into a window of n / ranks planes
int launch_win_first_two(vp_ctx* ctx, const Frame& f, const uint32_t* d_border, const IdWin& out, uint32_t ranks = 1, uint32_t rank = 0);
// ---- cyclic plane distribution (the first phase of the transposed multi-GPU pipeline; include/vphip.h, vp_jfa_window_*_cyclic) ----
// passes of the sequence n/2, n/4, ... that can run on planes dealt cyclically to `ranks` ranks (their steps are multiples of `ranks`): 0 or >= 2
uint32_t jfa_cyclic_passes(uint32_t n, uint32_t ranks);
// one pass with step k (a multiple of `ranks`) over the n / ranks planes of rank `rank`: jfa_dense.hip, jfa_pass_dense<CYC>
int launch_win_pass_cyclic(vp_ctx* ctx, const Frame& f, uint32_t k, const IdWin& in, const IdWin& out, uint32_t ranks, uint32_t rank);
#define VP_CYCLIC_DECL(NAME) int NAME(vp_ctx* ctx, const Frame& f, uint32_t k, const IdWin& in, const IdWin& out, uint32_t ranks, uint32_t rank)
VP_CYCLIC_DECL(launch_cyclic_id9_pass); VP_CYCLIC_DECL(launch_cyclic_id10_pass); VP_CYCLIC_DECL(launch_cyclic_idc_pass);
#undef VP_CYCLIC_DECL
// plane at + j * ranks + s of `out` := plane s * count + j of `in` (s < ranks, j < count): `ranks` chunks of `count` planes each, chunk s
// holding every ranks-th plane from s on, woven into consecutive planes (jfa_seed.hip)
int launch_win_interleave(vp_ctx* ctx, uint32_t n, const IdWin& in, const IdWin& out, uint32_t ranks, uint32_t count);
int launch_extract_count(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, int mode, uint64_t* h_count);
int launch_extract_write(vp_ctx* ctx, const Frame& f, const uint32_t* d_words, int mode, const float* d_sdf,
                         uint64_t* d_records, float* d_values, size_t capacity);

}  // namespace vp
