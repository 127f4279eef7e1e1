// capi.hip -- the extern "C" surface of libvphip.so (declared in include/vphip.h):
// context / stream / workspace management, argument validation, per-kernel hipEvent timing and
// the host-in/host-out conveniences that reproduce the reference's Compute() calling convention.
// The context's state is one struct per feature (vp_internal.h): vp_ctx_destroy and vp_ctx_release walk the features, and the calls
// that build a result the context owns share build_owned -- neither names a buffer.
#include "vp_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>

namespace vp {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what, const char* file, int line)
{
    // same information as the reference's gpuAssert line (vplib/src/debug_utils.h:43-50)
    snprintf(g_err, sizeof(g_err), "[%s:%d] HIP Assert: %s (%s)", file, line, hipGetErrorString(e), what);
    return (int)e;
}

void release(Buffer& b)
{
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr; b.bytes = 0;
}

int reserve(vp_ctx* ctx, Buffer& b, size_t bytes, bool headroom)
{
    if (bytes <= b.bytes) return 0;
    VP_HIP(hipStreamSynchronize(ctx->stream));
    if (b.ptr) VP_HIP(hipFree(b.ptr));
    b.ptr = nullptr; b.bytes = 0;
    const size_t want = headroom ? bytes + bytes / 4 : bytes;     // head-room: fewer regrows (not for the id volumes of the slab driver: GiBs)
    VP_HIP(hipMalloc(&b.ptr, want));
    b.bytes = want;
    return 0;
}

ProfScope::ProfScope(vp_ctx* c, int k) : ctx(c), kernel(k)
{
    if (!ctx->prof_on || !((ctx->prof_mask >> k) & 1u)) return;
    auto take = [&]() -> hipEvent_t {
        if (!ctx->prof_pool.empty()) { hipEvent_t e = ctx->prof_pool.back(); ctx->prof_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    };
    a = take(); b = take();
    if (a) (void)hipEventRecord(a, ctx->stream);
}

ProfScope::~ProfScope()
{
    if (!ctx->prof_on || !a || !b) return;
    (void)hipEventRecord(b, ctx->stream);
    ctx->prof_pending.push_back({kernel, a, b});
}

static int prof_fold(vp_ctx* ctx)
{
    if (ctx->prof_pending.empty()) return 0;
    VP_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& s : ctx->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            ctx->prof_ms[s.kernel] += ms;
            ctx->prof_n[s.kernel] += 1;
        }
        ctx->prof_pool.push_back(s.a);
        ctx->prof_pool.push_back(s.b);
    }
    ctx->prof_pending.clear();
    return 0;
}

static int check_frame(const vp_frame* f, const char* who, bool whole)
{
    if (!f) return set_error(VP_ERR_INVALID, "%s: null frame", who);
    if (f->n < 32 || f->n > 2048 || (f->n % 32) != 0)
        return set_error(VP_ERR_UNSUPPORTED, "%s: n=%u unsupported (need 32 <= n <= 2048, n %% 32 == 0)", who, f->n);
    if (!(f->z0 < f->z1) || f->z1 > f->n || (f->z0 % 8) != 0 || (f->z1 % 8) != 0)
        return set_error(VP_ERR_INVALID, "%s: bad slab [%u,%u) for n=%u (multiples of 8 required)", who, f->z0, f->z1, f->n);
    if (whole && !(f->z0 == 0 && f->z1 == f->n))
        return set_error(VP_ERR_INVALID, "%s: whole-grid frame required", who);
    if (!(f->voxel_size > 0.0f) || !std::isfinite(f->voxel_size))
        return set_error(VP_ERR_INVALID, "%s: voxel_size must be positive and finite", who);
    return 0;
}

// Work must land on the context's device even if the calling thread's current HIP device changed in between
// (the null stream in particular belongs to the CURRENT device).
static int bind_device(vp_ctx* ctx)
{
    VP_HIP(hipSetDevice(ctx->device));
    return 0;
}

// vp_extract must follow a vp_extract_count of the same grid CONTENTS; the record of that count is dropped as soon as the
// buffer it was taken from is written through this ABI or handed out again as a workspace slot.
// The same holds for the record of vp_jfa_start: its border mask (or init ids) was computed from the grid CONTENTS, so a write to
// that grid -- or to the workspace itself -- between start and run invalidates it ("same grid" in the header means same contents).
// The rule: ANY output of ANY call of this ABI that the caller addresses -- grids, id planes and windows, sdf and distance volumes, record
// and mesh arrays, an explicit JFA workspace -- is such a write; every entry point reports each of its outputs to grid_written before it
// launches (tests/test_ctx_records_gpu.py holds the table of writers against the entry points of the header).  "Before it launches" is
// before the checks of the launch functions themselves (vp_jfa_pass, vp_jfa_last_pass, vp_extract and the window calls can still be
// refused there): a record may be dropped by a call that then writes nothing, never kept by one that writes.
// Byte RANGES are compared: a write into the interior of the grid -- vp_voxelize / vp_csg on a slab frame, vp_memcpy_d2d
// into a sub-range -- invalidates the records like a write to its first byte does.
static bool overlaps(const void* a, size_t an, const void* b, size_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + (bn ? bn : 1) && b0 < a0 + (an ? an : 1);
}
static void grid_written(vp_ctx* ctx, const void* d_ptr, size_t bytes)
{
    if (!d_ptr) return;
    if (overlaps(d_ptr, bytes, ctx->ext.words, (size_t)ctx->ext.n * ctx->ext.n * ctx->ext.n / 8)) ctx->ext.words = nullptr;
    const vp_ctx::Jfa::Started& st = ctx->jfa.started;
    if (st.valid && (overlaps(d_ptr, bytes, st.words, (size_t)st.n * st.n * st.n / 8) || overlaps(d_ptr, bytes, st.work, st.work_bytes)))
        ctx->jfa.started.valid = false;
    if (overlaps(d_ptr, bytes, ctx->sn.words, (size_t)ctx->sn.n * ctx->sn.n * ctx->sn.n / 8)) ctx->sn.words = nullptr;
}

static const char* kNames[VP_K_ALL] = {
    "vox_setup", "vox_scan", "vox_scatter", "vox_tile", "vox_naive", "vox_fill",
    "csg_words", "jfa_init", "jfa_pass", "jfa_final", "surface", "jfa_first", "jfa_sparse", "jfa_dense", "jfa_last", "extract", "vox_zero", "jfa_redeal",
    "cvox_zero", "cvox_setup", "cvox_scan", "cvox_rows", "cvox_naive",
    "fill_x", "fill_y", "fill_z", "fill_final",
    "morph", "morph_naive",
    "comp_init", "comp_merge", "comp_init_naive", "comp_merge_naive", "comp_flatten", "comp_rank", "comp_relabel", "comp_sizes", "comp_select",
    "comp_write",
    "sn_cells", "sn_scan", "sn_verts", "sn_quads", "sn_relax", "sn_cells_naive", "sn_verts_naive", "sn_quads_naive", "sn_relax_naive",
    "edt_x", "edt_y", "edt_z", "edt_y_naive", "edt_z_naive", "edt_sdf", "edt_thresh",
    "md_setup", "md_scan", "md_count", "md_write", "md_brick", "md_fill", "md_prefill", "md_naive", "md_split"
};

}  // namespace vp

using namespace vp;

// The workspace slots of the host-in / host-out calls at the end of this file, and the round trip of those with one grid in and one result
// out (a template: it cannot stand inside extern "C"): the grid goes up into SLOT_GRID_A, call(d_words, d_out) is the device entry point,
// and its output -- a grid in SLOT_GRID_B or one 32-bit value per voxel in SLOT_SDF -- comes down.  The callers validate first: asking
// for a slot already drops the records of the grids that lay in it.
enum { SLOT_GRID_A = 0, SLOT_GRID_B = 1, SLOT_XYZ = 2, SLOT_TRI = 3, SLOT_SDF = 4, SLOT_NEAREST = 5 };

// a host array up into a slot
static int stage(vp_ctx* ctx, int slot, const void* h_src, size_t bytes, void** d_out)
{
    VP_TRY(vp_ctx_workspace(ctx, slot, bytes, d_out));
    return vp_upload(ctx, *d_out, h_src, bytes);
}

template <typename Call>
static int host_round_trip(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, void* h_out, int out_slot, Call call)
{
    void *din = nullptr, *dout = nullptr;
    const size_t wb = vp_grid_words(f) * 4, ob = out_slot == SLOT_SDF ? vp_grid_voxels(f) * 4 : wb;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_words, wb, &din));
    VP_TRY(vp_ctx_workspace(ctx, out_slot, ob, &dout));
    VP_TRY(call((const uint32_t*)din, dout));
    return vp_download(ctx, h_out, dout, ob);
}

// One path for the calls that build a result the context owns (vp_isonets, vp_winding, vp_thickness, vp_octree, vp_octree_expand,
// vp_skeleton, vp_geodesic, vp_watershed, vp_regions, vp_reconstruct, vp_extrema): `ft` is the feature that is built, `also` what the call writes besides that feature's buffers, launch() the
// work.  The inputs are read while every one of those buffers is written: an input that lies in one is refused (the last result has to be
// copied before it goes back in); `inputs` is empty for the calls that have never refused it.  The context's own buffers are outputs
// like any other: whatever was recorded about their bytes is gone -- about the bytes they hold now (a buffer that has to grow is freed
// first: a record left standing on it would be served on freed memory) and, after the launch, about the bytes they hold then.
template <typename Ft, typename Launch>
static int build_owned(vp_ctx* ctx, const char* who, Ft& ft, std::initializer_list<Buffer*> also,
                       std::initializer_list<std::pair<const void*, size_t>> inputs, Launch launch)
{
    auto all = [&](auto f) { ft.released(f); ft.kept(f); for (Buffer* b : also) f(*b); };
    int rc = 0;
    all([&](Buffer& b) {
        for (const auto& in : inputs)
            if (!rc && overlaps(in.first, in.second, b.ptr, b.bytes)) rc = set_error(VP_ERR_INVALID, "%s: a buffer of the context overlaps d_words", who);
    });
    VP_TRY(rc);
    auto written = [&](Buffer& b) { grid_written(ctx, b.ptr, b.bytes); };
    all(written);
    rc = launch();
    all(written);
    return rc;
}

extern "C" {

int vp_abi_version(void) { return VP_ABI_VERSION; }

const char* vp_last_error(void) { return g_err; }

int vp_device_count(int* out)
{
    if (!out) return set_error(VP_ERR_INVALID, "vp_device_count: null out");
    *out = 0;
    VP_HIP(hipGetDeviceCount(out));
    return 0;
}

int vp_ctx_create(int device, vp_ctx** out)
{
    if (!out) return set_error(VP_ERR_INVALID, "vp_ctx_create: null out");
    *out = nullptr;
    int count = 0;
    VP_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count)
        return set_error(VP_ERR_INVALID, "vp_ctx_create: device %d not present (%d visible)", device, count);
    VP_HIP(hipSetDevice(device));
    vp_ctx* c = new (std::nothrow) vp_ctx();
    if (!c) return set_error(VP_ERR_NOMEM, "vp_ctx_create: out of host memory");
    c->device = device;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) c->cus = v; }
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate", __FILE__, __LINE__); }
    c->stream = c->own_stream;
    *out = c;
    return 0;
}

int vp_ctx_destroy(vp_ctx* ctx)
{
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->each_feature([](auto& ft) { ft.released(release); ft.kept(release); });
    for (auto& s : ctx->prof_pending) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto e : ctx->prof_pool) (void)hipEventDestroy(e);
    if (ctx->vox.total_event) (void)hipEventDestroy(ctx->vox.total_event);
    if (ctx->cvox.event) (void)hipEventDestroy(ctx->cvox.event);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return 0;
}

int vp_ctx_set_stream(vp_ctx* ctx, void* hip_stream, int external)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_ctx_set_stream: null ctx");
    VP_TRY(bind_device(ctx));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = external ? (hipStream_t)hip_stream : ctx->own_stream;
    return 0;
}

int vp_ctx_sync(vp_ctx* ctx)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_ctx_sync: null ctx");
    VP_TRY(bind_device(ctx));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int vp_malloc(vp_ctx* ctx, size_t bytes, void** d_out)
{
    if (!ctx || !d_out) return set_error(VP_ERR_INVALID, "vp_malloc: null argument");
    VP_HIP(hipSetDevice(ctx->device));
    VP_HIP(hipMalloc(d_out, bytes ? bytes : 1));
    return 0;
}

int vp_free(vp_ctx* ctx, void* d_ptr)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_free: null ctx");
    VP_TRY(bind_device(ctx));
    // the whole allocation goes, not its first byte: a record may be about a range anywhere inside it
    void* base = nullptr;
    size_t size = 0;
    if (d_ptr && hipMemGetAddressRange(&base, &size, d_ptr) == hipSuccess && base == d_ptr && size) grid_written(ctx, d_ptr, size);
    else { (void)hipGetLastError(); grid_written(ctx, d_ptr, 1); }
    if (d_ptr) { VP_HIP(hipStreamSynchronize(ctx->stream)); VP_HIP(hipFree(d_ptr)); }
    return 0;
}

int vp_memcpy_d2d(vp_ctx* ctx, void* d_dst, const void* d_src, size_t bytes)
{
    if (!ctx || ((!d_dst || !d_src) && bytes)) return set_error(VP_ERR_INVALID, "vp_memcpy_d2d: null argument");
    VP_TRY(bind_device(ctx));
    grid_written(ctx, d_dst, bytes);
    if (bytes) VP_HIP(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int vp_ctx_workspace(vp_ctx* ctx, int slot, size_t bytes, void** d_out)
{
    if (!ctx || !d_out || slot < 0 || slot >= VP_WORKSPACE_SLOTS) return set_error(VP_ERR_INVALID, "vp_ctx_workspace: bad argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(reserve(ctx, ctx->ws.slots[slot], bytes ? bytes : 1));
    *d_out = ctx->ws.slots[slot].ptr;
    grid_written(ctx, *d_out, ctx->ws.slots[slot].bytes);             // whoever asks for the slot is about to fill it
    return 0;
}

int vp_ctx_release(vp_ctx* ctx)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_ctx_release: null ctx");
    VP_TRY(bind_device(ctx));
    VP_HIP(hipStreamSynchronize(ctx->stream));
    // every feature gives up the buffers it marks as released (vp_internal.h) and the result or record that lay in them
    ctx->each_feature([](auto& ft) { ft.released(release); ft.forget(); });
    return 0;
}

int vp_memset(vp_ctx* ctx, void* d_ptr, int byte_value, size_t bytes)
{
    if (!ctx || (!d_ptr && bytes)) return set_error(VP_ERR_INVALID, "vp_memset: null argument");
    VP_TRY(bind_device(ctx));
    grid_written(ctx, d_ptr, bytes);
    if (bytes) VP_HIP(hipMemsetAsync(d_ptr, byte_value, bytes, ctx->stream));
    return 0;
}

int vp_upload(vp_ctx* ctx, void* d_dst, const void* h_src, size_t bytes)
{
    if (!ctx || ((!d_dst || !h_src) && bytes)) return set_error(VP_ERR_INVALID, "vp_upload: null argument");
    VP_TRY(bind_device(ctx));
    grid_written(ctx, d_dst, bytes);
    if (bytes) {
        VP_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
        VP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int vp_download(vp_ctx* ctx, void* h_dst, const void* d_src, size_t bytes)
{
    if (!ctx || ((!h_dst || !d_src) && bytes)) return set_error(VP_ERR_INVALID, "vp_download: null argument");
    VP_TRY(bind_device(ctx));
    if (bytes) {
        VP_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        VP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

size_t vp_grid_words(const vp_frame* f) { return f ? (size_t)f->n * f->n * (f->z1 - f->z0) / 32 : 0; }
size_t vp_grid_voxels(const vp_frame* f) { return f ? (size_t)f->n * f->n * (f->z1 - f->z0) : 0; }

// Every grid / id / sdf buffer handed in must be 16-byte aligned (include/vphip.h): the kernels move them as 16-byte vectors.
static int check_aligned(const char* who, std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15u) return set_error(VP_ERR_INVALID, "%s: device buffer %p is not 16-byte aligned", who, p);
    return 0;
}

// The calls that serve whole grids only refuse a slab frame as unsupported (a frame that passed check_frame; check_frame's own `whole`
// refuses it as invalid: each entry point keeps the code it has always returned).
static int check_whole(const vp_frame* f, const char* who)
{
    if (f->z0 != 0 || f->z1 != f->n) return set_error(VP_ERR_UNSUPPORTED, "%s: slab frames are not served (whole grid only)", who);
    return 0;
}

static int check_algo(const char* who, int algo)
{
    if (algo != VP_ALGO_NAIVE && algo != VP_ALGO_TILED) return set_error(VP_ERR_INVALID, "%s: unknown algo %d", who, algo);
    return 0;
}

// What every call that serves whole grids up to n = 1024 checks first, in this order: the frame, the whole grid, the side -- `why` is what
// the refusal says in parentheses -- and, where the algo comes next, the algo.
static int check_grid_1024(const vp_frame* f, const char* who, const char* why = "32 <= n <= 1024")
{
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_whole(f, who));
    if (f->n > 1024) return set_error(VP_ERR_UNSUPPORTED, "%s: n=%u is not served (%s)", who, f->n, why);
    return 0;
}
static int check_grid_1024(const vp_frame* f, const char* who, int algo, const char* why = "32 <= n <= 1024")
{
    VP_TRY(check_grid_1024(f, who, why));
    return check_algo(who, algo);
}

static int check_morph_op(const char* who, int op)
{
    if (op != VP_MORPH_DILATE && op != VP_MORPH_ERODE && op != VP_MORPH_OPEN && op != VP_MORPH_CLOSE)
        return set_error(VP_ERR_INVALID, "%s: unknown op %d", who, op);
    return 0;
}

// an output that would be written while the input grid d_words is still being read
static int check_disjoint(const char* who, const char* out_name, const void* d_in, size_t in_bytes, const void* d_out, size_t out_bytes)
{
    if (overlaps(d_in, in_bytes, d_out, out_bytes)) return set_error(VP_ERR_INVALID, "%s: %s overlaps d_words", who, out_name);
    return 0;
}

// vp_voxelize and vp_voxelize_conservative: the same checks in front of two launchers
static int voxelize(const char* who, decltype(&launch_voxelize) launch, vp_ctx* ctx, const vp_frame* f, uint32_t* d_words, const float* d_xyz,
                    size_t nverts, const uint32_t* d_tri, size_t ntris, int algo, int accumulate)
{
    if (!ctx || !d_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_aligned(who, {d_words}));
    if (ntris && (!d_xyz || !d_tri || !nverts)) return set_error(VP_ERR_INVALID, "%s: null mesh arrays", who);
    VP_TRY(check_algo(who, algo));
    if (ntris > 0xFFFFFFFFull / 3) return set_error(VP_ERR_UNSUPPORTED, "%s: too many triangles", who);
    grid_written(ctx, d_words, vp_grid_words(f) * 4);
    return launch(ctx, make_frame(f), d_words, d_xyz, nverts, d_tri, ntris, algo, accumulate ? 1 : 0);
}

int vp_voxelize(vp_ctx* ctx, const vp_frame* f, uint32_t* d_words, const float* d_xyz, size_t nverts,
                const uint32_t* d_tri, size_t ntris, int algo, int accumulate)
{
    return voxelize("vp_voxelize", launch_voxelize, ctx, f, d_words, d_xyz, nverts, d_tri, ntris, algo, accumulate);
}

int vp_voxelize_conservative(vp_ctx* ctx, const vp_frame* f, uint32_t* d_words, const float* d_xyz, size_t nverts,
                             const uint32_t* d_tri, size_t ntris, int algo, int accumulate)
{
    return voxelize("vp_voxelize_conservative", launch_voxelize_conservative, ctx, f, d_words, d_xyz, nverts, d_tri, ntris, algo, accumulate);
}

int vp_fill_interior(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, uint32_t* h_rounds)
{
    const char* who = "vp_fill_interior";
    if (!ctx || !d_words || !d_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_whole(f, who));
    VP_TRY(check_aligned(who, {d_words, d_out}));
    const size_t bytes = vp_grid_words(f) * 4;
    VP_TRY(check_disjoint(who, "d_out", d_words, bytes, d_out, bytes));
    grid_written(ctx, d_out, bytes);
    return launch_fill_interior(ctx, f->n, d_words, d_out, h_rounds);
}

int vp_morph(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo)
{
    const char* who = "vp_morph";
    if (!ctx || !d_words || !d_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_whole(f, who));
    VP_TRY(check_morph_op(who, op));
    VP_TRY(check_algo(who, algo));
    if (radius > 32) return set_error(VP_ERR_UNSUPPORTED, "%s: radius %u is not served (0 .. 32)", who, radius);
    VP_TRY(check_aligned(who, {d_words, d_out}));
    const size_t bytes = vp_grid_words(f) * 4;
    VP_TRY(check_disjoint(who, "d_out", d_words, bytes, d_out, bytes));
    grid_written(ctx, d_out, bytes);
    return launch_morph(ctx, f->n, d_words, d_out, op, radius, algo);
}

static int check_fill(float fill, const char* who);

// what vp_edt, vp_edt_sdf and vp_edt_morph share: whole grids up to n = 1024, the algo
static int check_edt(const vp_frame* f, const char* who, int algo)
{
    return check_grid_1024(f, who, algo, "32 <= n <= 1024: the distance volume would be 32 GiB");
}

static int check_edt_seeds(const char* who, int seeds)
{
    if (seeds != VP_EDT_SEEDS_SET && seeds != VP_EDT_SEEDS_UNSET && seeds != VP_EDT_SEEDS_BORDER)
        return set_error(VP_ERR_INVALID, "%s: unknown seeds %d", who, seeds);
    return 0;
}

static int check_edt_morph(const char* who, int op, uint32_t radius)
{
    VP_TRY(check_morph_op(who, op));
    if (radius > 65535u) return set_error(VP_ERR_INVALID, "%s: radius %u (0 .. 65535)", who, radius);
    return 0;
}

int vp_edt(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int seeds, uint32_t* d_dist2, int algo)
{
    const char* who = "vp_edt";
    if (!ctx || !d_words || !d_dist2) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_edt(f, who, algo));
    VP_TRY(check_edt_seeds(who, seeds));
    VP_TRY(check_aligned(who, {d_words, d_dist2}));
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    VP_TRY(check_disjoint(who, "d_dist2", d_words, wb, d_dist2, vb));
    grid_written(ctx, d_dist2, vb);
    return launch_edt(ctx, make_frame(f), d_words, seeds, d_dist2, algo);
}

int vp_edt_sdf(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, float fill_unset, float* d_sdf, int algo)
{
    const char* who = "vp_edt_sdf";
    if (!ctx || !d_words || !d_sdf) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_edt(f, who, algo));
    VP_TRY(check_fill(fill_unset, who));
    VP_TRY(check_aligned(who, {d_words, d_sdf}));
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    VP_TRY(check_disjoint(who, "d_sdf", d_words, wb, d_sdf, vb));
    grid_written(ctx, d_sdf, vb);
    return launch_edt_sdf(ctx, make_frame(f), d_words, fill_unset, d_sdf, algo);
}

int vp_edt_morph(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo)
{
    const char* who = "vp_edt_morph";
    if (!ctx || !d_words || !d_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_edt(f, who, algo));
    VP_TRY(check_edt_morph(who, op, radius));
    VP_TRY(check_aligned(who, {d_words, d_out}));
    const size_t bytes = vp_grid_words(f) * 4;
    VP_TRY(check_disjoint(who, "d_out", d_words, bytes, d_out, bytes));
    grid_written(ctx, d_out, bytes);
    return launch_edt_morph(ctx, make_frame(f), d_words, d_out, op, radius, algo);
}

// what vp_mesh_distance and its host form share: whole grids up to n = 1024, the algo, the band
static int check_mesh_distance(const vp_frame* f, const char* who, uint32_t band, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (band < 1 || band > 32) return set_error(VP_ERR_INVALID, "%s: band %u (1 .. 32 voxels)", who, band);
    return 0;
}

int vp_mesh_distance(vp_ctx* ctx, const vp_frame* f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris,
                     const uint32_t* d_sign_words, uint32_t band, float* d_dist2, uint32_t* d_nearest, int algo)
{
    const char* who = "vp_mesh_distance";
    if (!ctx || !d_dist2) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_mesh_distance(f, who, band, algo));
    if (ntris && (!d_xyz || !d_tri || !nverts)) return set_error(VP_ERR_INVALID, "%s: null mesh arrays", who);
    if (ntris > 0xFFFFFFFFull / 3) return set_error(VP_ERR_UNSUPPORTED, "%s: too many triangles", who);
    VP_TRY(check_aligned(who, {d_xyz, d_tri, d_sign_words, d_dist2, d_nearest}));
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    for (const void* out : {(const void*)d_dist2, (const void*)d_nearest}) {
        if (overlaps(out, vb, d_xyz, nverts * 12) || overlaps(out, vb, d_tri, ntris * 12) || overlaps(out, vb, d_sign_words, wb))
            return set_error(VP_ERR_INVALID, "%s: an output overlaps an input", who);
    }
    if (overlaps(d_dist2, vb, d_nearest, vb)) return set_error(VP_ERR_INVALID, "%s: d_nearest overlaps d_dist2", who);
    grid_written(ctx, d_dist2, vb);
    grid_written(ctx, d_nearest, vb);
    return launch_mesh_distance(ctx, make_frame(f), d_xyz, nverts, d_tri, ntris, d_sign_words, band, d_dist2, d_nearest, algo);
}

int vp_mesh_distance_stats(vp_ctx* ctx, uint64_t* list_entries)
{
    if (!ctx || !list_entries) return set_error(VP_ERR_INVALID, "vp_mesh_distance_stats: null argument");
    *list_entries = ctx->md.last_total;
    return 0;
}

// what the three vp_components_* entry points share: whole grids up to n = 1024, connectivity and algo
static int check_components(const vp_frame* f, const char* who, int connectivity, int algo)
{
    VP_TRY(check_grid_1024(f, who, "32 <= n <= 1024: voxel indices are 32-bit"));
    if (connectivity != VP_CONN_6 && connectivity != VP_CONN_26) return set_error(VP_ERR_INVALID, "%s: unknown connectivity %d (6 or 26)", who, connectivity);
    VP_TRY(check_algo(who, algo));
    return 0;
}

static int check_filter_mode(const char* who, int mode, uint32_t param)
{
    if (mode != VP_COMP_KEEP_LARGEST && mode != VP_COMP_MIN_VOXELS) return set_error(VP_ERR_INVALID, "%s: unknown mode %d", who, mode);
    if (mode == VP_COMP_KEEP_LARGEST && (param < 1 || param > 16)) return set_error(VP_ERR_INVALID, "%s: KEEP_LARGEST m=%u outside 1 .. 16", who, param);
    return 0;
}

int vp_components_label(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_labels, int connectivity, int algo,
                        uint32_t* h_count)
{
    const char* who = "vp_components_label";
    if (!ctx || !d_words || !d_labels || !h_count) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_components(f, who, connectivity, algo));
    VP_TRY(check_aligned(who, {d_words, d_labels}));
    const size_t wb = vp_grid_words(f) * 4, lb = vp_grid_voxels(f) * 4;
    VP_TRY(check_disjoint(who, "d_labels", d_words, wb, d_labels, lb));
    grid_written(ctx, d_labels, lb);
    return launch_components_label(ctx, f->n, d_words, d_labels, connectivity, algo, h_count);
}

int vp_components_sizes(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_labels, uint32_t count, uint32_t* d_sizes)
{
    const char* who = "vp_components_sizes";
    if (!ctx || !d_labels || (!d_sizes && count)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_components(f, who, VP_CONN_6, VP_ALGO_TILED));
    VP_TRY(check_aligned(who, {d_labels, d_sizes}));
    if (count && overlaps(d_labels, vp_grid_voxels(f) * 4, d_sizes, (size_t)count * 4)) return set_error(VP_ERR_INVALID, "%s: d_sizes overlaps d_labels", who);
    if (count) grid_written(ctx, d_sizes, (size_t)count * 4);
    return launch_components_sizes(ctx, f->n, d_labels, count, d_sizes);
}

int vp_components_filter(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, int connectivity, int mode,
                         uint32_t param, int algo, uint32_t* h_count, uint64_t* h_kept)
{
    const char* who = "vp_components_filter";
    if (!ctx || !d_words || !d_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_components(f, who, connectivity, algo));
    VP_TRY(check_filter_mode(who, mode, param));
    VP_TRY(check_aligned(who, {d_words, d_out}));
    const size_t bytes = vp_grid_words(f) * 4;
    VP_TRY(check_disjoint(who, "d_out", d_words, bytes, d_out, bytes));
    grid_written(ctx, d_out, bytes);
    return launch_components_filter(ctx, f->n, d_words, d_out, connectivity, mode, param, algo, h_count, h_kept);
}

int vp_csg(vp_ctx* ctx, uint32_t* d_a, const uint32_t* d_b, size_t nwords, int op)
{
    if (!ctx || ((!d_a || !d_b) && nwords)) return set_error(VP_ERR_INVALID, "vp_csg: null argument");
    VP_TRY(bind_device(ctx));
    if (op < VP_OP_VOID || op > VP_OP_DIFFERENCE) return set_error(VP_ERR_INVALID, "vp_csg: unknown op %d", op);
    VP_TRY(check_aligned("vp_csg", {d_a, d_b}));
    grid_written(ctx, d_a, nwords * 4);
    return launch_csg(ctx, d_a, d_b, nwords, op);
}

int vp_stream_copy(vp_ctx* ctx, void* d_dst, const void* d_src, size_t bytes)
{
    if (!ctx || !d_dst || !d_src || bytes == 0 || (bytes % 16) != 0 || ((uintptr_t)d_dst % 16) != 0 || ((uintptr_t)d_src % 16) != 0)
        return set_error(VP_ERR_INVALID, "vp_stream_copy: 16-byte aligned buffers of a multiple of 16 bytes required");
    VP_TRY(bind_device(ctx));
    grid_written(ctx, d_dst, bytes);
    return launch_stream_copy(ctx, d_dst, d_src, bytes);
}

size_t vp_jfa_workspace_bytes(const vp_frame* f)
{
    // two id volumes + border mask
    return f ? 2 * vp_grid_voxels(f) * vp_jfa_id_bytes(f) + vp_grid_words(f) * 4 : 0;
}

size_t vp_jfa_id_bytes(const vp_frame* f) { return (f && f->n > 1024) ? 8 : 4; }

static int check_fill(float fill, const char* who)
{
    if (!std::isinf(fill)) return set_error(VP_ERR_INVALID, "%s: fill_unset must be +-infinity", who);
    return 0;
}

int vp_jfa_init(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const uint32_t* d_plane_below,
                const uint32_t* d_plane_above, void* d_ids)
{
    if (!ctx || !d_words || !d_ids) return set_error(VP_ERR_INVALID, "vp_jfa_init: null argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_jfa_init", false));
    VP_TRY(check_aligned("vp_jfa_init", {d_words, d_plane_below, d_plane_above, d_ids}));
    grid_written(ctx, d_ids, vp_grid_voxels(f) * vp_jfa_id_bytes(f));
    return launch_jfa_init(ctx, make_frame(f), d_words, d_plane_below, d_plane_above, d_ids, nullptr);
}

int vp_surface(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const uint32_t* d_plane_below,
               const uint32_t* d_plane_above, uint32_t* d_border_words)
{
    if (!ctx || !d_words || !d_border_words) return set_error(VP_ERR_INVALID, "vp_surface: null argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_surface", false));
    VP_TRY(check_aligned("vp_surface", {d_words, d_plane_below, d_plane_above, d_border_words}));
    grid_written(ctx, d_border_words, vp_grid_words(f) * 4);
    return launch_jfa_init(ctx, make_frame(f), d_words, d_plane_below, d_plane_above, nullptr, d_border_words);
}

int vp_jfa_pass(vp_ctx* ctx, const vp_frame* f, uint32_t k, const void* d_in, const void* d_minus,
                const void* d_plus, void* d_out, int algo)
{
    if (ctx) ctx->dense_shape_count = 0;
    if (!ctx || !d_in || !d_out || d_in == d_out) return set_error(VP_ERR_INVALID, "vp_jfa_pass: bad buffers");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_jfa_pass", false));
    VP_TRY(check_aligned("vp_jfa_pass", {d_in, d_minus, d_plus, d_out}));
    if (k == 0 || k >= f->n) return set_error(VP_ERR_INVALID, "vp_jfa_pass: step %u out of range", k);
    VP_TRY(check_algo("vp_jfa_pass", algo));
    // halos are mandatory wherever a neighbour plane exists outside the slab
    if (f->z0 > 0 && !d_minus) return set_error(VP_ERR_INVALID, "vp_jfa_pass: slab needs d_minus");
    if (f->z1 < f->n && !d_plus) return set_error(VP_ERR_INVALID, "vp_jfa_pass: slab needs d_plus");
    grid_written(ctx, d_out, vp_grid_voxels(f) * vp_jfa_id_bytes(f));
    return launch_jfa_pass(ctx, make_frame(f), k, d_in, d_minus, d_plus, d_out, algo);
}

int vp_jfa_finalize(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const void* d_ids,
                    float fill_unset, float* d_sdf)
{
    if (!ctx || !d_words || !d_ids || !d_sdf) return set_error(VP_ERR_INVALID, "vp_jfa_finalize: null argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_jfa_finalize", false));
    VP_TRY(check_fill(fill_unset, "vp_jfa_finalize"));
    grid_written(ctx, d_sdf, vp_grid_voxels(f) * 4);
    return launch_jfa_final(ctx, make_frame(f), d_words, d_ids, fill_unset, d_sdf);
}

// The two halves of vp_jfa (the reference times them separately: "::Initialization" / "::Processing",
// jfa/tiled.cu:265-334).  start: border mask (tile kernels) or init ids; run: every pass + the id -> sdf conversion.
static int jfa_check(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, void*& d_work, size_t& work_bytes, int algo, const char* who)
{
    if (!ctx || !d_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, true));
    VP_TRY(check_aligned(who, {d_words, d_work}));
    VP_TRY(check_algo(who, algo));
    if (!d_work) {                                                 // context-owned workspace (grow-only, reused by later calls)
        const void* before = ctx->jfa.work.ptr;
        VP_TRY(reserve(ctx, ctx->jfa.work, vp_jfa_workspace_bytes(f)));
        if (ctx->jfa.work.ptr != before) ctx->jfa.started.valid = false;   // regrown: what a vp_jfa_start left there is gone
        d_work = ctx->jfa.work.ptr;
        work_bytes = ctx->jfa.work.bytes;
    } else if (work_bytes < vp_jfa_workspace_bytes(f)) {
        return set_error(VP_ERR_INVALID, "%s: workspace too small", who);
    }
    return 0;
}

// The tile-kernel sequence of a whole grid: border mask -> passes n/2 + n/4 in one launch -> tile passes on two windows of n planes
// inside the workspace -> last pass fused with the id -> sdf conversion.
static bool jfa_tile_sequence(const Frame& fr, int algo) { return jfa_can_fuse_first_two(fr, algo) && fr.n / 4 >= 1; }

int vp_jfa_start(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, void* d_work, size_t work_bytes, int algo)
{
    const bool explicitWork = d_work != nullptr;                   // the context's own workspace is nobody's grid
    VP_TRY(jfa_check(ctx, f, d_words, d_work, work_bytes, algo, "vp_jfa_start"));
    const Frame fr = make_frame(f);
    const size_t volBytes = vp_grid_voxels(f) * vp_jfa_id_bytes(f);
    char* a = (char*)d_work;
    const bool mask = jfa_tile_sequence(fr, algo);
    ctx->jfa.started.valid = false;
    if (explicitWork) grid_written(ctx, d_work, vp_jfa_workspace_bytes(f));     // the workspace may be a grid somebody counted
    if (mask) VP_TRY(launch_jfa_init(ctx, fr, d_words, nullptr, nullptr, nullptr, (uint32_t*)(a + 2 * volBytes)));   // border mask only
    else      VP_TRY(launch_jfa_init(ctx, fr, d_words, nullptr, nullptr, a, nullptr));
    ctx->jfa.started = {true, mask, f->n, algo, d_work, work_bytes, d_words};
    return 0;
}

int vp_jfa_run(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, float fill_unset, float* d_sdf,
               void* d_work, size_t work_bytes, int algo)
{
    if (!d_sdf) return set_error(VP_ERR_INVALID, "vp_jfa_run: null argument");
    VP_TRY(check_aligned("vp_jfa_run", {d_sdf}));
    const bool explicitWork = d_work != nullptr;
    VP_TRY(jfa_check(ctx, f, d_words, d_work, work_bytes, algo, "vp_jfa_run"));
    VP_TRY(check_fill(fill_unset, "vp_jfa_run"));
    const Frame fr = make_frame(f);
    const size_t volBytes = vp_grid_voxels(f) * vp_jfa_id_bytes(f);
    char* a = (char*)d_work;
    char* b = a + volBytes;
    uint32_t k = f->n / 2;                                         // jfa/sequential.cpp:72
    // The workspace must hold what THIS sequence starts from: the record of the matching vp_jfa_start (same grid, frame size,
    // algo and workspace).  One start serves one run: the passes overwrite the volumes.
    const bool wantMask = jfa_tile_sequence(fr, algo);
    const vp_ctx::Jfa::Started st = ctx->jfa.started;
    ctx->jfa.started.valid = false;
    if (!st.valid || st.n != f->n || st.algo != algo || st.work != d_work || st.words != d_words || st.mask != wantMask)
        return set_error(VP_ERR_INVALID, "vp_jfa_run: call vp_jfa_start with the same grid, frame, algo and workspace first");
    if (explicitWork) grid_written(ctx, d_work, vp_jfa_workspace_bytes(f));     // the passes overwrite the volumes (the caller's: the context's own is nobody's grid)
    grid_written(ctx, d_sdf, vp_grid_voxels(f) * 4);               // the sdf is an output like any other
    if (wantMask) {
        // two windows of n planes (5 bytes per voxel above n = 1024, inside the 8-byte volumes of the workspace: nobody outside this
        // function sees them)
        IdWin wa, wb;
        wa.base = a; wb.base = b; wa.planes = wb.planes = f->n; wa.at = wb.at = 0;
        VP_TRY(launch_win_first_two(ctx, fr, (const uint32_t*)(b + volBytes), wa));    // passes n/2 and n/4 straight from the border mask
        for (k /= 4; k >= 1; k /= 2) {
            if (k == 1) return launch_win_pass(ctx, fr, 1, wa, wb, 1, d_words, fill_unset, d_sdf);     // last pass writes the sdf itself
            VP_TRY(launch_win_pass(ctx, fr, k, wa, wb, k, nullptr, 0.0f, nullptr));
            std::swap(wa, wb);
        }
        return set_error(VP_ERR_INVALID, "vp_jfa_run: internal: no last pass");       // n >= 96: the loop always ends in its k = 1 branch
    }
    for (; k >= 1; k /= 2) {
        if (k == 1 && jfa_pass_can_fuse_final(fr, k, algo))        // last pass writes the sdf itself
            return launch_jfa_pass_ex(ctx, fr, k, a, nullptr, nullptr, b, algo, d_words, fill_unset, d_sdf);
        VP_TRY(launch_jfa_pass(ctx, fr, k, a, nullptr, nullptr, b, algo));
        char* t = a; a = b; b = t;
    }
    return launch_jfa_final(ctx, fr, d_words, a, fill_unset, d_sdf);
}

int vp_jfa(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, float fill_unset, float* d_sdf,
           void* d_work, size_t work_bytes, int algo)
{
    if (!d_sdf) return set_error(VP_ERR_INVALID, "vp_jfa: null argument");
    VP_TRY(check_aligned("vp_jfa", {d_sdf}));
    VP_TRY(check_fill(fill_unset, "vp_jfa"));
    VP_TRY(vp_jfa_start(ctx, f, d_words, d_work, work_bytes, algo));
    return vp_jfa_run(ctx, f, d_words, fill_unset, d_sdf, d_work, work_bytes, algo);
}

size_t vp_jfa_state_bytes(const vp_frame* f, int algo)
{
    if (!f || check_frame(f, "vp_jfa_state_bytes", false) != 0) return 0;
    return (algo == VP_ALGO_TILED && win_compact(f->n)) ? 5 : vp_jfa_id_bytes(f);
}

int vp_jfa_last_shapes(const vp_ctx* ctx, vp_jfa_shape* out, int cap)
{
    if (!ctx) return 0;
    for (int i = 0; out && i < ctx->dense_shape_count && i < cap; ++i) out[i] = ctx->dense_shapes[i];
    return ctx->dense_shape_count;
}

int vp_jfa_can_start_from_mask(const vp_frame* f, int algo)
{
    return (f && check_frame(f, "vp_jfa_can_start_from_mask", false) == 0 && jfa_can_start_from_mask(make_frame(f), algo)) ? 1 : 0;
}

int vp_jfa_can_fuse_first_two(const vp_frame* f, int algo)
{
    return (f && check_frame(f, "vp_jfa_can_fuse_first_two", false) == 0 && jfa_can_fuse_first_two(make_frame(f), algo)) ? 1 : 0;
}

int vp_jfa_last_pass(vp_ctx* ctx, const vp_frame* f, const void* d_in, const void* d_minus, const void* d_plus,
                     void* d_scratch, const uint32_t* d_words, float fill_unset, float* d_sdf, int algo)
{
    if (ctx) ctx->dense_shape_count = 0;
    if (!ctx || !d_in || !d_scratch || !d_words || !d_sdf || d_in == d_scratch)
        return set_error(VP_ERR_INVALID, "vp_jfa_last_pass: bad buffers");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_jfa_last_pass", false));
    VP_TRY(check_aligned("vp_jfa_last_pass", {d_in, d_minus, d_plus, d_words, d_sdf}));
    VP_TRY(check_fill(fill_unset, "vp_jfa_last_pass"));
    VP_TRY(check_algo("vp_jfa_last_pass", algo));
    if (f->z0 > 0 && !d_minus) return set_error(VP_ERR_INVALID, "vp_jfa_last_pass: slab needs d_minus");
    if (f->z1 < f->n && !d_plus) return set_error(VP_ERR_INVALID, "vp_jfa_last_pass: slab needs d_plus");
    grid_written(ctx, d_scratch, vp_grid_voxels(f) * vp_jfa_id_bytes(f));
    grid_written(ctx, d_sdf, vp_grid_voxels(f) * 4);
    const Frame fr = make_frame(f);
    if (jfa_pass_can_fuse_final(fr, 1, algo))
        return launch_jfa_pass_ex(ctx, fr, 1, d_in, d_minus, d_plus, d_scratch, algo, d_words, fill_unset, d_sdf);
    VP_TRY(launch_jfa_pass(ctx, fr, 1, d_in, d_minus, d_plus, d_scratch, algo));
    return launch_jfa_final(ctx, fr, d_words, d_scratch, fill_unset, d_sdf);
}

// ---- id windows: the slab form of the tile kernels ------------------------------------------------
size_t vp_jfa_window_bytes(const vp_frame* f, uint32_t planes)
{
    if (!f || check_frame(f, "vp_jfa_window_bytes", false) != 0) return 0;
    return win_bytes(f->n, planes);
}

int vp_jfa_window_span(const vp_frame* f, uint32_t planes, uint32_t p0, uint32_t p1, size_t offset[2], size_t bytes[2])
{
    if (!offset || !bytes) return set_error(VP_ERR_INVALID, "vp_jfa_window_span: null argument");
    VP_TRY(check_frame(f, "vp_jfa_window_span", false));
    if (p0 > p1 || p1 > planes) return set_error(VP_ERR_INVALID, "vp_jfa_window_span: planes [%u, %u) of %u", p0, p1, planes);
    const size_t wp = win_plane_bytes(f->n), bp = (size_t)f->n * f->n;
    offset[0] = (size_t)p0 * wp; bytes[0] = (size_t)(p1 - p0) * wp;
    offset[1] = (size_t)planes * wp + (size_t)p0 * bp; bytes[1] = win_compact(f->n) ? (size_t)(p1 - p0) * bp : 0;
    return 0;
}

// A window and the frame it is used with: the planes of f must lie inside it; `below` / `above` = planes the call reads beyond them.
static int window_check(vp_ctx* ctx, const vp_frame* f, const vp_window* w, const char* who, uint32_t below, uint32_t above, IdWin& out)
{
    if (!ctx || !w || !w->d_ids) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_aligned(who, {w->d_ids}));
    if (f->n < kTileMinN) return set_error(VP_ERR_UNSUPPORTED, "%s: windows are the layout of the tile kernels (n >= %u)", who, kTileMinN);
    const uint64_t nz = f->z1 - f->z0;
    if (w->bytes < win_bytes(f->n, w->planes))
        return set_error(VP_ERR_INVALID, "%s: a window of %u planes needs %zu bytes, %zu given", who, w->planes, win_bytes(f->n, w->planes), w->bytes);
    if (w->planes == 0 || (uint64_t)w->at + nz + above > w->planes || w->at < below)
        return set_error(VP_ERR_INVALID, "%s: planes [%u, %u) at index %u (+%u below, +%u above) do not fit a window of %u planes", who, f->z0, f->z1, w->at, below, above, w->planes);
    out.base = (char*)w->d_ids; out.planes = w->planes; out.at = w->at;
    return 0;
}

// Every vp_jfa_window_* call that writes ids: the output window is a write through the ABI like any other (it may lie inside the workspace
// a vp_jfa_start left its state in, or be a grid a vp_extract_count counted): the records are dropped.
static void window_written(vp_ctx* ctx, const vp_window* w) { grid_written(ctx, w->d_ids, w->bytes); }

int vp_jfa_window_clear(vp_ctx* ctx, const vp_frame* f, const vp_window* w)
{
    if (!ctx || !w || !w->d_ids || !w->planes) return set_error(VP_ERR_INVALID, "vp_jfa_window_clear: null argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_jfa_window_clear", false));
    VP_TRY(check_aligned("vp_jfa_window_clear", {w->d_ids}));
    if (w->bytes < win_bytes(f->n, w->planes)) return set_error(VP_ERR_INVALID, "vp_jfa_window_clear: a window of %u planes needs %zu bytes, %zu given", w->planes, win_bytes(f->n, w->planes), w->bytes);
    IdWin iw; iw.base = (char*)w->d_ids; iw.planes = w->planes; iw.at = 0;
    window_written(ctx, w);
    return launch_win_clear(ctx, f->n, iw);
}

int vp_jfa_window_init(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const uint32_t* d_plane_below,
                       const uint32_t* d_plane_above, const vp_window* out)
{
    if (!d_words) return set_error(VP_ERR_INVALID, "vp_jfa_window_init: null argument");
    IdWin w;
    VP_TRY(window_check(ctx, f, out, "vp_jfa_window_init", 0, 0, w));
    VP_TRY(check_aligned("vp_jfa_window_init", {d_words, d_plane_below, d_plane_above}));
    window_written(ctx, out);
    return launch_win_init(ctx, make_frame(f), d_words, d_plane_below, d_plane_above, w);
}

int vp_jfa_window_first_pass(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_border_grid, const vp_window* out)
{
    if (!d_border_grid) return set_error(VP_ERR_INVALID, "vp_jfa_window_first_pass: null argument");
    IdWin w;
    VP_TRY(window_check(ctx, f, out, "vp_jfa_window_first_pass", 0, 0, w));
    VP_TRY(check_aligned("vp_jfa_window_first_pass", {d_border_grid}));
    const Frame fr = make_frame(f);
    if (!jfa_can_start_from_mask(fr, VP_ALGO_TILED)) return set_error(VP_ERR_UNSUPPORTED, "vp_jfa_window_first_pass: needs n %% 128 == 0");
    window_written(ctx, out);
    return launch_win_first_pass(ctx, fr, d_border_grid, w);
}

int vp_jfa_window_first_two(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_border_grid, const vp_window* out)
{
    if (!d_border_grid) return set_error(VP_ERR_INVALID, "vp_jfa_window_first_two: null argument");
    IdWin w;
    VP_TRY(window_check(ctx, f, out, "vp_jfa_window_first_two", 0, 0, w));
    VP_TRY(check_aligned("vp_jfa_window_first_two", {d_border_grid}));
    const Frame fr = make_frame(f);
    if (!jfa_can_fuse_first_two(fr, VP_ALGO_TILED) || w.planes != f->n || w.at != 0)
        return set_error(VP_ERR_INVALID, "vp_jfa_window_first_two: whole-grid frame and a window of n planes (at = 0) required");
    window_written(ctx, out);
    return launch_win_first_two(ctx, fr, d_border_grid, w);
}

// ---- cyclic plane distribution (the first phase of the transposed multi-GPU pipeline) ----
int vp_jfa_cyclic_passes(const vp_frame* f, uint32_t ranks)
{
    if (!f || check_frame(f, "vp_jfa_cyclic_passes", true) != 0) return 0;
    return (int)jfa_cyclic_passes(f->n, ranks);
}

// a whole-grid frame and a window of the n / ranks planes of one rank, at = 0
static int cyclic_check(vp_ctx* ctx, const vp_frame* f, const vp_window* w, uint32_t ranks, uint32_t rank, const char* who, IdWin& out)
{
    if (!ctx || !w || !w->d_ids) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, true));
    VP_TRY(check_aligned(who, {w->d_ids}));
    if (jfa_cyclic_passes(f->n, ranks) == 0 || rank >= ranks)
        return set_error(VP_ERR_UNSUPPORTED, "%s: n = %u cannot be dealt cyclically to %u ranks (rank %u): a power of two, n / ranks a multiple of 8, n/4 a multiple of it", who, f->n, ranks, rank);
    if (w->planes != f->n / ranks || w->at != 0 || w->bytes < win_bytes(f->n, w->planes))
        return set_error(VP_ERR_INVALID, "%s: a window of n / ranks = %u planes (at = 0, %zu bytes) required", who, f->n / ranks, win_bytes(f->n, f->n / ranks));
    out.base = (char*)w->d_ids; out.planes = w->planes; out.at = 0;
    return 0;
}

int vp_jfa_window_first_two_cyclic(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_border_grid, const vp_window* out, uint32_t ranks, uint32_t rank)
{
    if (!d_border_grid) return set_error(VP_ERR_INVALID, "vp_jfa_window_first_two_cyclic: null argument");
    IdWin w;
    VP_TRY(cyclic_check(ctx, f, out, ranks, rank, "vp_jfa_window_first_two_cyclic", w));
    VP_TRY(check_aligned("vp_jfa_window_first_two_cyclic", {d_border_grid}));
    window_written(ctx, out);
    return launch_win_first_two(ctx, make_frame(f), d_border_grid, w, ranks, rank);
}

int vp_jfa_window_pass_cyclic(vp_ctx* ctx, const vp_frame* f, uint32_t k, const vp_window* in, const vp_window* out, uint32_t ranks, uint32_t rank)
{
    const char* who = "vp_jfa_window_pass_cyclic";
    if (ctx) ctx->dense_shape_count = 0;
    IdWin wi, wo;
    VP_TRY(cyclic_check(ctx, f, in, ranks, rank, who, wi));
    VP_TRY(cyclic_check(ctx, f, out, ranks, rank, who, wo));
    if (overlaps(in->d_ids, win_bytes(f->n, in->planes), out->d_ids, win_bytes(f->n, out->planes))) return set_error(VP_ERR_INVALID, "%s: the two windows overlap", who);
    // one of the leading steps of the halving sequence, beyond the two of the fused start
    bool found = false;
    uint32_t c = jfa_cyclic_passes(f->n, ranks), kk = f->n / 2;
    for (uint32_t i = 0; i < c; ++i, kk /= 2) if (kk == k && i >= 2) found = true;
    if (!found) return set_error(VP_ERR_INVALID, "%s: step %u is not one of the steps n/8 .. of n = %u that are multiples of %u ranks", who, k, f->n, ranks);
    window_written(ctx, out);
    return launch_win_pass_cyclic(ctx, make_frame(f), k, wi, wo, ranks, rank);
}

int vp_jfa_window_interleave(vp_ctx* ctx, const vp_frame* f, const vp_window* in, const vp_window* out, uint32_t ranks, uint32_t count)
{
    const char* who = "vp_jfa_window_interleave";
    if (!ctx || !in || !out || !in->d_ids || !out->d_ids || !ranks || !count) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_aligned(who, {in->d_ids, out->d_ids}));
    if (f->n < kTileMinN) return set_error(VP_ERR_UNSUPPORTED, "%s: windows are the layout of the tile kernels (n >= %u)", who, kTileMinN);
    const uint64_t planes = (uint64_t)ranks * count;
    if (in->planes != planes || in->bytes < win_bytes(f->n, in->planes))
        return set_error(VP_ERR_INVALID, "%s: the source must be a window of exactly ranks x count = %llu planes", who, (unsigned long long)planes);
    if ((uint64_t)out->at + planes > out->planes || out->bytes < win_bytes(f->n, out->planes))
        return set_error(VP_ERR_INVALID, "%s: %llu planes at index %u do not fit a window of %u planes", who, (unsigned long long)planes, out->at, out->planes);
    if (overlaps(in->d_ids, win_bytes(f->n, in->planes), out->d_ids, win_bytes(f->n, out->planes))) return set_error(VP_ERR_INVALID, "%s: the two windows overlap", who);
    IdWin wi, wo;
    wi.base = (char*)in->d_ids; wi.planes = in->planes; wi.at = 0;
    wo.base = (char*)out->d_ids; wo.planes = out->planes; wo.at = out->at;
    window_written(ctx, out);
    return launch_win_interleave(ctx, f->n, wi, wo, ranks, count);
}

// planes a pass with step k reads below / above the planes of f, in window planes
static void pass_reach(const vp_frame* f, uint32_t k, uint32_t stride, uint32_t& below, uint32_t& above)
{
    if (stride == k) {                                              // consecutive planes: as far as the grid goes
        below = std::min(k, f->z0);
        above = std::min(k, f->n - f->z1);
    } else {                                                       // whole slabs `stride` planes away
        below = f->z1 > k ? stride : 0;                            // some plane z of f has z - k >= 0
        above = f->z0 + k < f->n ? stride : 0;
    }
}

static int window_pass(vp_ctx* ctx, const vp_frame* f, uint32_t k, const vp_window* in, const vp_window* out, uint32_t stride,
                       const uint32_t* d_words, float fill, float* d_sdf, const char* who)
{
    if (ctx) ctx->dense_shape_count = 0;                            // vp_jfa_last_shapes: the launches of this call, none if it is refused
    if (!in || !out || !in->d_ids || !out->d_ids || in->d_ids == out->d_ids) return set_error(VP_ERR_INVALID, "%s: bad windows", who);
    if (in->planes != out->planes || in->at != out->at) return set_error(VP_ERR_INVALID, "%s: the two windows must have the same planes / at", who);
    // two windows carved from one allocation that partly overlap would have the pass read planes it is overwriting
    if (f && f->n && overlaps(in->d_ids, win_bytes(f->n, in->planes), out->d_ids, win_bytes(f->n, out->planes)))
        return set_error(VP_ERR_INVALID, "%s: the two windows overlap", who);
    if (!f || k == 0 || k >= f->n) return set_error(VP_ERR_INVALID, "%s: step %u out of range", who, k);
    if (stride == 0 || (stride != k && (k < f->z1 - f->z0 || stride < f->z1 - f->z0)))
        return set_error(VP_ERR_INVALID, "%s: stride %u: either the step itself or, for a step of at least the slab height, the distance of the slabs in the window", who, stride);
    uint32_t below = 0, above = 0;
    pass_reach(f, k, stride, below, above);
    IdWin wi, wo;
    VP_TRY(window_check(ctx, f, in, who, below, above, wi));
    VP_TRY(window_check(ctx, f, out, who, 0, 0, wo));
    window_written(ctx, out);
    if (d_sdf) grid_written(ctx, d_sdf, vp_grid_voxels(f) * 4);     // vp_jfa_window_last_pass: the sdf of the region
    return launch_win_pass(ctx, make_frame(f), k, wi, wo, stride, d_words, fill, d_sdf);
}

int vp_jfa_window_pass(vp_ctx* ctx, const vp_frame* f, uint32_t k, const vp_window* in, const vp_window* out, uint32_t stride)
{
    return window_pass(ctx, f, k, in, out, stride, nullptr, 0.0f, nullptr, "vp_jfa_window_pass");
}

int vp_jfa_window_last_pass(vp_ctx* ctx, const vp_frame* f, const vp_window* in, const vp_window* scratch, uint32_t stride,
                            const uint32_t* d_words_region, float fill_unset, float* d_sdf_region)
{
    if (!d_words_region || !d_sdf_region) return set_error(VP_ERR_INVALID, "vp_jfa_window_last_pass: null argument");
    VP_TRY(check_aligned("vp_jfa_window_last_pass", {d_words_region, d_sdf_region}));
    VP_TRY(check_fill(fill_unset, "vp_jfa_window_last_pass"));
    return window_pass(ctx, f, 1, in, scratch, stride, d_words_region, fill_unset, d_sdf_region, "vp_jfa_window_last_pass");
}

// ---- export front end -------------------------------------------------------------------------
int vp_extract_count(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int mode, uint64_t* h_count)
{
    if (!ctx || !d_words) return set_error(VP_ERR_INVALID, "vp_extract_count: null argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_extract_count", true));
    if (mode < VP_EXTRACT_SET || mode > VP_EXTRACT_FACES) return set_error(VP_ERR_INVALID, "vp_extract_count: mode %d", mode);
    return launch_extract_count(ctx, make_frame(f), d_words, mode, h_count);
}

int vp_extract(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int mode, const float* d_sdf,
               uint64_t* d_records, float* d_values, size_t capacity)
{
    if (!ctx || !d_words || (!d_records && capacity)) return set_error(VP_ERR_INVALID, "vp_extract: null argument");
    if ((d_values != nullptr) != (d_sdf != nullptr)) return set_error(VP_ERR_INVALID, "vp_extract: d_sdf and d_values go together");
    VP_TRY(bind_device(ctx));
    VP_TRY(check_frame(f, "vp_extract", true));
    if (mode < VP_EXTRACT_SET || mode > VP_EXTRACT_FACES) return set_error(VP_ERR_INVALID, "vp_extract: mode %d", mode);
    // the records and values are outputs like any other: at most min(capacity, the standing count) of them are written.  Reported whether or
    // not that count is of this grid -- launch_extract_write alone decides that, and refuses below where it is not; an output that lies on
    // the grid itself drops the count here and is refused too
    const size_t cnt = (size_t)std::min<uint64_t>(capacity, ctx->ext.total);
    if (cnt) {
        grid_written(ctx, d_records, cnt * 8);
        grid_written(ctx, d_values, cnt * 4);
    }
    return launch_extract_write(ctx, make_frame(f), d_words, mode, d_sdf, d_records, d_values, capacity);
}

// ---- surface nets ------------------------------------------------------------------------------
// what the three vp_surfnets* entry points share: whole grids up to n = 1024
static int check_surfnets(const vp_frame* f, const char* who)
{
    return check_grid_1024(f, who, "32 <= n <= 1024: cell indices are 32-bit");
}

int vp_surfnets_count(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint64_t* h_vertices, uint64_t* h_quads)
{
    const char* who = "vp_surfnets_count";
    if (!ctx || !d_words || !h_vertices || !h_quads) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_surfnets(f, who));
    VP_TRY(check_algo(who, algo));
    VP_TRY(check_aligned(who, {d_words}));
    return launch_surfnets_count(ctx, f->n, d_words, algo, h_vertices, h_quads);
}

int vp_surfnets(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint32_t iterations, uint64_t* d_cells, float* d_xyz,
                uint32_t* d_quads, size_t vertex_capacity, size_t quad_capacity)
{
    const char* who = "vp_surfnets";
    if (!ctx || !d_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_surfnets(f, who));
    VP_TRY(check_algo(who, algo));
    if (iterations > 64) return set_error(VP_ERR_INVALID, "%s: %u iterations (0 .. 64)", who, iterations);
    if (ctx->sn.words != d_words || ctx->sn.algo != algo || ctx->sn.n != f->n)
        return set_error(VP_ERR_INVALID, "%s: call vp_surfnets_count with the same grid and algo first", who);
    if (vertex_capacity < ctx->sn.vertices || quad_capacity < ctx->sn.quads)
        return set_error(VP_ERR_INVALID, "%s: capacity %zu vertices / %zu quads, the grid has %llu / %llu", who, vertex_capacity, quad_capacity,
                         (unsigned long long)ctx->sn.vertices, (unsigned long long)ctx->sn.quads);
    if ((ctx->sn.vertices && (!d_cells || !d_xyz)) || (ctx->sn.quads && !d_quads)) return set_error(VP_ERR_INVALID, "%s: null output", who);
    const size_t gb = vp_grid_words(f) * 4, cb = (size_t)ctx->sn.vertices * 8, xb = (size_t)ctx->sn.vertices * 12, qb = (size_t)ctx->sn.quads * 16;
    if (overlaps(d_words, gb, d_cells, cb) || overlaps(d_words, gb, d_xyz, xb) || overlaps(d_words, gb, d_quads, qb))
        return set_error(VP_ERR_INVALID, "%s: an output overlaps d_words", who);
    grid_written(ctx, d_cells, cb); grid_written(ctx, d_xyz, xb); grid_written(ctx, d_quads, qb);     // writes like any other (not to this grid)
    return launch_surfnets_write(ctx, f->n, d_words, algo, iterations, d_cells, d_xyz, d_quads);
}

// ---- iso-surface nets --------------------------------------------------------------------------
static int check_isonets(const vp_frame* f, const char* who, int transform, float iso, uint32_t iterations, int algo)
{
    VP_TRY(check_surfnets(f, who));
    if (transform != VP_ISO_LINEAR && transform != VP_ISO_SIGNED_SQUARE) return set_error(VP_ERR_INVALID, "%s: unknown transform %d", who, transform);
    VP_TRY(check_algo(who, algo));
    if (!std::isfinite(iso)) return set_error(VP_ERR_INVALID, "%s: iso must be finite", who);
    if (iterations > 64) return set_error(VP_ERR_INVALID, "%s: %u iterations (0 .. 64)", who, iterations);
    return 0;
}

int vp_isonets(vp_ctx* ctx, const vp_frame* f, const float* d_field, int transform, float iso, uint32_t iterations, int want_normals,
               int algo, uint64_t* h_vertices, uint64_t* h_quads)
{
    const char* who = "vp_isonets";
    if (!ctx || !f || !d_field) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_isonets(f, who, transform, iso, iterations, algo));
    VP_TRY(check_aligned(who, {d_field}));
    VP_TRY(build_owned(ctx, who, ctx->iso, {}, {}, [&] { return launch_isonets(ctx, f->n, d_field, transform, iso, iterations, want_normals != 0, algo); }));
    return vp_isonets_result(ctx, nullptr, nullptr, nullptr, nullptr, h_vertices, h_quads);
}

int vp_isonets_result(vp_ctx* ctx, uint64_t** d_cells, float** d_xyz, float** d_normals, uint32_t** d_quads, uint64_t* h_vertices,
                      uint64_t* h_quads)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_isonets_result: null ctx");
    const bool any = ctx->iso.vertices != 0;                       // no vertex, hence no quad
    if (d_cells) *d_cells = any ? (uint64_t*)ctx->iso.cells.ptr : nullptr;
    if (d_xyz) *d_xyz = any ? (float*)ctx->iso.xyz.ptr : nullptr;
    if (d_normals) *d_normals = any && ctx->iso.has_normals ? (float*)ctx->iso.normals.ptr : nullptr;
    if (d_quads) *d_quads = any ? (uint32_t*)ctx->iso.quads.ptr : nullptr;
    if (h_vertices) *h_vertices = ctx->iso.vertices;
    if (h_quads) *h_quads = ctx->iso.quad_count;
    return 0;
}

// ---- generalized winding number ------------------------------------------------------------------
// what vp_winding and its host form share: whole grids up to n = 1024, the algo, beta in {0} U [1, 64], a finite level
static int check_winding(const vp_frame* f, const char* who, float beta, float level, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (!(beta == 0.0f || (beta >= 1.0f && beta <= 64.0f))) return set_error(VP_ERR_INVALID, "%s: beta %g (0, or 1 .. 64)", who, (double)beta);
    if (!std::isfinite(level)) return set_error(VP_ERR_INVALID, "%s: level must be finite", who);
    return 0;
}

int vp_winding(vp_ctx* ctx, const vp_frame* f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris, float beta,
               float level, int algo, uint64_t* h_inside_count)
{
    const char* who = "vp_winding";
    if (!ctx || !f) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_winding(f, who, beta, level, algo));
    if (ntris && (!d_xyz || !d_tri || !nverts)) return set_error(VP_ERR_INVALID, "%s: null mesh arrays", who);
    if (ntris > 0xFFFFFFFFull / 3) return set_error(VP_ERR_UNSUPPORTED, "%s: too many triangles", who);
    VP_TRY(check_aligned(who, {d_xyz, d_tri}));
    return build_owned(ctx, who, ctx->wn, {}, {},
                       [&] { return launch_winding(ctx, make_frame(f), d_xyz, nverts, d_tri, ntris, beta, level, algo, h_inside_count); });
}

int vp_winding_result(vp_ctx* ctx, float** d_w, uint32_t** d_inside, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_winding_result: null ctx");
    const bool any = ctx->wn.n != 0;
    if (d_w) *d_w = any ? (float*)ctx->wn.w.ptr : nullptr;
    if (d_inside) *d_inside = any ? (uint32_t*)ctx->wn.inside.ptr : nullptr;
    if (h_n) *h_n = ctx->wn.n;
    return 0;
}

// ---- local thickness -------------------------------------------------------------------------------
// what vp_thickness and its host form share: whole grids up to n = 1024, the algo, rmax in 1 .. 32, thin2 in 0 .. rmax^2
static int check_thickness(const vp_frame* f, const char* who, uint32_t rmax, uint32_t thin2, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (rmax < 1 || rmax > 32) return set_error(VP_ERR_INVALID, "%s: rmax %u (1 .. 32)", who, rmax);
    if (thin2 > rmax * rmax) return set_error(VP_ERR_INVALID, "%s: thin2 %u (0 .. rmax^2 = %u)", who, thin2, rmax * rmax);
    return 0;
}

int vp_thickness(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t rmax, uint32_t thin2, int algo, uint64_t* h_thin_count)
{
    const char* who = "vp_thickness";
    if (!ctx || !f || !d_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_thickness(f, who, rmax, thin2, algo));
    VP_TRY(check_aligned(who, {d_words}));
    // the distance volumes of the transform are written too
    return build_owned(ctx, who, ctx->th, {&ctx->edt.vol, &ctx->edt.vol2}, {{d_words, vp_grid_words(f) * 4}},
                       [&] { return launch_thickness(ctx, make_frame(f), d_words, rmax, thin2, algo, h_thin_count); });
}

int vp_thickness_result(vp_ctx* ctx, uint32_t** d_t2, uint32_t** d_thin, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_thickness_result: null ctx");
    const bool any = ctx->th.n != 0;
    if (d_t2) *d_t2 = any ? (uint32_t*)ctx->th.t2.ptr : nullptr;
    if (d_thin) *d_thin = any ? (uint32_t*)ctx->th.thin.ptr : nullptr;
    if (h_n) *h_n = ctx->th.n;
    return 0;
}

// ---- sparse voxel octree ---------------------------------------------------------------------------
int vp_octree(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint64_t* h_nodes)
{
    const char* who = "vp_octree";
    if (!ctx || !f || !d_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_grid_1024(f, who, algo));
    VP_TRY(check_aligned(who, {d_words}));
    return build_owned(ctx, who, ctx->oc, {}, {{d_words, vp_grid_words(f) * 4}}, [&] { return launch_octree(ctx, make_frame(f), d_words, algo, h_nodes); });
}

int vp_octree_result(vp_ctx* ctx, uint32_t** d_nodes, uint64_t* h_nodes, uint32_t* h_level_offset, uint32_t* h_full_leaves, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_octree_result: null ctx");
    const bool any = ctx->oc.n != 0;
    if (d_nodes) *d_nodes = any ? (uint32_t*)ctx->oc.nodes.ptr : nullptr;
    if (h_nodes) *h_nodes = any ? ctx->oc.count : 0;
    for (int l = 0; l < 11; ++l) {
        if (h_level_offset) h_level_offset[l] = any ? ctx->oc.level_offset[l] : 0u;
        if (h_full_leaves) h_full_leaves[l] = any ? ctx->oc.full_leaves[l] : 0u;
    }
    if (h_n) *h_n = ctx->oc.n;
    return 0;
}

int vp_octree_expand(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_nodes, uint64_t nodes, int algo)
{
    const char* who = "vp_octree_expand";
    if (!ctx || !f || !d_nodes) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_grid_1024(f, who, algo));
    if (nodes < 1 || nodes >= (1ull << 28)) return set_error(VP_ERR_INVALID, "%s: %llu nodes (1 .. 2^28 - 1)", who, (unsigned long long)nodes);
    VP_TRY(check_aligned(who, {d_nodes}));
    vp_ctx::OcExpand& ox = ctx->ocx;
    // the nodes are read while the context's grid is written: they may not lie in it (refused in this call's own words)
    if (overlaps(d_nodes, nodes * 8, ox.grid.ptr, ox.grid.bytes)) return set_error(VP_ERR_INVALID, "%s: d_nodes overlaps the context's grid", who);
    return build_owned(ctx, who, ox, {}, {}, [&]() -> int {
        ox.n = 0;                                                  // from here on the previous result is gone
        VP_TRY(reserve(ctx, ox.grid, vp_grid_words(f) * 4, false));
        VP_TRY(launch_octree_expand(ctx, make_frame(f), d_nodes, nodes, (uint32_t*)ox.grid.ptr, algo));
        ox.n = f->n;
        return 0;
    });
}

int vp_octree_expand_result(vp_ctx* ctx, uint32_t** d_words, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_octree_expand_result: null ctx");
    if (d_words) *d_words = ctx->ocx.n ? (uint32_t*)ctx->ocx.grid.ptr : nullptr;
    if (h_n) *h_n = ctx->ocx.n;
    return 0;
}

int vp_octree_validate_host(const uint32_t* h_nodes, uint64_t nodes, uint32_t n) { return octree_validate(h_nodes, nodes, n); }

// ---- topological thinning --------------------------------------------------------------------------
// what vp_skeleton and its host form share: whole grids up to n = 1024, the mode and the algo
static int check_skeleton(const vp_frame* f, const char* who, int mode, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (mode != VP_SKEL_KERNEL && mode != VP_SKEL_CURVE) return set_error(VP_ERR_INVALID, "%s: unknown mode %d", who, mode);
    return 0;
}

int vp_skeleton(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const uint32_t* d_anchor, int mode, uint32_t max_iters, int algo,
                uint64_t* h_stats)
{
    const char* who = "vp_skeleton";
    if (!ctx || !f || !d_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_skeleton(f, who, mode, algo));
    VP_TRY(check_aligned(who, {d_words, d_anchor}));
    const size_t wb = vp_grid_words(f) * 4;                        // (a null anchor overlaps nothing)
    return build_owned(ctx, who, ctx->sk, {}, {{d_words, wb}, {d_anchor, wb}},
                       [&] { return launch_skeleton(ctx, make_frame(f), d_words, d_anchor, mode, max_iters, algo, h_stats); });
}

int vp_skeleton_result(vp_ctx* ctx, uint32_t** d_skel, uint64_t* h_stats, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_skeleton_result: null ctx");
    const bool any = ctx->sk.n != 0;
    if (d_skel) *d_skel = any ? (uint32_t*)ctx->sk.grid.ptr : nullptr;
    if (h_stats)
        for (int i = 0; i < 3; ++i) h_stats[i] = any ? ctx->sk.stats[i] : 0;
    if (h_n) *h_n = ctx->sk.n;
    return 0;
}

// ---- geodesic distance ------------------------------------------------------------------------------
// what vp_geodesic and its host form share: whole grids up to n = 1024, the metric and the algo
static int check_geodesic(const vp_frame* f, const char* who, int metric, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (metric != VP_GEO_6 && metric != VP_GEO_26 && metric != VP_GEO_CHAMFER) return set_error(VP_ERR_INVALID, "%s: unknown metric %d", who, metric);
    return 0;
}

int vp_geodesic(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_mask, const uint32_t* d_seeds, int metric, int algo, uint64_t* h_stats)
{
    const char* who = "vp_geodesic";
    if (!ctx || !f || !d_mask || !d_seeds) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_geodesic(f, who, metric, algo));
    VP_TRY(check_aligned(who, {d_mask, d_seeds}));
    const size_t wb = vp_grid_words(f) * 4;
    return build_owned(ctx, who, ctx->gd, {}, {{d_mask, wb}, {d_seeds, wb}},
                       [&] { return launch_geodesic(ctx, make_frame(f), d_mask, d_seeds, metric, algo, h_stats); });
}

int vp_geodesic_result(vp_ctx* ctx, uint32_t** d_dist, uint32_t** d_reach, uint64_t* h_stats, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_geodesic_result: null ctx");
    const bool any = ctx->gd.n != 0;
    if (d_dist) *d_dist = any ? (uint32_t*)ctx->gd.dist.ptr : nullptr;
    if (d_reach) *d_reach = any ? (uint32_t*)ctx->gd.reach.ptr : nullptr;
    if (h_stats)
        for (int i = 0; i < 4; ++i) h_stats[i] = any ? ctx->gd.stats[i] : 0;
    if (h_n) *h_n = ctx->gd.n;
    return 0;
}

// ---- seeded watershed -------------------------------------------------------------------------------
// what vp_watershed and its host form share: whole grids up to n = 1024, order and quantum (where there is a priority field), the
// connectivity and the algo
static int check_watershed(const vp_frame* f, const char* who, bool priority, int order, uint32_t quantum, int conn, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (priority && order != VP_WS_ASCENDING && order != VP_WS_DESCENDING) return set_error(VP_ERR_INVALID, "%s: unknown order %d", who, order);
    if (priority && quantum == 0) return set_error(VP_ERR_INVALID, "%s: quantum must be at least 1", who);
    if (conn != VP_CONN_6 && conn != VP_CONN_26) return set_error(VP_ERR_INVALID, "%s: unknown connectivity %d", who, conn);
    return 0;
}

int vp_watershed(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_mask, const uint32_t* d_markers, const uint32_t* d_priority, int order,
                 uint32_t quantum, int connectivity, int algo, uint64_t* h_stats)
{
    const char* who = "vp_watershed";
    if (!ctx || !f || !d_mask || !d_markers) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_watershed(f, who, d_priority != nullptr, order, quantum, connectivity, algo));
    VP_TRY(check_aligned(who, {d_mask, d_markers, d_priority}));
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;   // (a null priority field overlaps nothing)
    return build_owned(ctx, who, ctx->wsd, {}, {{d_mask, wb}, {d_markers, vb}, {d_priority, vb}}, [&] {
        return launch_watershed(ctx, make_frame(f), d_mask, d_markers, d_priority, order, quantum, connectivity, algo, h_stats);
    });
}

int vp_watershed_result(vp_ctx* ctx, uint32_t** d_labels, uint32_t** d_cut, uint64_t* h_stats, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_watershed_result: null ctx");
    const bool any = ctx->wsd.n != 0;
    if (d_labels) *d_labels = any ? (uint32_t*)ctx->wsd.labels.ptr : nullptr;
    if (d_cut) *d_cut = any ? (uint32_t*)ctx->wsd.cut.ptr : nullptr;
    if (h_stats)
        for (int i = 0; i < 4; ++i) h_stats[i] = any ? ctx->wsd.stats[i] : 0;
    if (h_n) *h_n = ctx->wsd.n;
    return 0;
}

// ---- grayscale reconstruction and h-extrema -------------------------------------------------------------
// what vp_reconstruct, vp_extrema and their host forms share: whole grids up to n = 1024, the algo, the connectivity
static int check_reconstruct(const vp_frame* f, const char* who, int conn, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (conn != VP_CONN_6 && conn != VP_CONN_26) return set_error(VP_ERR_INVALID, "%s: unknown connectivity %d", who, conn);
    return 0;
}
static int check_rec_mode(const char* who, int mode)
{
    if (mode != VP_REC_DILATION && mode != VP_REC_EROSION) return set_error(VP_ERR_INVALID, "%s: unknown mode %d", who, mode);
    return 0;
}
static int check_extrema(const char* who, int kind, int scale)
{
    if (kind != VP_EXT_MAXIMA && kind != VP_EXT_MINIMA) return set_error(VP_ERR_INVALID, "%s: unknown kind %d", who, kind);
    if (scale != VP_EXT_LINEAR && scale != VP_EXT_SQRT16) return set_error(VP_ERR_INVALID, "%s: unknown scale %d", who, scale);
    return 0;
}

int vp_reconstruct(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_domain, const uint32_t* d_marker, const uint32_t* d_mask, int mode,
                   int connectivity, int algo, uint64_t* h_stats)
{
    const char* who = "vp_reconstruct";
    if (!ctx || !f || !d_marker || !d_mask) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_reconstruct(f, who, connectivity, algo));
    VP_TRY(check_rec_mode(who, mode));
    VP_TRY(check_aligned(who, {d_domain, d_marker, d_mask}));
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;   // (a null domain overlaps nothing)
    return build_owned(ctx, who, ctx->rc, {}, {{d_domain, wb}, {d_marker, vb}, {d_mask, vb}}, [&] {
        return launch_reconstruct(ctx, make_frame(f), d_domain, d_marker, d_mask, mode, connectivity, algo, h_stats);
    });
}

int vp_reconstruct_result(vp_ctx* ctx, uint32_t** d_field, uint64_t* h_stats, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_reconstruct_result: null ctx");
    const bool any = ctx->rc.n != 0;
    if (d_field) *d_field = any ? (uint32_t*)ctx->rc.field.ptr : nullptr;
    if (h_stats)
        for (int i = 0; i < 4; ++i) h_stats[i] = any ? ctx->rc.stats[i] : 0;
    if (h_n) *h_n = ctx->rc.n;
    return 0;
}

int vp_extrema(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_domain, const uint32_t* d_values, int kind, int scale, uint32_t h,
               int connectivity, int algo, uint64_t* h_stats)
{
    const char* who = "vp_extrema";
    if (!ctx || !f || !d_values) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_reconstruct(f, who, connectivity, algo));
    VP_TRY(check_extrema(who, kind, scale));
    VP_TRY(check_aligned(who, {d_domain, d_values}));
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    return build_owned(ctx, who, ctx->ex, {}, {{d_domain, wb}, {d_values, vb}}, [&] {
        return launch_extrema(ctx, make_frame(f), d_domain, d_values, kind, scale, h, connectivity, algo, h_stats);
    });
}

int vp_extrema_result(vp_ctx* ctx, uint32_t** d_scaled, uint32_t** d_flat, uint32_t** d_extrema, uint64_t* h_stats, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_extrema_result: null ctx");
    const bool any = ctx->ex.n != 0;
    if (d_scaled) *d_scaled = any ? (uint32_t*)ctx->ex.scaled.ptr : nullptr;
    if (d_flat) *d_flat = any ? (uint32_t*)ctx->ex.flat.ptr : nullptr;
    if (d_extrema) *d_extrema = any ? (uint32_t*)ctx->ex.extrema.ptr : nullptr;
    if (h_stats)
        for (int i = 0; i < 4; ++i) h_stats[i] = any ? ctx->ex.stats[i] : 0;
    if (h_n) *h_n = ctx->ex.n;
    return 0;
}

// ---- region analysis ----------------------------------------------------------------------------------
// what vp_regions and its host form share: whole grids up to n = 1024, the algo, the bound of the label count
static int check_regions(const vp_frame* f, const char* who, uint32_t count, int algo)
{
    VP_TRY(check_grid_1024(f, who, algo));
    if (count > VP_REGIONS_MAX)
        return set_error(VP_ERR_INVALID, "%s: count %u above VP_REGIONS_MAX = %u: filter the small components out first (minsize)", who, count,
                         (uint32_t)VP_REGIONS_MAX);
    return 0;
}

int vp_regions(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_labels, uint32_t count, const uint32_t* d_values, int algo, uint64_t* h_stats)
{
    const char* who = "vp_regions";
    if (!ctx || !f || !d_labels) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(bind_device(ctx));
    VP_TRY(check_regions(f, who, count, algo));
    VP_TRY(check_aligned(who, {d_labels, d_values}));
    const size_t vb = vp_grid_voxels(f) * 4;                          // (a null value field overlaps nothing)
    return build_owned(ctx, who, ctx->rg, {}, {{d_labels, vb}, {d_values, vb}}, [&] {
        return launch_regions(ctx, make_frame(f), d_labels, count, d_values, algo, h_stats);
    });
}

int vp_regions_result(vp_ctx* ctx, uint64_t** d_table, uint32_t* h_count, uint64_t* h_stats, uint32_t* h_n)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_regions_result: null ctx");
    const bool any = ctx->rg.n != 0;
    if (d_table) *d_table = any && ctx->rg.count ? (uint64_t*)ctx->rg.table.ptr : nullptr;
    if (h_count) *h_count = any ? ctx->rg.count : 0;
    if (h_stats)
        for (int i = 0; i < 4; ++i) h_stats[i] = any ? ctx->rg.stats[i] : 0;
    if (h_n) *h_n = ctx->rg.n;
    return 0;
}

// ---- host-in / host-out ----------------------------------------------------------------------
// Device buffers come from the context's workspace slots (grow-only): steady-state calls allocate nothing, where the
// reference's Compute() does ~15 cudaMalloc/cudaFree per call.
// vp_voxelize_host and vp_voxelize_conservative_host: mesh up, one of the two device calls, grid down
static int voxelize_host(const char* who, decltype(&vp_voxelize) call, vp_ctx* ctx, const vp_frame* f, uint32_t* h_words, const float* h_xyz,
                         size_t nverts, const uint32_t* h_tri, size_t ntris, int algo)
{
    if (!ctx || !h_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_frame(f, who, true));
    void *dw = nullptr, *dx = nullptr, *dt = nullptr;
    const size_t wb = vp_grid_words(f) * 4;
    VP_TRY(vp_ctx_workspace(ctx, SLOT_GRID_A, wb, &dw));
    VP_TRY(stage(ctx, SLOT_XYZ, h_xyz, nverts * 12, &dx));
    VP_TRY(stage(ctx, SLOT_TRI, h_tri, ntris * 12, &dt));
    VP_TRY(call(ctx, f, (uint32_t*)dw, (const float*)dx, nverts, (const uint32_t*)dt, ntris, algo, 0));
    return vp_download(ctx, h_words, dw, wb);
}

int vp_voxelize_host(vp_ctx* ctx, const vp_frame* f, uint32_t* h_words, const float* h_xyz, size_t nverts,
                     const uint32_t* h_tri, size_t ntris, int algo)
{
    return voxelize_host("vp_voxelize_host", vp_voxelize, ctx, f, h_words, h_xyz, nverts, h_tri, ntris, algo);
}

int vp_voxelize_conservative_host(vp_ctx* ctx, const vp_frame* f, uint32_t* h_words, const float* h_xyz, size_t nverts,
                                  const uint32_t* h_tri, size_t ntris, int algo)
{
    return voxelize_host("vp_voxelize_conservative_host", vp_voxelize_conservative, ctx, f, h_words, h_xyz, nverts, h_tri, ntris, algo);
}

int vp_fill_interior_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out)
{
    const char* who = "vp_fill_interior_host";
    if (!ctx || !h_words || !h_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_whole(f, who));
    return host_round_trip(ctx, f, h_words, h_out, SLOT_GRID_B,
                           [&](const uint32_t* dw, void* d) { return vp_fill_interior(ctx, f, dw, (uint32_t*)d, nullptr); });
}

int vp_morph_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out, int op, uint32_t radius, int algo)
{
    const char* who = "vp_morph_host";
    if (!ctx || !h_words || !h_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_frame(f, who, false));
    VP_TRY(check_whole(f, who));
    return host_round_trip(ctx, f, h_words, h_out, SLOT_GRID_B,
                           [&](const uint32_t* dw, void* d) { return vp_morph(ctx, f, dw, (uint32_t*)d, op, radius, algo); });
}

int vp_edt_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, int seeds, uint32_t* h_dist2, int algo)
{
    const char* who = "vp_edt_host";
    if (!ctx || !h_words || !h_dist2) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_edt(f, who, algo));
    VP_TRY(check_edt_seeds(who, seeds));
    return host_round_trip(ctx, f, h_words, h_dist2, SLOT_SDF,
                           [&](const uint32_t* dw, void* d) { return vp_edt(ctx, f, dw, seeds, (uint32_t*)d, algo); });
}

int vp_edt_sdf_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, float fill_unset, float* h_sdf, int algo)
{
    const char* who = "vp_edt_sdf_host";
    if (!ctx || !h_words || !h_sdf) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_edt(f, who, algo));
    VP_TRY(check_fill(fill_unset, who));
    return host_round_trip(ctx, f, h_words, h_sdf, SLOT_SDF,
                           [&](const uint32_t* dw, void* d) { return vp_edt_sdf(ctx, f, dw, fill_unset, (float*)d, algo); });
}

int vp_edt_morph_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out, int op, uint32_t radius, int algo)
{
    const char* who = "vp_edt_morph_host";
    if (!ctx || !h_words || !h_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_edt(f, who, algo));
    VP_TRY(check_edt_morph(who, op, radius));
    return host_round_trip(ctx, f, h_words, h_out, SLOT_GRID_B,
                           [&](const uint32_t* dw, void* d) { return vp_edt_morph(ctx, f, dw, (uint32_t*)d, op, radius, algo); });
}

int vp_mesh_distance_host(vp_ctx* ctx, const vp_frame* f, const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris,
                          const uint32_t* h_sign_words, uint32_t band, float* h_dist2, uint32_t* h_nearest, int algo)
{
    const char* who = "vp_mesh_distance_host";
    if (!ctx || !h_dist2) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_mesh_distance(f, who, band, algo));
    if (ntris && (!h_xyz || !h_tri || !nverts)) return set_error(VP_ERR_INVALID, "%s: null mesh arrays", who);
    void *dw = nullptr, *dx = nullptr, *dt = nullptr, *dd = nullptr, *dn = nullptr;
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    if (h_sign_words) VP_TRY(stage(ctx, SLOT_GRID_A, h_sign_words, wb, &dw));
    VP_TRY(stage(ctx, SLOT_XYZ, h_xyz, nverts * 12, &dx));
    VP_TRY(stage(ctx, SLOT_TRI, h_tri, ntris * 12, &dt));
    VP_TRY(vp_ctx_workspace(ctx, SLOT_SDF, vb, &dd));
    if (h_nearest) VP_TRY(vp_ctx_workspace(ctx, SLOT_NEAREST, vb, &dn));
    VP_TRY(vp_mesh_distance(ctx, f, (const float*)dx, nverts, (const uint32_t*)dt, ntris, (const uint32_t*)dw, band, (float*)dd, (uint32_t*)dn, algo));
    VP_TRY(vp_download(ctx, h_dist2, dd, vb));
    return h_nearest ? vp_download(ctx, h_nearest, dn, vb) : 0;
}

int vp_winding_host(vp_ctx* ctx, const vp_frame* f, const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris, float beta,
                    float level, int algo, float* h_w, uint32_t* h_inside, uint64_t* h_inside_count)
{
    const char* who = "vp_winding_host";
    if (!ctx || !f || (!h_w && !h_inside)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_winding(f, who, beta, level, algo));
    if (ntris && (!h_xyz || !h_tri || !nverts)) return set_error(VP_ERR_INVALID, "%s: null mesh arrays", who);
    void *dx = nullptr, *dt = nullptr;
    VP_TRY(stage(ctx, SLOT_XYZ, h_xyz, nverts * 12, &dx));
    VP_TRY(stage(ctx, SLOT_TRI, h_tri, ntris * 12, &dt));
    VP_TRY(vp_winding(ctx, f, (const float*)dx, nverts, (const uint32_t*)dt, ntris, beta, level, algo, h_inside_count));
    if (h_w) VP_TRY(vp_download(ctx, h_w, ctx->wn.w.ptr, vp_grid_voxels(f) * 4));
    return h_inside ? vp_download(ctx, h_inside, ctx->wn.inside.ptr, vp_grid_words(f) * 4) : 0;
}

int vp_thickness_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t rmax, uint32_t thin2, int algo, uint32_t* h_t2,
                      uint32_t* h_thin, uint64_t* h_thin_count)
{
    const char* who = "vp_thickness_host";
    if (!ctx || !f || !h_words || (!h_t2 && !h_thin)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_thickness(f, who, rmax, thin2, algo));
    void* dw = nullptr;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_words, vp_grid_words(f) * 4, &dw));
    VP_TRY(vp_thickness(ctx, f, (const uint32_t*)dw, rmax, thin2, algo, h_thin_count));
    if (h_t2) VP_TRY(vp_download(ctx, h_t2, ctx->th.t2.ptr, vp_grid_voxels(f) * 4));
    return h_thin ? vp_download(ctx, h_thin, ctx->th.thin.ptr, vp_grid_words(f) * 4) : 0;
}

int vp_octree_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, int algo, uint32_t* h_nodes, uint64_t capacity, uint64_t* h_count,
                   uint32_t* h_level_offset, uint32_t* h_full_leaves)
{
    const char* who = "vp_octree_host";
    if (!ctx || !f || !h_words || !h_count || (!h_nodes && capacity)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_grid_1024(f, who, algo));
    void* dw = nullptr;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_words, vp_grid_words(f) * 4, &dw));
    VP_TRY(vp_octree(ctx, f, (const uint32_t*)dw, algo, h_count));
    VP_TRY(vp_octree_result(ctx, nullptr, nullptr, h_level_offset, h_full_leaves, nullptr));
    if (*h_count > capacity) return set_error(VP_ERR_INVALID, "%s: capacity %llu below the %llu nodes of the tree", who,
                                              (unsigned long long)capacity, (unsigned long long)*h_count);
    return vp_download(ctx, h_nodes, ctx->oc.nodes.ptr, *h_count * 8);
}

int vp_octree_expand_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_nodes, uint64_t nodes, int algo, uint32_t* h_words)
{
    const char* who = "vp_octree_expand_host";
    if (!ctx || !f || !h_nodes || !h_words) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_grid_1024(f, who, algo));
    VP_TRY(octree_validate(h_nodes, nodes, f->n));                 // nothing that fails the check reaches the device
    void* dn = nullptr;
    VP_TRY(stage(ctx, SLOT_SDF, h_nodes, nodes * 8, &dn));
    VP_TRY(vp_octree_expand(ctx, f, (const uint32_t*)dn, nodes, algo));
    return vp_download(ctx, h_words, ctx->ocx.grid.ptr, vp_grid_words(f) * 4);
}

int vp_skeleton_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, const uint32_t* h_anchor, int mode, uint32_t max_iters, int algo,
                     uint32_t* h_skel, uint64_t* h_stats)
{
    const char* who = "vp_skeleton_host";
    if (!ctx || !f || !h_words || (!h_skel && !h_stats)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_skeleton(f, who, mode, algo));
    void *dw = nullptr, *da = nullptr;
    const size_t wb = vp_grid_words(f) * 4;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_words, wb, &dw));
    if (h_anchor) VP_TRY(stage(ctx, SLOT_GRID_B, h_anchor, wb, &da));
    VP_TRY(vp_skeleton(ctx, f, (const uint32_t*)dw, (const uint32_t*)da, mode, max_iters, algo, h_stats));
    return h_skel ? vp_download(ctx, h_skel, ctx->sk.grid.ptr, wb) : 0;
}

int vp_geodesic_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_mask, const uint32_t* h_seeds, int metric, int algo, uint32_t* h_dist,
                     uint32_t* h_reach, uint64_t* h_stats)
{
    const char* who = "vp_geodesic_host";
    if (!ctx || !f || !h_mask || !h_seeds || (!h_dist && !h_reach && !h_stats)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_geodesic(f, who, metric, algo));
    void *dm = nullptr, *ds = nullptr;
    const size_t wb = vp_grid_words(f) * 4;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_mask, wb, &dm));
    VP_TRY(stage(ctx, SLOT_GRID_B, h_seeds, wb, &ds));
    VP_TRY(vp_geodesic(ctx, f, (const uint32_t*)dm, (const uint32_t*)ds, metric, algo, h_stats));
    if (h_dist) VP_TRY(vp_download(ctx, h_dist, ctx->gd.dist.ptr, vp_grid_voxels(f) * 4));
    return h_reach ? vp_download(ctx, h_reach, ctx->gd.reach.ptr, wb) : 0;
}

int vp_watershed_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_mask, const uint32_t* h_markers, const uint32_t* h_priority, int order,
                      uint32_t quantum, int connectivity, int algo, uint32_t* h_labels, uint32_t* h_cut, uint64_t* h_stats)
{
    const char* who = "vp_watershed_host";
    if (!ctx || !f || !h_mask || !h_markers || (!h_labels && !h_cut && !h_stats)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_watershed(f, who, h_priority != nullptr, order, quantum, connectivity, algo));
    void *dm = nullptr, *dl = nullptr, *dp = nullptr;
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_mask, wb, &dm));
    VP_TRY(stage(ctx, SLOT_SDF, h_markers, vb, &dl));
    if (h_priority) VP_TRY(stage(ctx, SLOT_NEAREST, h_priority, vb, &dp));
    VP_TRY(vp_watershed(ctx, f, (const uint32_t*)dm, (const uint32_t*)dl, (const uint32_t*)dp, order, quantum, connectivity, algo, h_stats));
    if (h_labels) VP_TRY(vp_download(ctx, h_labels, ctx->wsd.labels.ptr, vb));
    return h_cut ? vp_download(ctx, h_cut, ctx->wsd.cut.ptr, wb) : 0;
}

int vp_reconstruct_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_domain, const uint32_t* h_marker, const uint32_t* h_mask, int mode,
                        int connectivity, int algo, uint32_t* h_field, uint64_t* h_stats)
{
    const char* who = "vp_reconstruct_host";
    if (!ctx || !f || !h_marker || !h_mask || (!h_field && !h_stats)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_reconstruct(f, who, connectivity, algo));
    VP_TRY(check_rec_mode(who, mode));
    void *dd = nullptr, *df = nullptr, *dg = nullptr;
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    if (h_domain) VP_TRY(stage(ctx, SLOT_GRID_A, h_domain, wb, &dd));
    VP_TRY(stage(ctx, SLOT_SDF, h_marker, vb, &df));
    VP_TRY(stage(ctx, SLOT_NEAREST, h_mask, vb, &dg));
    VP_TRY(vp_reconstruct(ctx, f, (const uint32_t*)dd, (const uint32_t*)df, (const uint32_t*)dg, mode, connectivity, algo, h_stats));
    return h_field ? vp_download(ctx, h_field, ctx->rc.field.ptr, vb) : 0;
}

int vp_extrema_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_domain, const uint32_t* h_values, int kind, int scale, uint32_t h,
                    int connectivity, int algo, uint32_t* h_scaled, uint32_t* h_flat, uint32_t* h_extrema, uint64_t* h_stats)
{
    const char* who = "vp_extrema_host";
    if (!ctx || !f || !h_values || (!h_scaled && !h_flat && !h_extrema && !h_stats)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_reconstruct(f, who, connectivity, algo));
    VP_TRY(check_extrema(who, kind, scale));
    void *dd = nullptr, *dv = nullptr;
    const size_t wb = vp_grid_words(f) * 4, vb = vp_grid_voxels(f) * 4;
    if (h_domain) VP_TRY(stage(ctx, SLOT_GRID_A, h_domain, wb, &dd));
    VP_TRY(stage(ctx, SLOT_SDF, h_values, vb, &dv));
    VP_TRY(vp_extrema(ctx, f, (const uint32_t*)dd, (const uint32_t*)dv, kind, scale, h, connectivity, algo, h_stats));
    if (h_scaled) VP_TRY(vp_download(ctx, h_scaled, ctx->ex.scaled.ptr, vb));
    if (h_flat) VP_TRY(vp_download(ctx, h_flat, ctx->ex.flat.ptr, vb));
    return h_extrema ? vp_download(ctx, h_extrema, ctx->ex.extrema.ptr, wb) : 0;
}

int vp_regions_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_labels, uint32_t count, const uint32_t* h_values, int algo, uint64_t* h_table,
                    uint64_t* h_stats)
{
    const char* who = "vp_regions_host";
    if (!ctx || !f || !h_labels || (!h_table && !h_stats)) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_regions(f, who, count, algo));
    void *dl = nullptr, *dv = nullptr;
    const size_t vb = vp_grid_voxels(f) * 4;
    VP_TRY(stage(ctx, SLOT_SDF, h_labels, vb, &dl));
    if (h_values) VP_TRY(stage(ctx, SLOT_NEAREST, h_values, vb, &dv));
    VP_TRY(vp_regions(ctx, f, (const uint32_t*)dl, count, (const uint32_t*)dv, algo, h_stats));
    return h_table && count ? vp_download(ctx, h_table, ctx->rg.table.ptr, (size_t)count * VP_REGION_WORDS * 8) : 0;
}

int vp_skeleton_table_host(vp_ctx* ctx, int algo, uint32_t* h_table)
{
    const char* who = "vp_skeleton_table_host";
    if (!h_table) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_algo(who, algo));
    if (!ctx) {
        skeleton_table_cpu(algo, h_table);
        return 0;
    }
    VP_TRY(bind_device(ctx));
    void* dt = nullptr;
    VP_TRY(vp_ctx_workspace(ctx, SLOT_SDF, (size_t)1 << 23, &dt));
    VP_TRY(launch_skeleton_table(ctx, algo, (uint32_t*)dt));
    return vp_download(ctx, h_table, dt, (size_t)1 << 23);
}

int vp_components_label_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_labels, int connectivity, int algo,
                             uint32_t* h_count)
{
    const char* who = "vp_components_label_host";
    if (!ctx || !h_words || !h_labels || !h_count) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_components(f, who, connectivity, algo));
    return host_round_trip(ctx, f, h_words, h_labels, SLOT_SDF,
                           [&](const uint32_t* dw, void* d) { return vp_components_label(ctx, f, dw, (uint32_t*)d, connectivity, algo, h_count); });
}

int vp_components_filter_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out, int connectivity, int mode,
                              uint32_t param, int algo, uint32_t* h_count, uint64_t* h_kept)
{
    const char* who = "vp_components_filter_host";
    if (!ctx || !h_words || !h_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_components(f, who, connectivity, algo));
    VP_TRY(check_filter_mode(who, mode, param));
    return host_round_trip(ctx, f, h_words, h_out, SLOT_GRID_B, [&](const uint32_t* dw, void* d) {
        return vp_components_filter(ctx, f, dw, (uint32_t*)d, connectivity, mode, param, algo, h_count, h_kept);
    });
}

int vp_surfnets_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t iterations, uint64_t* h_cells, float* h_xyz,
                     uint32_t* h_quads, size_t vertex_capacity, size_t quad_capacity, uint64_t* h_vertices, uint64_t* h_quads_out)
{
    const char* who = "vp_surfnets_host";
    if (!ctx || !h_words || !h_vertices || !h_quads_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_surfnets(f, who));
    if (iterations > 64) return set_error(VP_ERR_INVALID, "%s: %u iterations (0 .. 64)", who, iterations);
    const bool counts_only = !h_cells && !h_xyz && !h_quads;
    if (!counts_only && (!h_cells || !h_xyz || !h_quads)) return set_error(VP_ERR_INVALID, "%s: the three outputs go together", who);
    void *dw = nullptr, *dc = nullptr, *dx = nullptr, *dq = nullptr;
    const size_t wb = vp_grid_words(f) * 4;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_words, wb, &dw));
    uint64_t nv = 0, nq = 0;
    VP_TRY(vp_surfnets_count(ctx, f, (const uint32_t*)dw, VP_ALGO_TILED, &nv, &nq));
    if (!counts_only && (vertex_capacity < nv || quad_capacity < nq))
        return set_error(VP_ERR_INVALID, "%s: capacity %zu vertices / %zu quads, the grid has %llu / %llu", who, vertex_capacity, quad_capacity,
                         (unsigned long long)nv, (unsigned long long)nq);
    if (!counts_only && nv) {
        VP_TRY(vp_ctx_workspace(ctx, SLOT_GRID_B, nv * 8, &dc));         // the grid stays in slot A, so the count stands
        VP_TRY(vp_ctx_workspace(ctx, SLOT_XYZ, nv * 12, &dx));
        VP_TRY(vp_ctx_workspace(ctx, SLOT_TRI, nq * 16, &dq));
        VP_TRY(vp_surfnets(ctx, f, (const uint32_t*)dw, VP_ALGO_TILED, iterations, (uint64_t*)dc, (float*)dx, (uint32_t*)dq, nv, nq));
        VP_TRY(vp_download(ctx, h_cells, dc, nv * 8));
        VP_TRY(vp_download(ctx, h_xyz, dx, nv * 12));
        VP_TRY(vp_download(ctx, h_quads, dq, nq * 16));
    }
    *h_vertices = nv; *h_quads_out = nq;
    return 0;
}

int vp_isonets_host(vp_ctx* ctx, const vp_frame* f, const float* h_field, int transform, float iso, uint32_t iterations, int algo,
                    uint64_t* h_cells, float* h_xyz, float* h_normals, uint32_t* h_quads, size_t vertex_capacity, size_t quad_capacity,
                    uint64_t* h_vertices, uint64_t* h_quads_out)
{
    const char* who = "vp_isonets_host";
    if (!ctx || !f || !h_field || !h_vertices || !h_quads_out) return set_error(VP_ERR_INVALID, "%s: null argument", who);
    VP_TRY(check_isonets(f, who, transform, iso, iterations, algo));
    const bool counts_only = !h_cells && !h_xyz && !h_normals && !h_quads;
    if (!counts_only && (!h_cells || !h_xyz || !h_quads)) return set_error(VP_ERR_INVALID, "%s: records, positions and quads go together", who);
    void* df = nullptr;
    const size_t fb = vp_grid_voxels(f) * 4;
    VP_TRY(stage(ctx, SLOT_SDF, h_field, fb, &df));
    uint64_t nv = 0, nq = 0;
    VP_TRY(vp_isonets(ctx, f, (const float*)df, transform, iso, iterations, h_normals != nullptr, algo, &nv, &nq));
    if (!counts_only && (vertex_capacity < nv || quad_capacity < nq))
        return set_error(VP_ERR_INVALID, "%s: capacity %zu vertices / %zu quads, the field has %llu / %llu", who, vertex_capacity, quad_capacity,
                         (unsigned long long)nv, (unsigned long long)nq);
    if (!counts_only && nv) {
        VP_TRY(vp_download(ctx, h_cells, ctx->iso.cells.ptr, nv * 8));
        VP_TRY(vp_download(ctx, h_xyz, ctx->iso.xyz.ptr, nv * 12));
        if (h_normals) VP_TRY(vp_download(ctx, h_normals, ctx->iso.normals.ptr, nv * 12));
        VP_TRY(vp_download(ctx, h_quads, ctx->iso.quads.ptr, nq * 16));
    }
    *h_vertices = nv; *h_quads_out = nq;
    return 0;
}

int vp_csg_host(vp_ctx* ctx, uint32_t* h_a, const uint32_t* h_b, size_t nwords, int op)
{
    if (!ctx || ((!h_a || !h_b) && nwords)) return set_error(VP_ERR_INVALID, "vp_csg_host: null argument");
    void *da = nullptr, *db = nullptr;
    VP_TRY(stage(ctx, SLOT_GRID_A, h_a, nwords * 4, &da));
    VP_TRY(stage(ctx, SLOT_GRID_B, h_b, nwords * 4, &db));
    VP_TRY(vp_csg(ctx, (uint32_t*)da, (const uint32_t*)db, nwords, op));
    return vp_download(ctx, h_a, da, nwords * 4);
}

int vp_jfa_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, float fill_unset, float* h_sdf, int algo)
{
    if (!ctx || !h_words || !h_sdf) return set_error(VP_ERR_INVALID, "vp_jfa_host: null argument");
    VP_TRY(check_frame(f, "vp_jfa_host", true));
    return host_round_trip(ctx, f, h_words, h_sdf, SLOT_SDF,
                           [&](const uint32_t* dw, void* d) { return vp_jfa(ctx, f, dw, fill_unset, (float*)d, nullptr, 0, algo); });
}

// ---- profiling -------------------------------------------------------------------------------
int vp_prof_enable(vp_ctx* ctx, int on)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_prof_enable: null ctx");
    VP_TRY(bind_device(ctx));
    if (!on) VP_TRY(prof_fold(ctx));
    ctx->prof_on = on != 0;
    return 0;
}

int vp_prof_select(vp_ctx* ctx, uint64_t kernel_mask)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_prof_select: null ctx");
    ctx->prof_mask = kernel_mask;
    return 0;
}

int vp_prof_reset(vp_ctx* ctx)
{
    if (!ctx) return set_error(VP_ERR_INVALID, "vp_prof_reset: null ctx");
    VP_TRY(bind_device(ctx));
    VP_TRY(prof_fold(ctx));
    for (int i = 0; i < VP_K_ALL; ++i) { ctx->prof_ms[i] = 0; ctx->prof_n[i] = 0; }
    return 0;
}

int vp_prof_get(vp_ctx* ctx, int kernel, double* total_ms, uint64_t* launches)
{
    if (!ctx || kernel < 0 || kernel >= VP_K_ALL) return set_error(VP_ERR_INVALID, "vp_prof_get: bad argument");
    VP_TRY(bind_device(ctx));
    VP_TRY(prof_fold(ctx));
    if (total_ms) *total_ms = ctx->prof_ms[kernel];
    if (launches) *launches = ctx->prof_n[kernel];
    return 0;
}

const char* vp_prof_name(int kernel) { return (kernel >= 0 && kernel < VP_K_ALL) ? kNames[kernel] : "?"; }

}  // extern "C"
