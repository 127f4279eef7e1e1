/*
 * vphip.h -- C ABI of libvphip.so, the MI355X (gfx950) implementation of the reference's
 * voxelize -> CSG -> JFA hot path.
 *
 * The reference (bigmat18/cuda-mesh-voxelization) has no FFI layer: its boundary is the vplib
 * C++ template API.  Each entry point below names the reference interface it stands behind;
 * the C++ mirror of that API (cuda_mesh_voxelization_amd/vplib/) and the Python harness call
 * nothing but these functions.  All citations are file:line under the reference repo.
 *
 * Conventions
 *   - Every function returns 0 on success, otherwise a non-zero code (hipError_t value, or
 *     VP_ERR_* below) and stores a message retrievable with vp_last_error().  Nothing throws,
 *     nothing calls exit(): the C++ mirror turns a non-zero code into the reference's
 *     print-and-exit behaviour (vplib/src/debug_utils.h:43-50).
 *   - Pointers named d_* are device pointers (any hipMalloc'd / torch-owned memory of the
 *     context's device); h_* are host pointers.  The caller owns every buffer.
 *   - Work is enqueued on the context's stream and is asynchronous unless stated otherwise.
 *   - Grid layout is the reference's (vplib/src/grid/voxels_grid.h:116-129,
 *     vplib/src/grid/grid.h:89-92): voxel (x,y,z) is bit (x + y*n + z*n*n) of a little-endian
 *     uint32 word array, LSB first; dense fields (sdf) are x-fastest float arrays.
 *   - A vp_frame may describe a Z-slab [z0,z1) of the global n^3 grid: buffers then hold only
 *     those planes (plane z0 first).  z0 = 0, z1 = n is the whole grid.
 */
#ifndef VPHIP_H
#define VPHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_ABI_VERSION 6

enum {
    VP_OK = 0,
    VP_ERR_INVALID = 10001,     /* bad argument (null pointer, unsupported n, finite fill, ...) */
    VP_ERR_UNSUPPORTED = 10002, /* valid request this build cannot serve */
    VP_ERR_NOMEM = 10003
};

/* vplib/src/proc_utils.h:7-9  enum class Types {SEQUENTIAL, NAIVE, TILED, OPENMP}: the GPU values */
enum { VP_ALGO_NAIVE = 1, VP_ALGO_TILED = 2 };

/* vplib/src/csg/csg.h:10-12  enum class Op {VOID, UNION, INTERSECTION, DIFFERENCE} */
enum { VP_OP_VOID = 0, VP_OP_UNION = 1, VP_OP_INTERSECTION = 2, VP_OP_DIFFERENCE = 3 };

/* Grid frame: what VoxelsGrid carries besides its words (voxels_grid.h:39-43,160-169),
 * plus the Z-slab this buffer holds. */
typedef struct vp_frame {
    uint32_t n;           /* voxels per side of the GLOBAL grid (n % 32 == 0, 32 <= n <= 2048) */
    float    voxel_size;
    float    origin[3];
    uint32_t z0, z1;      /* planes held: z0 <= z < z1; multiples of 8 */
} vp_frame;

typedef struct vp_ctx vp_ctx;

/* ---- context ------------------------------------------------------------------------------
 * Replaces `cudaSetDevice(0)` + default stream + per-call cudaMalloc/cudaFree of the reference
 * (apps/cli/main.cpp:22-23, vplib/src/cuda_ptr.h:15-93).  The context owns a stream and a
 * grow-only workspace so that steady-state calls allocate nothing. */
int vp_device_count(int* out);                                    /* devices visible to the process */
int vp_ctx_create(int device, vp_ctx** out);
int vp_ctx_destroy(vp_ctx* ctx);
/* external != 0: enqueue on the caller's hipStream_t `hip_stream` (NULL = the device's null stream,
 * which is what torch's default stream is); external == 0: back to the context's own stream. */
int vp_ctx_set_stream(vp_ctx* ctx, void* hip_stream, int external);
int vp_ctx_sync(vp_ctx* ctx);
const char* vp_last_error(void);
int vp_abi_version(void);

/* ---- device memory (CudaPtr<T> equivalent, vplib/src/cuda_ptr.h:24-93) ---------------------
 * Alignment contract: every grid, id, sdf and workspace buffer handed to the entry points below must be 16-byte aligned -- what
 * hipMalloc, vp_malloc and the usual framework allocators return; the kernels move these buffers as 16-byte vectors.  A pointer
 * that is not is refused with VP_ERR_INVALID (slab planes inside such a buffer are aligned by construction: n % 32 == 0). */
int vp_malloc(vp_ctx* ctx, size_t bytes, void** d_out);
/* vp_free takes the base pointer of an allocation and counts as a write to ALL of it for the records a context keeps about caller
 * buffers (see vp_jfa_start): a record about a range anywhere inside the freed allocation is dropped. */
int vp_free(vp_ctx* ctx, void* d_ptr);
int vp_memset(vp_ctx* ctx, void* d_ptr, int byte_value, size_t bytes);           /* async */
/* CudaPtr's copy constructor / assignment: device-to-device deep copy (cuda_ptr.h:42-53).  async */
int vp_memcpy_d2d(vp_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* Measurement aid (no reference counterpart; SURVEY.md 8(d) asks for a stream-copy peak measured on the box): a plain 16-bytes-
 * per-lane grid-stride copy kernel on the context's stream -- the access shape of the CSG and prefix-XOR kernels with nothing
 * computed.  bench.py times it over 1 GiB and reports the HBM-bound kernels against that rate beside the 8 TB/s specification.
 * Buffers 16-byte aligned, bytes a multiple of 16.  async */
int vp_stream_copy(vp_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* Context-owned scratch: slot in [0, VP_WORKSPACE_SLOTS), grow-only, valid until the next call for the same slot
 * with a larger size, vp_ctx_release or vp_ctx_destroy.  What the Compute() wrappers use instead of the reference's
 * per-call cudaMalloc/cudaFree (vox/tiled.cu:496-575 allocates ~15 buffers per call). */
#define VP_WORKSPACE_SLOTS 8
int vp_ctx_workspace(vp_ctx* ctx, int slot, size_t bytes, void** d_out);
/* Frees every workspace slot and the JFA workspace (synchronises). */
int vp_ctx_release(vp_ctx* ctx);
int vp_upload(vp_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);        /* blocking */
int vp_download(vp_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);      /* blocking */

/* words in the buffer of a frame: n*n*(z1-z0)/32 */
size_t vp_grid_words(const vp_frame* f);
/* voxels in the buffer of a frame: n*n*(z1-z0) */
size_t vp_grid_voxels(const vp_frame* f);

/* ---- voxelize -----------------------------------------------------------------------------
 * Stands behind VOX::Compute<Types::NAIVE|TILED,T>(HostVoxelsGrid<T>&, const Mesh&)
 * (vplib/src/vox/vox.h:107-111, vox/naive.cu:86-122, vox/tiled.cu:488-576); the result is the
 * bitmask of VOX::Compute<Types::SEQUENTIAL> (vox/sequential.cpp:6-63).
 *   d_xyz   nverts x 3 float  (Mesh::Coords, mesh.h:133-170)
 *   d_tri   ntris x 3 uint32  (Mesh::FacesCoords; ntris = indices/3 as in sequential.cpp:16)
 *   accumulate = 0: d_words is overwritten (GPU variants of the reference replace the grid,
 *                   vox/tiled.cu:572-575); 1: XOR into the existing words (sequential semantics).
 * Asynchronous in steady state: list sizes stay on the device (no read-back, no stream synchronisation).  The FIRST call, and
 * any call that needs a larger internal buffer than the context has (grow-only), synchronises the stream and allocates:
 * the record list of large triangles (80 B each; 5 MiB, then what earlier calls counted + 25 %, at most one per triangle -- a
 * large triangle that finds it full is rasterised in place, so any size is correct), the tile work queue (>= 4 MiB, grows
 * the same way) and the 8 x 8-column tile tables. */
int vp_voxelize(vp_ctx* ctx, const vp_frame* f, uint32_t* d_words,
                const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris,
                int algo, int accumulate);

/* ---- conservative surface voxelization (no reference counterpart) ---------------------------
 * The reference promises "solid or surface voxel grids" (README) but has only the solid parity rule above, which needs a closed,
 * consistently crossed mesh; on an open mesh or a triangle soup its columns streak to the grid edge.  This voxelizer sets voxel
 * (i, j, k) iff its CLOSED box overlaps the CLOSED triangle (Schwarz & Seidel 2010, section 3.1: the 26-separating test).  In float32,
 * in this association, without FMA contraction (the contract):
 *   corner      p.a = o.a + (float)idx * vs
 *   setup       e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2;  nrm = Cross(e0, e1).  A triangle contributes NOTHING if an index is >= nverts,
 *               a vertex coordinate is not finite, or nrm == (0, 0, 0).
 *   box         p.a <= max.a && p.a + vs >= min.a on every axis (min / max of the three vertices)
 *   plane       c.a = nrm.a > 0 ? vs : 0;  d1 = Dot(nrm, c - v0), d2 = Dot(nrm, (vs - c) - v0), Dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 *               t = Dot(nrm, p), s1 = t + d1, s2 = t + d2; the voxel fails if (s1 > 0 && s2 > 0) || (s1 < 0 && s2 < 0)
 *   projections (u, v) = (x, y), (y, z), (z, x) with sigma = (nrm.z, nrm.x, nrm.y) >= 0 ? 1 : -1; for each edge e_i starting at v_i:
 *               ne = (-e_i.v * sigma, e_i.u * sigma), de = ((-(ne.u v_i.u + ne.v v_i.v)) + max(0, vs ne.u)) + max(0, vs ne.v)
 *               (max(0, x) = x > 0 ? x : 0); the voxel passes iff (ne.u p.u + ne.v p.v) + de >= 0 for all nine
 * accumulate = 0: d_words is overwritten (zero-fill, then OR); 1: OR into the existing words (a union -- not the XOR of vp_voxelize).
 * Slab frames are served: a slab's words are those planes of the whole-grid result.  Argument checks as vp_voxelize.
 * VP_ALGO_NAIVE: one thread per triangle, one atomicOr per set voxel.  VP_ALGO_TILED: small triangles rasterised by their setup
 * thread (one atomicOr per touched word), the rows of large ones dealt to lanes over the whole device.  Same bits.
 * Asynchronous in steady state; the first call, and any call that needs a larger large-triangle list than the context has (grow-only,
 * 64 Ki records of 176 B or what earlier calls counted + 25 %, a large triangle that finds it full is walked in place), synchronises
 * and allocates. */
int vp_voxelize_conservative(vp_ctx* ctx, const vp_frame* f, uint32_t* d_words,
                             const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris,
                             int algo, int accumulate);

/* ---- interior fill (no reference counterpart) -----------------------------------------------
 * Turns a grid into a solid by filling every enclosed empty region.  A voxel is EXTERIOR if it is not set in d_words and either lies
 * on the grid boundary (x, y or z in {0, n-1}) or is face-adjacent (6-connectivity) to an exterior voxel; d_out = NOT exterior, i.e.
 * d_words plus every empty voxel the boundary cannot reach (scipy.ndimage.binary_fill_holes with its default structure).  The
 * conservative grid above is 26-separating, so a 6-connected flood cannot cross a surface that is closed at voxel scale: filling it
 * gives the solid of an open mesh whose holes are smaller than a voxel, or of a soup that covers a closed surface (DESIGN.md
 * section 10).  No connectivity option.
 *   Whole-grid frames only: a slab frame (z0 != 0 || z1 != n) returns VP_ERR_UNSUPPORTED.  d_out must not overlap d_words
 *   (VP_ERR_INVALID); both 16-byte aligned.  Every refusal leaves d_out untouched.
 *   h_rounds (may be NULL) receives the number of propagation rounds that ran -- one round sweeps x, y and z -- including the final
 *   round that changed nothing.
 * BLOCKING: rounds are enqueued in batches and their convergence flags read back once per batch; when the call returns, d_out is
 * complete and the stream is idle.  It cannot be captured in a graph.  The flags (a few words, grow-only) belong to the context. */
int vp_fill_interior(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, uint32_t* h_rounds);

/* ---- ball morphology: dilate, erode, open, close (no reference counterpart) --------------------
 * B_r = {(dx, dy, dz) in Z^3 : dx^2 + dy^2 + dz^2 <= r^2}, integer r; everything below is integer arithmetic.
 *   VP_MORPH_DILATE  voxel p is set iff some d in B_r has p - d inside the grid and set: voxels outside the grid read as EMPTY, the
 *                    result is clipped to the grid (scipy.ndimage.binary_dilation(W, structure=ball, border_value=0)).
 *   VP_MORPH_ERODE   NOT dilate(NOT W, r): voxels outside the grid read as SET (scipy.ndimage.binary_erosion(W, structure=ball,
 *                    border_value=1)).  The frame is the tight bounding box, so meshes touch the grid faces; a border of 0 would eat
 *                    them.  With these two borders (dilate, erode) is an adjunction on the grid lattice, hence:
 *   VP_MORPH_OPEN    dilate(erode(W)): idempotent, a subset of W (removes specks thinner than the ball).
 *   VP_MORPH_CLOSE   erode(dilate(W)): idempotent, a superset of W.
 *   radius 0 copies the grid; 1 .. 32 is served (the x reach stays inside the two neighbouring words); above 32: VP_ERR_UNSUPPORTED.
 * REPAIRING AN OPEN SHELL: vp_fill_interior needs holes smaller than a voxel.  For holes up to about 2 R voxels wide:
 *     dilate(conservative grid, R)  ->  vp_fill_interior  ->  erode(., R)
 * The dilation plugs the hole, the fill makes the solid, the erosion puts the outer surface back where it was (a shallow dimple of at
 * most about k^2 R voxels remains behind a k x k hole).  CLOSE IS NOT THAT RECIPE: fill(close(W, R)) still leaks, because the erosion
 * inside close runs BEFORE the fill and re-opens the plug from the side -- the plug is thinner than the ball.
 *   Whole-grid frames only: a slab frame (z0 != 0 || z1 != n) returns VP_ERR_UNSUPPORTED.  d_out must not overlap d_words
 *   (VP_ERR_INVALID); both 16-byte aligned.  Null pointers, an unknown op, an unknown algo: VP_ERR_INVALID.  Every refusal leaves
 *   d_out untouched.
 *   algo: VP_ALGO_NAIVE -- one thread per output word, every row of the ball x-dilated by its own half-width; VP_ALGO_TILED -- the rows
 *   folded in by Horner over the half-widths, tiles staged in LDS.  Same bits.
 * Open and close run two passes through an intermediate grid of n^3/8 bytes, a grow-only buffer of the context.  ASYNCHRONOUS in steady
 * state: the call only enqueues kernels on the context's stream; the call that first grows a buffer of the context may synchronise.
 * Like every writer of a grid, it drops a pending vp_jfa_start whose words (or workspace) d_out overlaps. */
enum { VP_MORPH_DILATE = 0, VP_MORPH_ERODE = 1, VP_MORPH_OPEN = 2, VP_MORPH_CLOSE = 3 };
int vp_morph(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo);

/* ---- exact Euclidean distance transform (no reference counterpart) ------------
 * Integer arithmetic only: d_dist2[x + n (y + n z)] = the minimum over the SEED voxels q of |p - q|^2 in voxel units, one uint32 per voxel
 * (4 n^3 bytes, x fastest like the sdf); VP_EDT_NONE where the grid has no seed at all.  The largest value is 3 * 1023^2, exact in float.
 *   VP_EDT_SEEDS_SET     the set voxels
 *   VP_EDT_SEEDS_UNSET   the unset voxels
 *   VP_EDT_SEEDS_BORDER  the JFA's seeds (vp_surface): set voxels with an unset 26-neighbour or a 26-neighbour outside the grid
 * Voxels outside the grid are never seeds.
 *   vp_edt        the transform above.
 *   vp_edt_sdf    the exact counterpart of vp_jfa: D = the SEEDS_BORDER transform, sdf = +-((float)D * (voxel_size * voxel_size)) --
 *                 the product formed once in float, then one conversion and one multiply -- positive on set voxels, negative on unset
 *                 ones; a grid without seeds (the empty grid) gives fill_unset everywhere.  fill_unset must be +-infinity.  D lives in
 *                 d_sdf and is converted in place.  Same sign bits and the same zeros as vp_jfa; |vp_jfa| >= |vp_edt_sdf| everywhere.
 *   vp_edt_morph  vp_morph's four ops with its two border rules, radius 0 .. 65535: dilate = D_SET <= r^2, erode = D_UNSET > r^2 (outside
 *                 reads as set: it is never a seed), open = dilate(erode), close = erode(dilate); radius 0 copies; radius > 65535:
 *                 VP_ERR_INVALID.  The distance volume (4 n^3 bytes) and the intermediate grid are grow-only buffers of the context.
 * Three separable passes: x straight from the bit words (nearest seed bit left and right), then y and z as out(i) = min_j g(j) + (i - j)^2.
 *   algo: VP_ALGO_NAIVE -- column passes with one thread per voxel from global memory into a second 4 n^3 volume of the context;
 *   VP_ALGO_TILED -- whole columns of a bundle of adjacent x staged in LDS, written back in place (no second volume).  Same bytes.
 * Whole-grid frames only: a slab frame returns VP_ERR_UNSUPPORTED; so does n > 1024 (the volume would be 32 GiB).  The outputs must not
 * overlap d_words; every buffer is 16-byte aligned.  Null pointers, unknown seeds / op / algo: VP_ERR_INVALID.  Every refusal leaves the
 * outputs untouched.  The calls only enqueue work once the context's buffers have grown (the border mask n^3/8, NAIVE's second volume,
 * vp_edt_morph's distance volume and intermediate grid; the volumes are freed by vp_ctx_release).  Like every writer, they drop a pending
 * vp_jfa_start / extract / surfnets count whose bytes the output overlaps. */
enum { VP_EDT_SEEDS_SET = 0, VP_EDT_SEEDS_UNSET = 1, VP_EDT_SEEDS_BORDER = 2 };
#define VP_EDT_NONE 0xFFFFFFFFu
int vp_edt(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int seeds, uint32_t* d_dist2, int algo);
int vp_edt_sdf(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, float fill_unset, float* d_sdf, int algo);
int vp_edt_morph(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, int op, uint32_t radius, int algo);

/* ---- narrow-band distance to the triangles of a mesh, with the nearest face (no reference counterpart) ----------
 * vp_jfa and vp_edt_sdf measure from voxel centre to the centre of the nearest border VOXEL; this field is measured to the TRIANGLES.
 * Everything is float32, every operation one correctly rounded IEEE operation in the association written here, no FMA contraction (the
 * library is built with -ffp-contract=off); the branch conditions are part of the contract.  Dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 *   sample point  p = the voxel centre as vp_voxelize forms it: p.a = o.a + (((float)i * vs) + (vs / 2.0f))
 *   triangle      a, b, c = its three vertices in index order.  It contributes NOTHING if an index is >= nverts, a vertex coordinate is not
 *                 finite, or Cross(e0, e1) == (0, 0, 0) with e0 = b - a, e1 = c - b in the association of vp_voxelize_conservative.
 *   D2(p, t)      the region walk of Ericson, Real-Time Collision Detection 5.1.5, to the closest point q of the closed triangle:
 *                   ab = b - a, ac = c - a, ap = p - a;  d1 = Dot(ab, ap), d2 = Dot(ac, ap);      d1 <= 0 && d2 <= 0:  q = a
 *                   bp = p - b;  d3 = Dot(ab, bp), d4 = Dot(ac, bp);                              d3 >= 0 && d4 <= d3:  q = b
 *                   vc = (d1 d4) - (d3 d2);      vc <= 0 && d1 >= 0 && d3 <= 0:  v = d1 / (d1 - d3),  q.a = a.a + (ab.a v)
 *                   cp = p - c;  d5 = Dot(ab, cp), d6 = Dot(ac, cp);                              d6 >= 0 && d5 <= d6:  q = c
 *                   vb = (d5 d2) - (d1 d6);      vb <= 0 && d2 >= 0 && d6 <= 0:  w = d2 / (d2 - d6),  q.a = a.a + (ac.a w)
 *                   va = (d3 d6) - (d5 d4), e43 = d4 - d3, e56 = d5 - d6;
 *                                                va <= 0 && e43 >= 0 && e56 >= 0:  w = e43 / (e43 + e56),  q.a = b.a + ((c.a - b.a) w)
 *                   otherwise the face: den = (va + vb) + vc, v0 = vb / den, w0 = vc / den;  v = v0 > 0 ? v0 : 0, then v = v < 1 ? v : 1;
 *                                                wl = 1 - v;  w = w0 > 0 ? w0 : 0, then w = w < wl ? w : wl;  q.a = (a.a + (ab.a v)) + (ac.a w)
 *                 the first condition that holds decides, in this order.  The two clamps of the face are the identity in exact arithmetic
 *                 (there 0 < v0, 0 < w0, v0 + w0 < 1); in float they keep q inside the triangle when rounding has left va, vb, vc with mixed
 *                 signs, which is what lets every culling below be proved.  A comparison with a NaN is false.
 *                 Then d = p - q and D2 = (d.x d.x + d.y d.y) + d.z d.z.
 *   band          B = (float)band * vs, B2 = B * B; band = 1 .. 32 voxels, anything else: VP_ERR_INVALID.  A candidate whose D2 is not
 *                 finite, or for which D2 < B2 does not hold, is dropped: a centre at distance exactly B is NOT within the band.
 *   field         m(p) = min(B2, the minimum of D2(p, t) over the candidates);  d_dist2[x + n (y + n z)] = s m(p), squared world units like
 *                 the sdf; s = +1 everywhere when d_sign_words is NULL (unsigned field), otherwise +1 on the set voxels of that grid and -1
 *                 on the unset ones (the sign convention of vp_jfa and vp_edt_sdf; a zero distance on an unset voxel is -0.0f).
 *   nearest face  d_nearest[...] (may be NULL) = the lowest triangle index among the candidates that attain m(p), VP_MESH_NONE where there
 *                 is no candidate: the lexicographic minimum of (D2 bits, index).  Ties are the normal case -- every triangle around a
 *                 shared vertex returns that vertex bit for bit.  ntris = 0 gives s B2 and VP_MESH_NONE everywhere.
 * A min over a set: the result does not depend on the order of evaluation, nor on which pairs were culled -- candidate ranges never decide a
 * value, they only skip pairs that provably fail D2 < B2 as computed in float32.
 * THE SIGN is whatever grid the caller passes.  With vp_voxelize's grid it is the reference's column rule: a voxel is set from the cell
 * that CONTAINS the crossing, not from the first centre behind it, so along x a centre up to half a voxel outside the surface can carry +.
 * That is a property of the reference's solid rule, not of this field; a caller who needs a centre-exact sign passes a grid of their own
 * (vp_winding below builds one from the mesh).
 *   algo: VP_ALGO_NAIVE -- one thread per triangle over the voxels of its band box, one 64-bit atomicMin per accepted pair on the key
 *   (D2 bits << 32) | index, then a streaming split; VP_ALGO_TILED -- triangles binned to 8 x 8 x 8-voxel bricks (count, scan, write; the
 *   brick rows of large triangles dealt to lanes), one workgroup per brick with the records staged through LDS, (D2, index) in registers,
 *   one plain store per voxel; bricks without a list by a streaming fill.  Same bytes.
 * Whole-grid frames only: a slab frame returns VP_ERR_UNSUPPORTED; so does n > 1024.  Every buffer is 16-byte aligned; the outputs must not
 * overlap the inputs or each other.  Null ctx / f / d_dist2, null mesh arrays with ntris > 0, an unknown algo, band 0 or above 32:
 * VP_ERR_INVALID.  Every refusal leaves the outputs untouched.
 * VP_ALGO_TILED is BLOCKING once per call: the list lengths of the brick planes (n / 8 totals) are read back to size the lists, so it
 * cannot be captured in a graph; VP_ALGO_NAIVE only enqueues once its buffer has grown.  Grow-only buffers of the context, all freed by
 * vp_ctx_release: the key volume of NAIVE (8 n^3 bytes), the triangle records (96 B each), their row counts and row scan (12 B per
 * triangle), the brick counts, write cursors and offsets (16 B per brick, plus 8 B per plane of bricks) and the brick lists (4 B per entry; at most 2^27 entries per launch -- a grid whose lists are longer runs in several z
 * ranges of bricks, a single plane of bricks above the cap being a range of its own).  Like every writer, it drops a pending
 * vp_jfa_start / extract / surfnets count whose bytes an output overlaps.
 * vp_mesh_distance_stats: *list_entries = the (triangle, brick) pairs the last VP_ALGO_TILED call of this context listed (512 pairs of
 * (triangle, voxel) each reach the per-pair bounds).  Measurement only. */
#define VP_MESH_NONE 0xFFFFFFFFu
int vp_mesh_distance(vp_ctx* ctx, const vp_frame* f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris,
                     const uint32_t* d_sign_words /* may be NULL */, uint32_t band, float* d_dist2, uint32_t* d_nearest /* may be NULL */,
                     int algo);
int vp_mesh_distance_stats(vp_ctx* ctx, uint64_t* list_entries);

/* ---- connected components: labels, sizes, size filters (no reference counterpart) ----------------
 * Set voxels are the foreground, voxels outside the grid are empty.  connectivity: VP_CONN_6 (face neighbours) or VP_CONN_26 (face, edge
 * and corner neighbours) = scipy.ndimage.generate_binary_structure(3, 1) and (3, 3).  Integer arithmetic only.
 *   vp_components_label   d_labels: one uint32 per voxel, x fastest like the sdf (4 n^3 bytes); 0 = background; components are numbered
 *                         1 .. K in increasing order of their lowest linear voxel index x + n (y + n z), so the volume equals
 *                         scipy.ndimage.label(vox_zyx, structure)[0] element for element.  *h_count = K.  Needs no second volume: d_labels is
 *                         the parent array of a lock-free union-find while the call runs.
 *   vp_components_sizes   d_sizes[k - 1] = voxels of component k, for the `count` = K components of a label volume (labels above count are
 *                         ignored; count = 0 writes nothing).  d_sizes holds count uint32.
 *   vp_components_filter  bit grid -> bit grid.  VP_COMP_KEEP_LARGEST, param = m in 1 .. 16: the m largest components stay (all if K <= m;
 *                         ties go to the lower label).  VP_COMP_MIN_VOXELS, param = v: the components with at least v voxels stay (v = 0
 *                         and v = 1 copy the grid).  *h_count = K, *h_kept = voxels set in d_out (either may be NULL).  An empty grid gives
 *                         K = 0 and an empty d_out, not an error.  The label volume is a grow-only buffer of the context (4 n^3 bytes:
 *                         4 GiB at n = 1024), which vp_ctx_release frees.
 *   Whole-grid frames only: a slab frame returns VP_ERR_UNSUPPORTED; so does n > 1024 (voxel indices need 33 bits there and the label
 *   volume would be 32 GiB).  d_labels / d_out must not overlap d_words, and every buffer is 16-byte aligned.  Null pointers, an unknown
 *   connectivity, mode or algo, m outside 1 .. 16: VP_ERR_INVALID.  Every refusal leaves the outputs untouched.
 *   algo: VP_ALGO_NAIVE -- one thread per voxel, one union per set backward neighbour; VP_ALGO_TILED -- trees start as whole x runs and
 *   the merge makes one union per pair of adjacent runs.  Same labels: a component's root is its lowest voxel index whatever the order
 *   of execution.
 * BLOCKING: all three return when the work is complete and the stream is idle (K and the kept count come back through a pinned host
 * word of the context; vp_components_filter also reads K once midway, to size its per-component arrays).  They cannot be captured in a
 * graph.  Like every writer of a grid, they drop a pending vp_jfa_start or extract count whose bytes d_labels / d_sizes / d_out overlap. */
enum { VP_CONN_6 = 6, VP_CONN_26 = 26 };
enum { VP_COMP_KEEP_LARGEST = 0, VP_COMP_MIN_VOXELS = 1 };
int vp_components_label(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_labels, int connectivity, int algo,
                        uint32_t* h_count);
int vp_components_sizes(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_labels, uint32_t count, uint32_t* d_sizes);
int vp_components_filter(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t* d_out, int connectivity, int mode,
                         uint32_t param, int algo, uint32_t* h_count, uint64_t* h_kept);

/* ---- surface nets: a closed quad mesh from a bit grid (Gibson 1998; no reference counterpart) ----------------
 * Grid and cells.  Voxel (x, y, z) occupies the lattice cube [x, x+1]^3, its centre is at x + 0.5; voxels outside the grid are empty.  A
 * CELL (cx, cy, cz), each coordinate in -1 .. n-1, is the cube whose eight corners are the centres of the voxels (cx+dx, cy+dy, cz+dz),
 * d in {0, 1}: (n+1)^3 cells, linear cell index (cx+1) + (n+1) ((cy+1) + (n+1) (cz+1)).  Bit dx + 2 dy + 4 dz of the 8-bit CORNER MASK is
 * set iff that voxel is set; a cell is ACTIVE iff its mask is neither 0 nor 255.
 * Vertices.  One per active cell, numbered 0 .. V-1 in increasing linear cell index.  Record (d_cells): cell index | corner mask << 40,
 * the shape of the vp_extract record.
 * Positions (d_xyz): float32 x 3 per vertex, in LATTICE coordinates (voxel units; the frame's origin and voxel size are not applied).
 * Before relaxation, over the cell's twelve edges in local coordinates 0 .. 1: m = the edges whose two corners differ, S_a = the sum over
 * those edges of twice the midpoint's coordinate a (each term 0, 1 or 2);  p_a = ((float)c_a + 0.5f) + (float)S_a / (float)(2 m) -- the
 * correctly rounded float quotient, then one float add.  Every component lies strictly inside (c_a + 0.5, c_a + 1.5).
 * Quads (d_quads): uint32 x 4 vertex indices, one quad per pair of face-adjacent voxels of which exactly one is set (outside = unset).
 * The quad is owned by the cell that has the edge between the two voxel centres as one of the three edges leaving its corner 0 towards
 * +x, +y or +z (always active, always inside the cell range); quads are ordered by owner cell index, then by axis x, y, z.  With the
 * owner (i, j, k) = (cx, cy, cz) the four vertices are those of the cells
 *     x-edge: (i, j-1, k-1), (i, j, k-1), (i, j, k), (i, j-1, k)
 *     y-edge: (i-1, j, k-1), (i-1, j, k), (i, j, k), (i, j, k-1)
 *     z-edge: (i-1, j-1, k), (i, j-1, k), (i, j, k), (i-1, j, k)
 * in that order when the LOWER voxel of the pair is the set one (the outward normal points along + axis), reversed (d, c, b, a) when the
 * upper one is.  Triangles, where needed, are (a, b, c) and (a, c, d).  Q equals the number of faces vp_extract reports in
 * VP_EXTRACT_EXPOSED mode; the surface is closed: every directed edge (a, b) occurs as often as (b, a).
 * Relaxation.  iterations = 0 .. 64 Jacobi steps (each reads the previous buffer and writes the other).  The neighbours of a vertex are
 * the cells across the faces -x, +x, -y, +y, -z, +z, in that order; a neighbour across a face exists iff that face's four corners are
 * mixed (both cells are then active; an active cell has at least two such faces).  Per component: acc = the first neighbour's value, the
 * others added left to right in float; q = acc / (float)deg, correctly rounded; then q = min(max(q, lo), hi) with lo = (float)c_a +
 * 0.5625f, hi = (float)c_a + 1.4375f -- the cell shrunk by 1/16, exact in float for every served n.  Vertices never leave their cell.
 * Every operation is one IEEE operation in a prescribed order (the library is built with -ffp-contract=off), so records, quads and
 * positions are the same bits for both algos and for the host restatement.
 *   vp_surfnets_count   *h_vertices = V, *h_quads = Q.  BLOCKING (the totals are read back); cannot be captured in a graph.
 *   vp_surfnets         writes V records, V positions and Q quads and runs the relaxation; the result ends in d_xyz for any iteration
 *                       count.  It must follow a vp_surfnets_count of the same grid CONTENTS, frame side and algo ("same grid" as for
 *                       vp_extract: the count is dropped as soon as any output of any call of this ABI lands on any part of the
 *                       grid -- the rule stated at vp_jfa_start); otherwise, or with a capacity
 *                       below V / Q: VP_ERR_INVALID.  Enqueues only, once the context's buffers have grown.  The outputs must not overlap
 *                       d_words; d_cells / d_xyz / d_quads may be NULL only when V (Q) is 0.
 * Scratch memory is the context's: the rank lookup (VP_ALGO_NAIVE: a uint32 vertex-index volume, 4 (n+1)^3 bytes -- 4.3 GB at n = 1024;
 * VP_ALGO_TILED: active-cell bits and one exclusive count per 32 cells, about n^3/4 bytes) and the second position buffer (12 V bytes),
 * grow-only, freed by vp_ctx_release.
 * Whole-grid frames only: a slab frame returns VP_ERR_UNSUPPORTED; so does n > 1024 ((n+1)^3 stays below 2^31).  Null pointers, an unknown
 * algo and iterations > 64: VP_ERR_INVALID.  Every refusal leaves the outputs untouched.
 *   algo: VP_ALGO_NAIVE -- one thread per cell reads its eight voxel bits one by one; VP_ALGO_TILED -- one lane per 32 cells of a cell row,
 *   corner words from two words of each of four voxel rows.  Same bytes. */
int vp_surfnets_count(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint64_t* h_vertices, uint64_t* h_quads);
int vp_surfnets(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint32_t iterations, uint64_t* d_cells, float* d_xyz,
                uint32_t* d_quads, size_t vertex_capacity, size_t quad_capacity);

/* ---- iso-surface nets: surface nets of a scalar field at an iso level (no reference counterpart) ----------------
 * The mesh of the surface-nets section above, taken from a float field instead of a bit grid: vertices are placed by the field's edge
 * crossings (sub-voxel), normals come from its gradient.  Lattice coordinates, cells, corner masks, the record cell index | mask << 40,
 * vertex order, quad ownership, order and winding, and the relaxation are EXACTLY those of the surface-nets section, applied to the
 * INSIDE set defined below: the topology is that of a bit grid, so the mesh is always closed.  Only "inside", the starting positions
 * and the normals are new.  Everything is float32; every operation written is one correctly rounded IEEE operation, in the association
 * written, without contraction.
 * Value.  d_field: n^3 floats, x fastest, the value v at each voxel centre.  transform = VP_ISO_LINEAR: g = v.  transform =
 * VP_ISO_SIGNED_SQUARE: g = copysignf(sqrtf(fabsf(v)), v) -- the convention of every sdf of this library (squared world units, + on set
 * voxels).  h = g - iso, one subtraction; iso must be finite.  A voxel outside the grid has h = NaN.
 * Inside.  A voxel is inside iff the bit pattern of h, read as uint32, is <= 0x7F800000: +0 .. +inf.  -0, negatives and every NaN are
 * outside.  So at iso 0 a field signed by a grid (+0.0f on set border voxels, -0.0f on unset ones) has exactly that grid as its inside set.
 * Position.  The twelve edges of a cell are visited by axis x, y, z and per axis by the lower corners c = 0 .. 7 that have the axis bit
 * clear, ascending.  For a crossing edge (its ends differ in "inside") with lower corner c and upper corner d:  t = h[c] / (h[c] - h[d]);
 * if !(t >= 0 && t <= 1) then t = 0.5f (0/0, inf/inf, corners outside the grid).  The edge's point has coordinate t on its own axis and
 * (float)((c >> a) & 1) on the other two.  Per component a: acc starts at +0.0f, the points of the crossing edges are added left to
 * right; q = acc / (float)m with m the number of crossing edges; p_a = ((float)c_a + 0.5f) + q.  Every component lies in the closed
 * interval [c_a + 0.5, c_a + 1.5].
 * Normals (optional).  With h0 .. h7 the corner values:
 *     G_x = ((h1-h0) + (h3-h2)) + ((h5-h4) + (h7-h6))
 *     G_y = ((h2-h0) + (h3-h1)) + ((h6-h4) + (h7-h5))
 *     G_z = ((h4-h0) + (h5-h1)) + ((h6-h2) + (h7-h3))
 * L2 = (G_x G_x + G_y G_y) + G_z G_z.  If !(L2 > 0) or L2 is infinite the normal is (0, 0, 0) -- every cell with a corner outside the grid
 * is such a cell.  Otherwise L = sqrtf(L2) and N_a = (-G_a) / L: inside is positive, so -G points outward.  Normals belong to the
 * unrelaxed cell; the relaxation does not change them.
 * Relaxation.  iterations = 0 .. 64 Jacobi steps of the surface-nets section, unchanged, with the same clamp; they start from the
 * positions above.
 * Degenerate facts.  A field that is +0.0f on the set and -0.0f on the unset voxels of a grid (or +inf / -inf likewise) gives, at iso 0,
 * the BYTES of the surface nets of that grid for records, positions and quads: every t is 0.5 and every sum is exact.  A single inside
 * voxel with h = +1 among h = -3 gives 8 vertices: every crossing lies 1/4 of an edge from the voxel, so each vertex sits (1/4 + 0 + 0) / 3 = 1/12 from the voxel centre
 * per axis, where the bit grid puts it at 1/6.
 *   vp_isonets          builds the whole mesh into grow-only buffers that the CONTEXT owns: records (8 V bytes), positions (12 V),
 *                       normals (12 V, only if want_normals != 0) and quads (16 Q).  BLOCKING: V and Q are read back and returned
 *                       (h_vertices / h_quads may be NULL).  The buffers stay valid until the next vp_isonets, vp_ctx_release or
 *                       vp_ctx_destroy.  Scratch (rank lookup, second position buffer) is shared with the surface-nets calls, so the
 *                       call DROPS a pending surface-nets count, as a second count would: the write call that follows is refused
 *                       with VP_ERR_INVALID and never served from overwritten scratch.
 *   vp_isonets_result   pointers and counts of the last build; any argument may be NULL.  Before any build, after a release and after a
 *                       build that failed half way: V = Q = 0 and NULL pointers.  *d_normals is NULL when the build did not ask for normals.
 *   vp_isonets_host     host in, host out, with the convention of the surface-nets host call: all four outputs NULL = counts only; a
 *                       capacity below V / Q: VP_ERR_INVALID (found after the build: the context then holds the new mesh); h_normals alone may be
 *                       NULL.  The field is staged through a workspace slot.
 * Whole-grid frames only: a slab frame and n > 1024 return VP_ERR_UNSUPPORTED.  Null ctx / f / d_field, a field that is not 16-byte
 * aligned, an unknown transform or algo, a non-finite iso and iterations > 64: VP_ERR_INVALID.  A refusal leaves the previous result and
 * its counts as they were.
 *   algo: VP_ALGO_TILED -- the field is streamed once into the inside grid (one ballot = 64 bits), the surface-nets launches run on that
 *   grid, then one lane per vertex gathers its eight corner values and recomputes h (no n^3 float volume is kept); VP_ALGO_NAIVE -- one
 *   thread per 32 voxels classifies them one by one, and one thread per cell places its vertex from its own eight field values through
 *   the index volume.  Same bytes.  Timing: classification books under VP_K_SN_CELLS(_NAIVE), placement under VP_K_SN_VERTS(_NAIVE). */
enum { VP_ISO_LINEAR = 0, VP_ISO_SIGNED_SQUARE = 1 };
int vp_isonets(vp_ctx* ctx, const vp_frame* f, const float* d_field, int transform, float iso, uint32_t iterations,
               int want_normals, int algo, uint64_t* h_vertices, uint64_t* h_quads);
int vp_isonets_result(vp_ctx* ctx, uint64_t** d_cells, float** d_xyz, float** d_normals, uint32_t** d_quads,
                      uint64_t* h_vertices, uint64_t* h_quads);
int vp_isonets_host(vp_ctx* ctx, const vp_frame* f, const float* h_field, int transform, float iso, uint32_t iterations, int algo,
                    uint64_t* h_cells, float* h_xyz, float* h_normals, uint32_t* h_quads, size_t vertex_capacity, size_t quad_capacity,
                    uint64_t* h_vertices, uint64_t* h_quads_out);

/* ---- generalized winding number: inside / outside from the mesh itself (no reference counterpart) ----------------
 * w(p) = (1 / 4 pi) sum over the valid triangles t of the signed solid angle Omega_t(p) (Jacobson et al. 2013), with the dipole far field
 * of Barill et al. 2018 over a pyramid of bricks.  w is 1 inside a closed mesh whose triangles are counter-clockwise seen from outside, 0
 * outside it, k where k shells overlap, -1 inside an inverted shell, and varies smoothly through an open boundary.
 * Everything below is float32 unless a cast says otherwise; every operation written is one correctly rounded IEEE operation in the
 * association written, no contraction.  Dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;  max2(a, b) = a > b ? a : b.
 *   sample point  p = the voxel centre as vp_voxelize forms it: p.a = o.a + (((float)i * vs) + (vs / 2.0f))
 *   triangle      v0, v1, v2 in index order; valid as for vp_mesh_distance: every index < nverts, every coordinate finite, and
 *                 nrm = Cross(e0, e1) != (0, 0, 0) with e0 = v1 - v0, e1 = v2 - v1 in the association of vp_voxelize_conservative.
 *   exact term    a = v0 - p, b = v1 - p, c = v2 - p;  la = sqrtf(Dot(a, a)), lb, lc likewise;
 *                 x = ((b.y c.z) - (b.z c.y), (b.z c.x) - (b.x c.z), (b.x c.y) - (b.y c.x));  det = Dot(a, x);
 *                 den = ((((la lb) lc) + (Dot(a, b) lc)) + (Dot(b, c) la)) + (Dot(c, a) lb);  Omega = 2.0f * atan2w(det, den)
 *                 (Van Oosterom & Strackee 1983).  A pair with det == 0, or with det or den not finite, contributes 0: p on a vertex, p in the
 *                 triangle's plane -- the principal value, so a centre on the surface reads about 1/2.
 *   atan2w(y, x)  the library's own, no libm: ax = fabsf(x), ay = fabsf(y);  t = min(ax, ay) / max(ax, ay);  s = t t;
 *                 q = C9;  q = (q s) + C8;  ...  q = (q s) + C0  (VP_WN_ATAN_C* below);  r = q t;
 *                 ay > ax: r = VP_WN_HALF_PI - r;  then x < 0: r = VP_WN_PI - r;  then y < 0: r = -r.
 *   far term      of a node with centre c and area vector N:  d = c - p;  r2 = Dot(d, d);  Omega = Dot(d, N) / (r2 * sqrtf(r2)); dropped (0)
 *                 if not finite.
 *   sum           every term is quantised before it is added: q = llrint((double)Omega * 2^36) (round to nearest even), S = the sum of the q
 *                 modulo 2^64, read as a two's complement int64;  w = (float)(((double)S * 2^-36) / VP_WN_FOUR_PI);  inside = (w >= level).
 *                 Integer addition is associative: the result does not depend on the order of the triangles, on atomics or on lists.
 *                 |Omega| < 2^3, so the sum of up to 2^24 terms cannot wrap; vp_winding admits up to (2^32 - 1) / 3 triangles, and above
 *                 2^24 the forms still agree bit for bit (every form adds modulo 2^64), but w is meaningful only while the true sum
 *                 stays below 2^63 -- always, for a mesh whose winding number is below 2^24 in absolute value.
 * THE HIERARCHY decides which terms exist and is part of the contract.  nb = n / 8.
 *   leaves        the 8 x 8 x 8-voxel bricks of vp_mesh_distance.  A valid triangle belongs to ONE leaf, that of its centroid:
 *                 g.a = ((v0.a + v1.a) + v2.a) / 3.0f;  q.a = floorf(((g.a - o.a) / vs) / 8.0f);
 *                 b.a = q.a >= (float)(nb - 1) ? nb - 1 : (q.a > 0 ? (int)q.a : 0)  -- clamped to the grid (a NaN gives 0), so a mesh scaled
 *                 out of the frame is served; a node's box comes from its triangles, not from its cell, so the clamp costs no accuracy.
 *   levels        level k has ceil(nb / 2^k) nodes per side, up to the level with one node (n = 96: 12, 6, 3, 2, 1); node (x, y, z) of level
 *                 k + 1 has the children (2x + i, 2y + j, 2z + l), i, j, l in {0, 1}, that lie inside level k.
 *   node          count = its triangles; box = per axis the minimum and maximum of their vertex coordinates in the INTEGER order of floats
 *                 (-0 < +0);  h.a = (hi.a - lo.a) / 2.0f;  c.a = lo.a + h.a;  r = sqrtf(Dot(h, h));
 *                 area vector: per triangle and axis  s = ((double)nrm.a * 2^23) / ((double)vs * (double)vs)  -- nrm / 2 in units of
 *                 vs^2 2^-24 --, then s > 2^62: s = 2^62;  s < -2^62: s = -2^62;  s != s: s = 0;  A.a = llrint(s); the node's A = the sum of its
 *                 triangles' modulo 2^64 (two's complement);  N.a = (float)((double)A.a * (((double)vs * (double)vs) * 2^-24)).
 *                 A node without triangles contributes nothing.  Accuracy statements assume no wrap: the summed |area| of a node below
 *                 2^38 voxel faces.
 *   evaluation    per (brick of voxels B, node): lo.a / hi.a = the centres of the brick's first / last voxel along a;
 *                 g.a = max2(0, max2(lo.a - c.a, c.a - hi.a));  br = beta * r;  FAR iff Dot(g, g) > br * br && beta > 0.
 *                 From the root: a FAR node is one far term for each of the 512 voxels of B; otherwise a leaf contributes its triangles
 *                 exactly and an inner node is descended into.
 *   beta          0: no far field, the brute-force sum over all valid triangles (the accuracy anchor); 1 .. 64: the opening parameter.
 *                 Anything else, or not finite: VP_ERR_INVALID.  level must be finite.  Only the dipole (Barill's order 1) is implemented.
 *   vp_winding         builds w (4 n^3 bytes, x fastest) and the inside grid (n^3 / 8 bytes, the library's bit layout) into grow-only
 *                      buffers that the CONTEXT owns; vp_ctx_release frees them.  Enqueues only, once the buffers have grown (nothing is
 *                      read back); with h_inside_count != NULL it BLOCKS and stores the number of inside voxels.
 *   vp_winding_result  pointers to the last result and the side it is for; any argument may be NULL.  Before a build and after a release:
 *                      NULL pointers and side 0.  The inside grid is a grid like any other: vp_mesh_distance takes it as d_sign_words
 *                      (the centre-exact sign), and vp_csg, vp_morph, vp_extract, vp_surfnets, vp_jfa, ... read it as their input.
 *   vp_winding_host    host in, host out (mesh staged through workspace slots); h_w or h_inside may be NULL, not both.
 * Whole-grid frames only: a slab frame and n > 1024 return VP_ERR_UNSUPPORTED.  Null ctx / f, null mesh arrays with ntris > 0, mesh arrays
 * that are not 16-byte aligned, an unknown algo: VP_ERR_INVALID.  A refusal is decided before anything is touched and leaves the previous
 * result as it was.
 *   algo: VP_ALGO_TILED -- one workgroup per brick walks the pyramid once for its 512 voxels (the far test depends on the brick and the
 *   node only), near leaves' records staged through LDS, two 64-bit accumulators per lane, inside bits by ballot; VP_ALGO_NAIVE -- one
 *   thread per voxel walks the pyramid from global memory.  Same bytes.  Scratch of the context (grow-only, freed by vp_ctx_release): the
 *   records sorted by leaf (48 B per triangle) and the pyramid (84 B per node + 4 B per leaf and per triangle).  Timing books under the keys
 *   of the corresponding vp_mesh_distance stages: VP_K_MD_SETUP, _SCAN, _WRITE, _COUNT (the level reductions), _BRICK, _NAIVE, _SPLIT (the
 *   inside count, when asked for). */
#define VP_WN_ATAN_C0 0x1.000000p+0f
#define VP_WN_ATAN_C1 -0x1.5554eep-2f
#define VP_WN_ATAN_C2 0x1.9986eap-3f
#define VP_WN_ATAN_C3 -0x1.23c878p-3f
#define VP_WN_ATAN_C4 0x1.bd901cp-4f
#define VP_WN_ATAN_C5 -0x1.506f4ap-4f
#define VP_WN_ATAN_C6 0x1.c2c986p-5f
#define VP_WN_ATAN_C7 -0x1.d2c990p-6f
#define VP_WN_ATAN_C8 0x1.397f42p-7f
#define VP_WN_ATAN_C9 -0x1.8ba540p-10f
#define VP_WN_HALF_PI 0x1.921fb6p+0f
#define VP_WN_PI 0x1.921fb6p+1f
#define VP_WN_FOUR_PI 0x1.921fb54442d18p+3 /* double */
int vp_winding(vp_ctx* ctx, const vp_frame* f, const float* d_xyz, size_t nverts, const uint32_t* d_tri, size_t ntris, float beta,
               float level, int algo, uint64_t* h_inside_count /* may be NULL */);
int vp_winding_result(vp_ctx* ctx, float** d_w, uint32_t** d_inside, uint32_t* h_n);
int vp_winding_host(vp_ctx* ctx, const vp_frame* f, const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris, float beta,
                    float level, int algo, float* h_w, uint32_t* h_inside, uint64_t* h_inside_count /* may be NULL */);

/* ---- local thickness: the largest inscribed ball through every voxel (no reference counterpart) ------------------
 * For every set voxel the squared radius of the largest ball that fits inside the solid and contains the voxel (Hildebrand & Ruegsegger
 * 1997, the "Local Thickness" of Fiji / BoneJ), exact in integers, in a band of rmax = 1 .. 32 voxels.  S = the set voxels of a whole-grid
 * frame, n <= 1024, n % 32 == 0; voxel coordinates are integers, |p - c|^2 = dx^2 + dy^2 + dz^2.
 *   capped inscribed radius   D(c) = min(E(c), W(c), rmax^2) for c in S, where
 *                 E = vp_edt with VP_EDT_SEEDS_UNSET: the exact squared distance to the nearest unset voxel, VP_EDT_NONE on a grid
 *                 without an unset voxel (the min takes care of that);
 *                 W(c) = (1 + min(x, n-1-x, y, n-1-y, z, n-1-z))^2: the squared distance to the nearest voxel OUTSIDE the grid.
 *                 OUTSIDE THE GRID COUNTS AS EMPTY HERE: the object ends at the frame's wall.  (vp_edt_morph's erode treats the
 *                 outside as no seed, i.e. as solid; this operator does not.)  So every set voxel has 1 <= D <= rmax^2, and the open
 *                 ball of squared radius D(c) around c holds set voxels only and stays inside the grid.
 *   thickness     T2(p) = max { D(c) : c in S, |p - c|^2 < D(c) } for p in S, and 0 for p not in S.  The comparison is strict.  uint32, x
 *                 fastest, 4 n^3 bytes, like d_dist2.  The local thickness in voxels is 2 sqrt(T2); callers multiply by the voxel size.
 *                 A region thicker than 2 rmax reads rmax^2: saturated.  The operator is a band, like vp_mesh_distance.
 *   thin grid     bit p = p in S && T2(p) < thin2, thin2 in 0 .. rmax^2 (0: the empty grid).  A grid like any other: vp_components_*,
 *                 vp_morph, vp_extract, vp_surfnets, ... read it unchanged.  A thickness of W whole voxels is thin iff 4 T2 < W^2, i.e.
 *                 thin2 = ceil(W^2 / 4).
 * Integer arithmetic and a maximum over a set: numpy, the C++ host form, VP_ALGO_NAIVE and VP_ALGO_TILED give the same bytes whatever any
 * of them culls.  Facts (tests/test_thickness_cpu.py holds them on hand cases and random grids):
 *   slab read-out     a slab w voxels wide, far from the walls, reads T2 = ceil(w / 2)^2 (w = 1 .. 7: 1, 1, 4, 4, 9, 9, 16): the discrete
 *                     read-out of a w-voxel wall is 2 ceil(w / 2).
 *   bounds            T2 >= D pointwise; max T2 = max D; T2 = 0 exactly on the unset voxels.
 *   saturation        {T2 = rmax^2} = {p : the VP_EDT_SEEDS_SET transform of the seed set {c in S : min(E, W) >= rmax^2} is < rmax^2 at
 *                     p}: the saturated region is one more separable transform and needs no ball.
 *   cap consistency   T2 at rmax <= min(T2 at r', rmax^2) for r' > rmax, with equality wherever T2 at r' < rmax^2; elsewhere the
 *                     inequality can be strict (a ball larger than rmax, cut down to rmax, covers less).
 *   opening           for every t that occurs as a value of D, every voxel of {VP_EDT_SEEDS_SET of {D >= t} < t} -- the opening by the
 *                     open ball of squared radius t -- has T2 >= t.
 * Gap or channel width is the same call on the complemented words; the frame's wall then acts as solid.
 *   vp_thickness         builds T2 and the thin grid into grow-only buffers that the CONTEXT owns; vp_ctx_release frees them.  Enqueues
 *                        only, once the buffers have grown; with h_thin_count != NULL it BLOCKS and stores the number of thin voxels.
 *   vp_thickness_result  pointers to the last result and the side it is for; any argument may be NULL.  Before a build and after a
 *                        release: NULL pointers and side 0.
 *   vp_thickness_host    host in, host out (the grid staged through a workspace slot); h_t2 or h_thin may be NULL, not both.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / words, words that are not 16-byte aligned, d_words overlapping a buffer the
 * context writes in this call (its result buffers among them: copy the last thin grid before measuring it), rmax outside 1 .. 32,
 * thin2 > rmax^2, an unknown algo: VP_ERR_INVALID.  A refusal is decided before anything is touched and leaves the previous result as it
 * was.  The result buffers are outputs like any other: a pending vp_jfa_start / vp_extract_count / vp_surfnets_count of a grid they
 * overlap is dropped.
 *   algo: VP_ALGO_NAIVE -- the UNSET transform, then one thread per set voxel c paints its ball with atomicMax(T2[p], D(c)), then a
 *   streaming pass for the thin bits; its cost is the sum of the ball volumes: the check, not the product.  VP_ALGO_TILED -- the transform,
 *   D as uint16 with a summary per 8 x 8 x 8 brick, the saturated region by the identity above, then one workgroup per brick that has a set,
 *   unsaturated voxel gathers from the neighbour bricks within rmax - 1 voxels (bricks and candidates whose balls cannot reach the brick
 *   are skipped; survivors go through an LDS batch), no atomics on the field; a streaming fill writes the other bricks.  Scratch of the
 *   context (grow-only, freed by vp_ctx_release): the distance volume(s) of vp_edt_morph, 2 n^3 + n^3 / 4 bytes and 8 bytes per brick.
 *   Timing books under existing keys: the transforms under VP_K_EDT_X / _Y / _Z (NAIVE: _Y_NAIVE / _Z_NAIVE), the cap, threshold and
 *   thin-grid passes under VP_K_EDT_THRESH, the brick kernel under VP_K_MD_BRICK, the scatter under VP_K_MD_NAIVE, the fill under
 *   VP_K_MD_FILL, the count under VP_K_MD_SPLIT. */
int vp_thickness(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t rmax, uint32_t thin2, int algo,
                 uint64_t* h_thin_count /* may be NULL; BLOCKS when given */);
int vp_thickness_result(vp_ctx* ctx, uint32_t** d_t2, uint32_t** d_thin, uint32_t* h_n);
int vp_thickness_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t rmax, uint32_t thin2, int algo,
                      uint32_t* h_t2, uint32_t* h_thin /* either may be NULL, not both */, uint64_t* h_thin_count /* may be NULL */);

/* ---- sparse voxel octree: build from any grid, expand back (no reference counterpart) ---------------------------
 * The compact, hierarchical form of a bit grid.  Whole-grid frames, n % 32 == 0, n <= 1024; any grid of this library goes in.
 *   geometry      The tree covers the cube of side P = NextPow2(n), L = log2 P levels, 5 <= L <= 10.  Voxels outside the grid are empty
 *                 (n = 96: P = 128; n = 160: P = 256).  A level-l cell, l = 0 .. L, has side P >> l.  A cell is EMPTY if it has no set
 *                 voxel, FULL if all of its voxels are set (possible only for a cell inside the grid), else MIXED.
 *   stored nodes  one for the root, always, and one for every mixed cell of the levels 1 .. L - 1.  Full and empty cells are never stored:
 *                 full subtrees are pruned.
 *   order         breadth-first, level by level; within a level in ascending Morton code of the cell coordinates (bit i of x -> bit 3 i,
 *                 of y -> 3 i + 1, of z -> 3 i + 2).  Child index c = x + 2 y + 4 z, so the children of a node are consecutive and in c
 *                 order.  The order is unique: two trees of the same grid are the same bytes.
 *   record        two uint32, 8 bytes.  masks: bits 0 .. 7 `valid` (child c is not empty), bits 8 .. 15 `full` (child c is full), full a
 *                 subset of valid, the upper 16 bits 0.  child: the absolute index of the first stored (mixed) child, 0 when there is none
 *                 (index 0 is the root and never a child).  The stored children are the set bits of valid & ~full, found at child + rank.
 *                 At level L - 1 the children are voxels: valid == full == the 2 x 2 x 2 bits and child == 0.
 *   summary       uint32 level_offset[11]: entries 0 .. L are the running sums of the per-level node counts, the rest repeat M, the total.
 *                 uint32 full_leaves[11]: the full children counted per level of their parent, so that the sum over l of
 *                 full_leaves[l] * (P >> (l + 1))^3 is the number of set voxels.  M < 2^28.
 * Facts (tests/test_octree_cpu.py): the empty grid is one node with masks 0; the full 32^3 or 64^3 grid one node with masks 0xFFFF; the
 * full 96^3 grid has the levels [1, 7, 0, 0, 0, 0, 0]; expand(build(g)) == g; build is injective; a grid placed in a larger frame with the
 * same P has the same tree.  Worst case (noise): M <= (8^L - 1) / 7 nodes, about 1.14 P^3 bytes -- the node buffer is sized from the count.
 *   vp_octree               builds the tree into grow-only buffers that the CONTEXT owns; vp_ctx_release frees them.  BLOCKS once: the
 *                           summary is read back and the node buffer sized exactly.  h_nodes (may be NULL) receives M.
 *   vp_octree_result        the last result: the device nodes, M, the two summaries (11 entries each) and the side it is for; any argument
 *                           may be NULL.  Before a build and after a release: NULL, 0, zeros and side 0.
 *   vp_octree_expand        a tree back into a bit grid of side f->n (P from f->n: a tree built at n = 96 expands into n = 128 as the
 *                           zero-padded grid), into a grow-only grid that the CONTEXT owns, like the nodes (every output of this
 *                           section is the context's; vp_ctx_release frees it).  Overwrites every word; enqueues only, once the grid
 *                           has grown.
 *   vp_octree_expand_result the grid of the last vp_octree_expand and its side; either argument may be NULL.  Before an expand and after
 *                           a release: NULL and side 0.  A grid like any other: copy it before the next expand overwrites it.  The kernels read a child only if its index is below
 *                           `nodes` (anything else counts as empty) and descend L levels at most: whatever the bytes are, they neither
 *                           read outside the buffer nor loop.  What they produce from bytes that are not a tree is unspecified.
 *   vp_octree_host          host in, host out (the grid staged through a workspace slot).  *h_count receives M; a capacity below M returns
 *                           VP_ERR_INVALID without writing h_nodes (call again with room for *h_count records).
 *   vp_octree_expand_host   validates (below) before anything goes to the device, then expands.
 *   vp_octree_validate_host pure CPU, no context: 0 for a well-formed tree of a grid of side n, else VP_ERR_INVALID (vp_last_error says
 *                           which node): upper mask bits, full not within valid, a stored cell of a level >= 1 that is empty or full, a
 *                           mixed "voxel", a child that is not exactly the running sum of the stored children so far (out of range included),
 *                           levels that do not end exactly at M, a full child that pokes out of the grid, a valid child outside it.
 *                           Everything that comes from a file goes through it before it may reach a device.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / pointers, buffers that are not 16-byte aligned, an unknown algo, d_words
 * overlapping a buffer the context writes in vp_octree (its own nodes among them: copy them first), d_nodes overlapping the context's
 * grid in vp_octree_expand, nodes outside 1 .. 2^28 - 1: VP_ERR_INVALID.  A refusal is decided before anything is touched and leaves the previous
 * result as it was.
 *   algo: VP_ALGO_NAIVE -- a state byte per cell of every level in Morton order, filled bottom-up by one thread per cell, per level a
 *   one-workgroup scan of the stored flags, then one thread per cell writes the record of a stored one; memory about 5.7 bytes per side-2
 *   cell (0.7 P^3).  VP_ALGO_TILED -- one workgroup per 32^3 block of bits staged in LDS reduces the five levels inside the block (sides 2
 *   .. 32) from any / all bits; a count launch, one workgroup for the levels above the blocks and every scan, a write launch that repeats
 *   the reduction and stores each record at level_offset + block offset + rank; no atomics.  Expand: NAIVE one thread per voxel, TILED
 *   one lane per word (the walk to the side-32 cell, then at most 31 node visits along x).
 *   Timing books under existing keys (vp_prof_select's mask is full): TILED count under VP_K_MD_COUNT, the upper levels and every scan
 *   under VP_K_MD_SCAN, the writes under VP_K_MD_WRITE; NAIVE state volumes under VP_K_MD_PREFILL, its scans under VP_K_MD_SCAN, its
 *   writes under VP_K_MD_NAIVE; expand (both) under VP_K_MD_FILL. */
int vp_octree(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint64_t* h_nodes /* may be NULL */);
int vp_octree_result(vp_ctx* ctx, uint32_t** d_nodes, uint64_t* h_nodes, uint32_t* h_level_offset /* 11 */, uint32_t* h_full_leaves /* 11 */,
                     uint32_t* h_n);
int vp_octree_expand(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_nodes, uint64_t nodes, int algo);
int vp_octree_expand_result(vp_ctx* ctx, uint32_t** d_words, uint32_t* h_n);
int vp_octree_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, int algo, uint32_t* h_nodes, uint64_t capacity,
                   uint64_t* h_count, uint32_t* h_level_offset /* 11, may be NULL */, uint32_t* h_full_leaves /* 11, may be NULL */);
int vp_octree_expand_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_nodes, uint64_t nodes, int algo, uint32_t* h_words);
int vp_octree_validate_host(const uint32_t* h_nodes, uint64_t nodes, uint32_t n);

/* ---- topological thinning: curve skeletons and homotopy kernels (no reference counterpart) ------------------------
 * Reduces a solid to a one-voxel-wide remainder with the same topology (the "Skeletonize3D" next to the "Local Thickness" of Fiji / BoneJ,
 * ITK's binary thinning), as an 8-subfield parallel thinning for (26, 6) connectivity.  S = the set voxels of a whole-grid frame,
 * n % 32 == 0, n <= 1024.  OUTSIDE THE GRID COUNTS AS EMPTY, as in vp_thickness.
 *   neighbourhood   a 27-bit mask m(p), bit i = (dx+1) + 3 (dy+1) + 9 (dz+1) set iff p + (dx, dy, dz) is in S; bit 13 is the centre and is
 *                   ignored.  N26 = all other bits, N18 = those with |dx| + |dy| + |dz| <= 2, N6 = the six faces.
 *   simple point    simple(m) holds iff (a) the object bits m & N26 are non-empty and form exactly one 26-connected component, and (b) the
 *                   background bits ~m & N18 contain at least one face bit and all face bits among them lie in one 6-connected component
 *                   of ~m & N18 (Bertrand & Malandain 1994 for (26, 6)).  It depends on 26 bits only; exactly 25,985,144 of the 2^26
 *                   neighbourhoods are simple.
 *   one iteration   B = { p in S, p not in the anchor, some face neighbour of p unset or outside the grid }, taken ONCE, at the start of
 *                   the iteration.  Eight sub-iterations follow, s = 0 .. 7 in ascending order, s = (x & 1) | (y & 1) << 1 | (z & 1) << 2
 *                   in absolute voxel coordinates.  In sub-iteration s every p in B of subfield s that is still set is examined against
 *                   the CURRENT S and deleted iff simple(m(p)) and, in mode VP_SKEL_CURVE, popcount(m & N26) != 1 (line ends stay).
 *                   Two voxels of one subfield are never 26-neighbours, so simultaneous deletion equals sequential deletion in any
 *                   order: topology is preserved by construction and the result does not depend on the order of execution.
 *   termination     iterations repeat until one deletes nothing or max_iters have run (max_iters = 0: no limit); `iterations` counts the
 *                   iterations run, the empty last one included.  Every other iteration deletes at least one voxel.
 *   modes           VP_SKEL_KERNEL: no end-point rule -- a ball shrinks to one voxel, a torus to a closed loop, a shell with a cavity to a
 *                   closed one-voxel surface.  VP_SKEL_CURVE: the centre line.
 *   anchor          optional grid whose voxels are never deleted (with VP_SKEL_KERNEL: anchored homotopic thinning, e.g. around the
 *                   maxima of vp_edt).
 * Integer logic with a fixed sub-iteration order: numpy, the C++ host form, VP_ALGO_NAIVE and VP_ALGO_TILED give the same bytes and the
 * same three statistics h_stats = { voxels left, iterations, voxels deleted }.
 *   vp_skeleton         builds the skeleton into a grow-only grid that the CONTEXT owns; vp_ctx_release frees it.  BLOCKS: the deleted
 *                       count of every iteration is read back.
 *   vp_skeleton_result  pointer to the last result, its statistics and the side it is for; any argument may be NULL.  Before a build and
 *                       after a release: NULL, zeros and side 0.
 *   vp_skeleton_host    host in, host out (grid and anchor staged through workspace slots); h_skel or h_stats may be NULL, not both.
 *   vp_skeleton_table_host   bit c of the 2^21 words = simple(m) for m = (c & 0x1FFF) | (c >> 13) << 14, the 26 non-centre bits packed.
 *                       ctx = NULL: computed on the CPU; otherwise by one launch.  VP_ALGO_NAIVE: the plain form of simple(), a flood fill
 *                       over adjacency masks; VP_ALGO_TILED: the shift form -- in the x + 3 y + 9 z packing a 26-dilation is three masked
 *                       shift pairs, a 6-dilation the OR of six masked shifts, run for a fixed 9 steps for (a) and 11 for (b): an
 *                       exhaustive run needs at most 8 and 10 dilations to reach the component, one more shows the fixed point.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / words, a buffer that is not 16-byte aligned, d_words or d_anchor
 * overlapping a buffer the context writes in this call (its result grid among them: copy the last skeleton before thinning it further),
 * an unknown mode or algo: VP_ERR_INVALID.  A refusal is decided before anything is touched and leaves the previous result as it was.
 * The result grid is an output like any other: a pending vp_jfa_start / vp_extract_count / vp_surfnets_count of a grid it overlaps is
 * dropped.
 *   algo: both run one border-mark launch and eight sub-iteration launches per iteration.  VP_ALGO_NAIVE -- one lane per word of 32
 *   voxels from global memory with the plain form, ping-pong between two grids.  VP_ALGO_TILED -- one workgroup per block of 32 x 16 x 16
 *   voxels staged in LDS with a one-voxel halo, candidates compacted over the workgroup before the shift form runs, updated in place (in
 *   sub-iteration s only subfield-s bits change and nobody reads a subfield-s bit but its owner), driven by the list of the blocks that,
 *   or a 26-neighbour of which, lost a voxel in the previous iteration (count, scan, write; no atomics on the grid).  Scratch of the
 *   context (grow-only, freed by vp_ctx_release): n^3 / 8 bytes of border words, NAIVE's second grid, 8 bytes per block.
 *   Timing books under existing keys: the copy of the input and the border marks under VP_K_SURFACE, the sub-iterations under
 *   VP_K_MORPH (TILED) / VP_K_MORPH_NAIVE, the block list under VP_K_MD_SCAN, the final count under VP_K_MD_SPLIT, the device table
 *   under VP_K_MD_NAIVE (plain form) / VP_K_MD_BRICK (shift form). */
enum { VP_SKEL_KERNEL = 0, VP_SKEL_CURVE = 1 };
int vp_skeleton(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const uint32_t* d_anchor /* may be NULL */, int mode,
                uint32_t max_iters, int algo, uint64_t* h_stats /* 3, may be NULL: voxels left, iterations, voxels deleted */);
int vp_skeleton_result(vp_ctx* ctx, uint32_t** d_skel, uint64_t* h_stats /* 3 */, uint32_t* h_n);
int vp_skeleton_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, const uint32_t* h_anchor /* may be NULL */, int mode,
                     uint32_t max_iters, int algo, uint32_t* h_skel, uint64_t* h_stats /* either may be NULL, not both */);
int vp_skeleton_table_host(vp_ctx* ctx /* NULL: computed on the CPU */, int algo, uint32_t* h_table /* 2^21 words: bit c = simple(c) */);

/* ---- geodesic distance: path length inside the solid from seed voxels (no reference counterpart) ----------------
 * Every other distance of the library (JFA, vp_edt, vp_mesh_distance) is a straight line and goes through walls.  This is the geodesic
 * distance map that Fiji / MorphoLibJ put beside "Local Thickness" and "Skeletonize3D": the length of the shortest path that stays
 * inside a mask, from a set of seed voxels to every voxel of the mask.
 *   inputs      a whole-grid frame, n % 32 == 0, n <= 1024; a mask grid M and a seed grid S, both bit grids in the library's layout.
 *               OUTSIDE THE GRID COUNTS AS NOT IN M.  The seeds used are S & M: seed bits outside M are ignored.
 *   step        from a voxel of M to one of its 26 neighbours that is also in M.  No other voxel has to be set for a diagonal step: two
 *               cubes of M that touch at one corner are connected for the metrics with corner steps (MorphoLibJ's rule).  A step that
 *               changes 1, 2 or 3 coordinates costs w1, w2 or w3:
 *                 VP_GEO_6        (1, -, -)   face steps only
 *                 VP_GEO_26       (1, 1, 1)   all 26 steps
 *                 VP_GEO_CHAMFER  (3, 4, 5)   all 26 steps (Borgefors; divide by 3 for voxels)
 *   output D    one uint32 per voxel, x fastest like vp_edt: the minimum cost over all such paths from any used seed.  Seeds read 0;
 *               voxels of M that no path reaches, and voxels outside M, read VP_GEO_NONE.  Sums saturate at VP_GEO_MAX: the add is
 *               min(d + w, VP_GEO_MAX) in every form (monotone, so the fixed point stays unique; not reachable in practice at n <= 1024).
 *   reach R     a bit grid, one bit set per voxel with D != VP_GEO_NONE: the components of M that touch a used seed (morphological
 *               reconstruction; face-connected for VP_GEO_6, 26-connected for the others).
 *   h_stats     { seeds used |S & M|, voxels reached, the largest finite D, the lowest linear index x + n (y + n z) of a voxel that
 *               attains it }.  With no seed used D is VP_GEO_NONE everywhere, R is empty and the statistics are zeros.  Nothing that
 *               depends on the number of rounds is reported.
 * The distances are integers and the minimum over paths is unique: numpy, the C++ host form, VP_ALGO_NAIVE and VP_ALGO_TILED give the same
 * bytes and statistics whatever the order of execution (the argument is in csrc/geodesic.hip and DESIGN.md section 21).
 *   vp_geodesic         builds D and R into grow-only buffers that the CONTEXT owns (4 n^3 and n^3 / 8 bytes); vp_ctx_release frees them.
 *                       BLOCKS: convergence is read back -- a batch of round flags at a time (NAIVE), the length of the list of active
 *                       blocks once per round (TILED).
 *   vp_geodesic_result  pointers to the last D and R, the statistics and the side they are for; any argument may be NULL.  Before a build
 *                       and after a release: NULL, zeros and side 0.
 *   vp_geodesic_host    host in, host out (mask and seeds staged through workspace slots); any two of h_dist / h_reach / h_stats may be
 *                       NULL, not all three.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / mask / seeds, a buffer that is not 16-byte aligned, d_mask or d_seeds
 * overlapping a buffer the context writes in this call (the last D and R among them: copy them first), an unknown metric or algo:
 * VP_ERR_INVALID.  A refusal is decided before anything is touched and leaves the previous result as it was.
 *   algo: VP_ALGO_NAIVE -- one lane per voxel of M pulls min(D[q] + w) over its allowed neighbours from global memory, in place;
 *   whole-grid launches repeat until one changes nothing.  VP_ALGO_TILED -- one workgroup per active block of 32 x 16 x 16 voxels, D and a
 *   one-voxel halo staged in LDS (45 KB), relaxed inside the block until a sweep changes nothing or a fixed number of sweeps have run,
 *   changed values written back; a block whose face, edge or corner voxel changed raises the flags of the neighbour blocks that see the
 *   voxel, the next list comes from the flags by count, scan, write; the first list is the blocks that hold a used seed or see one in their halo (a seed reads 0
 *   from the start and is never "changed", so the launch that writes the initial D raises them by the same rule), the loop ends with the
 *   first empty list; a block that is never listed sees VP_GEO_NONE only.  No atomics on D; kernel boundaries are the only synchronisation between workgroups.  Scratch of the context
 *   (grow-only, freed by vp_ctx_release): 8 bytes per block.
 *   Timing books under existing keys: the launch that writes the initial D under VP_K_MD_FILL, the final reach / statistics launch under
 *   VP_K_MD_SPLIT, the block list under VP_K_MD_SCAN, the TILED relaxation rounds under VP_K_MD_BRICK, the NAIVE rounds under
 *   VP_K_MD_NAIVE. */
enum { VP_GEO_6 = 0, VP_GEO_26 = 1, VP_GEO_CHAMFER = 2 };
#define VP_GEO_NONE 0xFFFFFFFFu
#define VP_GEO_MAX 0xFFFFFFFEu
int vp_geodesic(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_mask, const uint32_t* d_seeds, int metric, int algo,
                uint64_t* h_stats /* 4, may be NULL: seeds used, voxels reached, largest finite D, lowest index that attains it */);
int vp_geodesic_result(vp_ctx* ctx, uint32_t** d_dist, uint32_t** d_reach, uint64_t* h_stats /* 4 */, uint32_t* h_n);
int vp_geodesic_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_mask, const uint32_t* h_seeds, int metric, int algo,
                     uint32_t* h_dist, uint32_t* h_reach, uint64_t* h_stats /* any two may be NULL, not all three */);

/* ---- seeded watershed and geodesic influence zones: split touching parts (no reference counterpart) ----------------
 * Every operator above that produces regions stops at connectivity: two grains that touch are one component.  This is the marker-controlled
 * watershed that MorphoLibJ calls "Distance Transform Watershed 3D": a priority field is flooded level by level from one marker per object
 * and cut where the floods meet.  Without a priority field it gives the geodesic influence zones of the markers.
 *   inputs      a whole-grid frame, n % 32 == 0, n <= 1024; a mask M, a bit grid (OUTSIDE THE GRID COUNTS AS NOT IN M); a marker volume L0,
 *               one uint32 per voxel, x fastest like vp_components_label's output: 0 = no marker, labels 1 .. VP_WS_LABEL_MAX = 2^20 - 1;
 *               markers outside M are ignored (their labels are not looked at); a label may cover several voxels and several blobs; an
 *               optional priority field P, one uint32 per voxel in vp_edt's layout (its output can be passed as it is).
 *   order       VP_WS_ASCENDING floods from low P, VP_WS_DESCENDING from high P (what a distance map needs: the caller inverts nothing).
 *   levels      level(v) = P(v) / quantum (integer division, quantum >= 1) for v in M; the levels present in M are run in flood order.
 *               P == NULL: ONE level that holds all of M -- the influence-zones mode; quantum and order are then ignored.  max - min of
 *               the levels over M must be < VP_WS_MAX_SPAN = 16384: otherwise VP_ERR_INVALID, and the message names the smallest
 *               quantum that fits.
 *   flooding    W = L0 on M, 0 elsewhere.  For each present level h in flood order: A = { v in M : W(v) = 0, level(v) not later than h };
 *               the sources are the voxels with W != 0 at the start of the level.  A path is a source u0 followed by v1 .. vk in A,
 *               consecutive voxels being neighbours under `connectivity` (VP_CONN_6 / VP_CONN_26; a diagonal step needs no other voxel
 *               set).  Its key is (k, level(u0), W(u0)), compared lexicographically, "level" in flood order: fewer hops win, then the
 *               source that lies earlier in flood order, then the smaller label.  Every v in A that some path reaches takes the label of
 *               its minimum key; all assignments of a level take effect together, and a voxel labelled in level h is a source, with its
 *               own level(v), from the next level on.  After the last level the voxels of M with W = 0 are exactly those that no path in
 *               M joins to a marker.
 *               The source-level term keeps the lower label from creeping sideways along an interface one voxel per level (two equal
 *               balls, exact D^2, quantum 1: no voxel off the symmetry plane with it, thousands without it).  At a coarse quantum the
 *               sources share levels and the term does nothing: that is the contract, not a defect.
 *   output W    the label volume, one uint32 per voxel (4 n^3 bytes).
 *   output C    the CUT GRID, a bit grid: bit v is set iff W(v) != 0 and no neighbour u (same connectivity) has W(u) > W(v).  A
 *               one-sided, one-voxel cut: no two voxels of C with different labels are neighbours, so C feeds vp_components_*,
 *               vp_thickness, vp_octree and the meshers as "the parts, separated".
 *   h_stats     { marker voxels used |L0 != 0 & M|, voxels labelled, distinct levels present in M (1 in zones mode, 0 for an empty M),
 *               voxels cut = labelled - |C| }.  Nothing that depends on the number of rounds is reported.  With no marker in M: W = 0,
 *               C empty, { 0, 0, levels, 0 }.
 * Integer keys and a minimum over paths that is unique level by level: numpy, the C++ host form, VP_ALGO_NAIVE and VP_ALGO_TILED give the
 * same bytes and statistics whatever the order of execution (the argument is in csrc/watershed.hip and DESIGN.md section 22).
 *   vp_watershed         builds W and C into grow-only buffers that the CONTEXT owns; vp_ctx_release frees them.  BLOCKS: a pre-pass over
 *                        M, L0 and P is read back once (min / max level, largest label, the levels present), then per present level the
 *                        round flags (NAIVE) or the list length (TILED).
 *   vp_watershed_result  pointers to the last W and C, the statistics and the side they are for; any argument may be NULL.  Before a
 *                        build and after a release: NULL, zeros and side 0.
 *   vp_watershed_host    host in, host out (staged through workspace slots); h_priority may be NULL; any two of h_labels / h_cut /
 *                        h_stats may be NULL, not all three.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / mask / markers, a buffer that is not 16-byte aligned, an input
 * overlapping a buffer the context writes in this call (the last W and C among them: copy them first), an unknown order (with P),
 * connectivity or algo, quantum 0 (with P), a marker label in M above VP_WS_LABEL_MAX, a level span of VP_WS_MAX_SPAN or more:
 * VP_ERR_INVALID.  The last two are found by the pre-pass, which writes scratch only: every refusal leaves the previous result as it was.
 *   algo: both keep one 64-bit key per voxel (8 n^3 bytes of scratch), [arrival time : 30 | level rank of the source : 14 | label : 20],
 *   read and written across workgroups with single 8-byte accesses.  VP_ALGO_NAIVE -- one lane per voxel from global memory, in place;
 *   per level whole-grid launches repeat until one changes nothing.  VP_ALGO_TILED -- one workgroup per active block of 32 x 16 x 16
 *   voxels, the keys and a one-voxel halo staged in LDS (about 90 KB: one workgroup per CU), swept until nothing changes or a fixed
 *   number of sweeps ran; neighbour blocks are flagged as in vp_geodesic; the first list of a level is the blocks whose recorded range
 *   of P meets the level.  Kernel boundaries are the only synchronisation between workgroups, and they separate the levels.
 *   Timing books under existing keys: the pre-pass under VP_K_MD_FILL, the final W / C / counts launch under VP_K_MD_SPLIT, the block
 *   lists under VP_K_MD_SCAN, the TILED rounds under VP_K_MD_BRICK, the NAIVE rounds under VP_K_MD_NAIVE. */
enum { VP_WS_ASCENDING = 0, VP_WS_DESCENDING = 1 };
#define VP_WS_LABEL_MAX 0xFFFFFu
#define VP_WS_MAX_SPAN 16384u
int vp_watershed(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_mask, const uint32_t* d_markers, const uint32_t* d_priority /* may be NULL */,
                 int order, uint32_t quantum, int connectivity, int algo,
                 uint64_t* h_stats /* 4, may be NULL: markers used, voxels labelled, levels present, voxels cut */);
int vp_watershed_result(vp_ctx* ctx, uint32_t** d_labels, uint32_t** d_cut, uint64_t* h_stats /* 4 */, uint32_t* h_n);
int vp_watershed_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_mask, const uint32_t* h_markers, const uint32_t* h_priority /* may be NULL */,
                      int order, uint32_t quantum, int connectivity, int algo, uint32_t* h_labels, uint32_t* h_cut,
                      uint64_t* h_stats /* any two may be NULL, not all three */);

/* ---- grayscale reconstruction and h-extrema: automatic watershed markers (no reference counterpart) ------------------
 * vp_watershed floods from one marker per object, and the only marker source above is vp_components_label of one erosion radius for the
 * whole grid.  This is what MorphoLibJ's "Distance Transform Watershed 3D" picks its markers with (its "dynamic" parameter): the extended
 * maxima of the distance map, through grayscale morphological reconstruction -- which also fills holes, removes peaks and gives h-domes.
 *   inputs      a whole-grid frame, n % 32 == 0, n <= 1024; a marker field F and a mask field G, one uint32 per voxel, x fastest, in
 *               vp_edt's layout; a domain M, a bit grid, NULL = every voxel.  OUTSIDE THE GRID COUNTS AS NOT IN M.
 *   work values u(v) = v for VP_REC_DILATION, u(v) = ~v for VP_REC_EROSION; off M the work value of both fields is 0.
 *   dilation    R is the unique field with R(p) = min(G(p), max(R0(p), max over the neighbours q of p in M of R(q))), R0 = min(F, G):
 *               R(p) is the maximum over paths q .. p inside M of min(R0(q), min of G along the path).  Neighbours under `connectivity`
 *               (VP_CONN_6 / VP_CONN_26; a diagonal step needs no other voxel set).
 *   erosion     the same on the complemented values, the result complemented back: rec_erosion(F, G) = ~rec_dilation(~F, ~G).
 *   output R    one uint32 per voxel (4 n^3 bytes); off M it reads 0 for dilation and 0xFFFFFFFF for erosion.
 *   walls       A WORK VALUE OF 0 INSIDE M BEHAVES EXACTLY LIKE "NOT IN M": the voxel stays at 0 and nothing passes through it (G = 0 for
 *               dilation, G = 0xFFFFFFFF for erosion).
 *   h_stats     { |M|, voxels of M with R != R0, the sum of R over M (exact in 64 bits), the largest R over M (erosion: the smallest; 0
 *               for an empty M) }.  Nothing that depends on the number of rounds is reported.
 * Integers and a monotone fixed point that is unique: numpy, the C++ host form, VP_ALGO_NAIVE and VP_ALGO_TILED give the same bytes and
 * statistics whatever the order of execution (the argument is in csrc/reconstruct.hip and DESIGN.md section 25).
 *   vp_reconstruct         builds R into a grow-only buffer that the CONTEXT owns; vp_ctx_release frees it.  BLOCKS: convergence is read
 *                          back -- a batch of round flags at a time (NAIVE), the length of the list of active blocks once per round (TILED).
 *   vp_reconstruct_result  pointer to the last R, the statistics and the side they are for; any argument may be NULL.  Before a build and
 *                          after a release: NULL, zeros and side 0.
 *   vp_reconstruct_host    host in, host out (staged through workspace slots); h_domain may be NULL; h_field or h_stats may be NULL, not both.
 * vp_extrema composes it: h-maxima / h-minima and the extended extrema of a value field.
 *   V scaled    VP_EXT_LINEAR: the values as they are.  VP_EXT_SQRT16: floor(sqrt(256 v)) in exact 64-bit integer arithmetic, for every
 *               uint32 -- a squared distance such as vp_edt's becomes a distance in sixteenths of a voxel, a fixed h means the same depth
 *               at every size, and vp_watershed can flood V at quantum 1 where D^2 is refused.
 *   H flattened VP_EXT_MAXIMA: H = rec_dilation(V - h, V), the subtraction saturating at 0.  VP_EXT_MINIMA: H = rec_erosion(V + h, V), the
 *               addition saturating at 0xFFFFFFFF.  Both on the domain; off it H reads as R does.  h = 0 gives H = V on M.
 *   E extrema   a bit grid: for maxima p is in E iff H(p) > 0 and the plateau of p -- the connected set in M of equal H -- has no neighbour
 *               in M with a larger H; equivalently H(p) > rec_dilation(H - 1, H)(p), which is how it is built.  Minima are the dual.  A
 *               voxel whose work value is 0 is never an extremum (for D^2: the voxels outside the solid).  The markers of vp_watershed are
 *               vp_components_label(E, connectivity): the caller chains it.
 *   h_stats     { |M|, |E|, the largest H over M (minima: the smallest; 0 for an empty M), voxels of M with H != V }.
 *   vp_extrema / _result / _host   as above: V, H and E live in grow-only buffers of the context (4 n^3 + 4 n^3 + n^3 / 8 bytes) in a feature
 *               of their own, the second reconstruction in 4 n^3 bytes of scratch; all are freed by vp_ctx_release.  A vp_extrema call
 *               leaves vp_reconstruct_result as it was, and the other way round.  _host: any three of h_scaled / h_flat / h_extrema /
 *               h_stats may be NULL, not all four.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / marker / mask / values, a buffer that is not 16-byte aligned, an input
 * overlapping a buffer the context writes in this call (the last result among them: copy it first), an unknown mode / kind / scale /
 * connectivity / algo: VP_ERR_INVALID.  A refusal is decided before anything is touched and leaves the previous result as it was.
 *   algo: VP_ALGO_NAIVE -- one lane per voxel with room (R < G) pulls the maximum over its neighbours from global memory, in place;
 *   whole-grid launches repeat until one changes nothing.  VP_ALGO_TILED -- one workgroup per active block of 32 x 16 x 16 voxels, R and a
 *   one-voxel halo staged in LDS (45 KB), the lane's row of G in registers, swept until nothing rises or a fixed number of sweeps have
 *   run, changed values written back; neighbour blocks are flagged as in vp_geodesic; the first list is the blocks that hold a voxel with
 *   R0 < G (only such a voxel can ever change), the loop ends with the first empty list.  No atomics on R; kernel boundaries are the only
 *   synchronisation between workgroups.  Scratch of the context (grow-only, freed by vp_ctx_release): 8 bytes per block.
 *   Timing books under existing keys: the launches that write R0 and the scaled / shifted fields under VP_K_MD_FILL, the final launches
 *   (statistics, un-complementing, the extrema ballot) under VP_K_MD_SPLIT, the block list under VP_K_MD_SCAN, the TILED rounds under
 *   VP_K_MD_BRICK, the NAIVE rounds under VP_K_MD_NAIVE. */
enum { VP_REC_DILATION = 0, VP_REC_EROSION = 1 };
enum { VP_EXT_MAXIMA = 0, VP_EXT_MINIMA = 1 };
enum { VP_EXT_LINEAR = 0, VP_EXT_SQRT16 = 1 };
int vp_reconstruct(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_domain /* bit grid, may be NULL: the whole grid */,
                   const uint32_t* d_marker, const uint32_t* d_mask, int mode, int connectivity, int algo,
                   uint64_t* h_stats /* 4, may be NULL: |M|, voxels with R != R0, sum of R, largest (erosion: smallest) R */);
int vp_reconstruct_result(vp_ctx* ctx, uint32_t** d_field, uint64_t* h_stats /* 4 */, uint32_t* h_n);
int vp_reconstruct_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_domain /* may be NULL */, const uint32_t* h_marker,
                        const uint32_t* h_mask, int mode, int connectivity, int algo, uint32_t* h_field,
                        uint64_t* h_stats /* either may be NULL, not both */);
int vp_extrema(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_domain /* may be NULL */, const uint32_t* d_values, int kind, int scale,
               uint32_t h, int connectivity, int algo,
               uint64_t* h_stats /* 4, may be NULL: |M|, |E|, largest (minima: smallest) H, voxels with H != V */);
int vp_extrema_result(vp_ctx* ctx, uint32_t** d_scaled, uint32_t** d_flat, uint32_t** d_extrema, uint64_t* h_stats /* 4 */, uint32_t* h_n);
int vp_extrema_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_domain /* may be NULL */, const uint32_t* h_values, int kind, int scale,
                    uint32_t h, int connectivity, int algo, uint32_t* h_scaled, uint32_t* h_flat, uint32_t* h_extrema,
                    uint64_t* h_stats /* any three may be NULL, not all */);

/* ---- region analysis: per-label volume, moments, surface, Euler number (no reference counterpart) -------------------
 * The last step of voxelize -> repair -> split -> measure: what MorphoLibJ calls "Analyze Regions 3D".  vp_components_sizes stops at one
 * voxel count per label; this gives, per label of a label volume, everything that is an integer sum, minimum or maximum over voxels.
 *   inputs      a whole-grid frame, n % 32 == 0, n <= 1024; a label volume W, one uint32 per voxel, x fastest: what vp_components_label
 *               and vp_watershed write; count = K <= VP_REGIONS_MAX = 2^20 - 1 (= VP_WS_LABEL_MAX); an optional value field, one uint32 per
 *               voxel in vp_edt's layout (D^2, T2, a geodesic distance: any uint32).
 *   label       the EFFECTIVE LABEL of a voxel is l(v) = W(v) if 1 <= W(v) <= K, else 0: labels above K are ignored, as
 *               vp_components_sizes ignores them; A VOXEL OUTSIDE THE GRID HAS l = 0.  Voxel coordinates are the integers x, y, z in
 *               0 .. n - 1; the frame's origin and voxel size enter only the derived quantities of the wrappers.
 *   output      a table of K records of VP_REGION_WORDS = 26 uint64; record k - 1 belongs to label k:
 *                 0        V: voxels with l = k
 *                 1 - 3    min x, y, z over them            4 - 6    max x, y, z
 *                 7 - 9    sum x, y, z                      10 - 15  sum x^2, y^2, z^2, xy, xz, yz
 *                 16 - 18  exposed faces with normal +-x, +-y, +-z: faces of a voxel of k whose neighbour across the face has l != k
 *                          (background, another label or outside the grid)
 *                 19       contact faces: those exposed faces (all axes) whose neighbour has l != 0
 *                 20       n0: lattice points with at least one of their 8 incident voxels in k
 *                 21       n1: lattice edges with at least one of their 4 incident voxels in k
 *                 22 - 24  sum, min, max of the value field over k (0, 0, 0 when d_values is NULL)
 *                 25       the lowest linear index x + n (y + n z) of a voxel of k
 *               A label with V = 0 has an ALL-ZERO record.  The Euler number of the closed-cube complex of k (26-connected foreground,
 *               the convention of vp_skeleton) is chi = n0 - n1 + n2 - V with n2 = (6 V + F) / 2, F = words 16 + 17 + 18: the faces of
 *               the complex follow from the exposed ones, so n2 is not stored.  Every sum fits: sum x^2 <= 1023^2 * 2^30 < 2^51, the sum
 *               of the values <= (2^32 - 1) * 2^30 < 2^62.
 *   h_stats     { sum of V, labels with V > 0, voxels with W > K (ignored), interfaces = sum of the contact faces / 2 }.
 * Every word is an integer sum, minimum or maximum, so numpy, the C++ host form, VP_ALGO_NAIVE and VP_ALGO_TILED give the same bytes whatever
 * the order of execution.
 *   vp_regions         builds the table into a grow-only buffer that the CONTEXT owns; vp_ctx_release frees it.  BLOCKS: the four totals
 *                      are read back.  count = 0 is legal: an empty table, and the statistics still report the ignored voxels.
 *   vp_regions_result  the last table, its K, the statistics and the side they are for; any argument may be NULL.  Before a build and
 *                      after a release: NULL, zeros and side 0.
 *   vp_regions_host    host in, host out (staged through workspace slots); h_values may be NULL; one of h_table / h_stats may be NULL,
 *                      not both.
 * A slab frame and n > 1024: VP_ERR_UNSUPPORTED.  Null ctx / f / labels, a buffer that is not 16-byte aligned, count above VP_REGIONS_MAX
 * (filter with vp_components_filter's minsize first), an unknown algo, an input overlapping the context's table: VP_ERR_INVALID.  Every
 * refusal leaves the previous result as it was.
 *   algo: VP_ALGO_NAIVE -- one lane per voxel from global memory: its 26 neighbours, then up to 26 global 64-bit atomics.  VP_ALGO_TILED --
 *   one workgroup per block of 32 x 16 x 16 voxels, labels and a one-voxel halo staged in LDS; a lane walks an x row and keeps the run of
 *   its current label in registers in block-local coordinates (every block-local sum but the value sum fits 32 bits), flushes it at a
 *   change of label into one of 16 label slots in LDS, and the occupied slots are shifted to grid coordinates in 64-bit arithmetic and
 *   go out with 26 global atomics per (block, label); a label that finds no free slot sends its runs straight to the table.
 *   Timing books under existing keys: the clear launch under VP_K_MD_FILL, the finishing launch under VP_K_MD_SPLIT, the TILED kernel
 *   under VP_K_MD_BRICK, the NAIVE kernel under VP_K_MD_NAIVE. */
#define VP_REGION_WORDS 26
#define VP_REGIONS_MAX 0xFFFFFu
int vp_regions(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_labels, uint32_t count, const uint32_t* d_values /* may be NULL */, int algo,
               uint64_t* h_stats /* 4, may be NULL: sum of V, labels with V > 0, voxels ignored, interfaces */);
int vp_regions_result(vp_ctx* ctx, uint64_t** d_table, uint32_t* h_count, uint64_t* h_stats /* 4 */, uint32_t* h_n);
int vp_regions_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_labels, uint32_t count, const uint32_t* h_values /* may be NULL */, int algo,
                    uint64_t* h_table /* count * 26, may be NULL */, uint64_t* h_stats /* may be NULL, not both */);

/* ---- CSG ----------------------------------------------------------------------------------
 * Stands behind CSG::Compute<Types::NAIVE,T,func>(grid1, grid2, Op) (vplib/src/csg/csg.h:35-36,
 * csg/naive.cu:26-64): d_a[i] = d_a[i] op d_b[i] with the functors of csg.h:14-30. */
int vp_csg(vp_ctx* ctx, uint32_t* d_a, const uint32_t* d_b, size_t nwords, int op);

/* ---- JFA ----------------------------------------------------------------------------------
 * Stands behind JFA::Compute<Types::NAIVE|TILED,T>(HostVoxelsGrid<T>&, HostGrid<float>&)
 * (vplib/src/jfa/jfa.h:42-43, jfa/naive.cu:121-180, jfa/tiled.cu:244-337); results are those of
 * the sequential path (jfa/sequential.cpp:7-127): signed SQUARED distance, +inside, -outside.
 *
 * State between passes is one packed id per voxel -- the coordinates of the nearest seed found so far -- instead of the
 * reference's float sdf + float3 position (jfa/sequential.cpp:69-70); distances are recomputed from it with the reference's
 * expressions.  Two layouts:
 *   PLAIN ids   vp_jfa_id_bytes(f) = 4 bytes per voxel for n <= 1024, 8 for n <= 2048, x-fastest, in planes the CALLER addresses
 *               (vp_jfa_init / vp_jfa_pass / vp_jfa_finalize below): the form of the direct kernel (VP_ALGO_NAIVE).
 *   WINDOWS     buffers in the library's own layout (vp_jfa_window_*): what the tile kernels (VP_ALGO_TILED, n >= 96) run on.
 * Id buffers are opaque either way.
 *
 * vp_jfa runs seeding + all passes + the id -> sdf conversion on one device for a whole-grid frame.
 *   fill_unset  value the caller pre-filled the sdf with (apps/cli/main.cpp:200 uses -INFINITY);
 *               must be +-infinity (a finite fill is undefined behaviour in the reference).
 *   d_work      scratch of vp_jfa_workspace_bytes(f) bytes (two id volumes + border mask), or NULL: the
 *               context then keeps a grow-only workspace of its own (work_bytes ignored).
 *   algo        VP_ALGO_NAIVE: direct kernel; VP_ALGO_TILED: tile kernels.  Same results. */
size_t vp_jfa_workspace_bytes(const vp_frame* f);
size_t vp_jfa_id_bytes(const vp_frame* f);
/* Bytes of id state per voxel that vp_jfa really streams per pass -- the S of SURVEY.md 8(d) "as implemented": 4 for n <= 1024; above
 * that 5 with VP_ALGO_TILED (windows: a 32-bit word plane + a byte plane), 8 with VP_ALGO_NAIVE.  Measurement only. */
size_t vp_jfa_state_bytes(const vp_frame* f, int algo);
/* Which tile kernels the most recent pass call of this context launched (vp_jfa_window_pass, vp_jfa_window_last_pass,
 * vp_jfa_window_pass_cyclic, and vp_jfa_pass / vp_jfa_last_pass: every one of them clears the record when it starts, so a call that is
 * refused or served by another kernel leaves it empty): one entry per launch in launch order, the template arguments of the
 * instantiation and the size of its grid.  Returns the number of launches (at most 4: a pass whose plane chains are split makes two)
 * and stores the first min(that, cap) of them in `out`; 0 for a null context.  A host-side note, no device work.  Measurement and
 * tests only: the shapes are an implementation detail and change with the kernels. */
typedef struct vp_jfa_shape {
    uint32_t id_format;   /* 9, 10: the 32-bit ids of n <= 512 / n <= 1024; 11: the compact ids above */
    uint32_t rows;        /* y rows per tile */
    uint32_t planes;      /* z planes per tile */
    uint32_t threads;     /* per workgroup */
    uint32_t final_pass;  /* 1: fused with the id -> sdf conversion */
    uint32_t pair_mode;   /* 0 (none), 1, 2, 4, 8 */
    uint32_t closed;      /* != 0: the closed 8 x 8 tile of the pass k = n/8 */
    uint32_t full;        /* 1: compile-time chain lengths */
    uint32_t cyclic;      /* 1: cyclic plane distribution */
    uint32_t tiles;       /* tiles of the launch */
    uint32_t split;       /* how many of them run as two half-row workgroups (grid = tiles + split) */
} vp_jfa_shape;
int vp_jfa_last_shapes(const vp_ctx* ctx, vp_jfa_shape* out, int cap);
int vp_jfa(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, float fill_unset,
           float* d_sdf, void* d_work, size_t work_bytes, int algo);
/* vp_jfa in the two parts the reference times separately ("::Initialization" = seeding, jfa/tiled.cu:265-290;
 * "::Processing" = the passes, jfa/tiled.cu:292-334): vp_jfa == vp_jfa_start + vp_jfa_run on the same workspace.
 * This is the sequence JFA::Compute<NAIVE|TILED> and the CLI run -- the same kernels the benchmark times.
 * The context records what vp_jfa_start left in the workspace (grid pointer, n, algo, workspace, border mask or init ids);
 * vp_jfa_run returns VP_ERR_INVALID unless exactly that start preceded it -- one start serves one run, and the record is
 * dropped when the workspace is released, regrown or freed, and when the grid buffer or the workspace is written through this ABI
 * in between.  The rule, not a list of functions: ANY output of ANY call of this ABI that lands on ANY part of the grid or of the
 * workspace (a slab of the grid, a sub-range of the workspace: the byte ranges are compared) is such a write -- grids, id planes and
 * windows, sdf and distance volumes, labels, records and mesh arrays, the explicit workspace of another vp_jfa* call -- and so are
 * vp_free of the allocation that holds it and the buffer handed out again by vp_ctx_workspace: "the same grid" means the same
 * CONTENTS -- the border mask of the start no longer describes them.  A buffer that merely touches the range (ends where it begins, begins where it ends)
 * is no write to it.  A caller that writes with its own kernels must start again itself. */
int vp_jfa_start(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, void* d_work, size_t work_bytes, int algo);
int vp_jfa_run(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, float fill_unset,
               float* d_sdf, void* d_work, size_t work_bytes, int algo);

/* The stages separately on PLAIN ids in caller-addressed planes, for Z-slab sharding (halo exchange happens between calls).
 * Halo pointers may be NULL where the slab touches the global boundary.
 *   init:  d_plane_below / d_plane_above = bitmask plane z0-1 / z1 (n*n/32 words each).
 *   pass:  step k; d_minus holds id planes [z0-k, min(z0, z1-k)), d_plus holds
 *          [max(z1, z0+k), z1+k), each clipped to the global grid but indexed from the unclipped
 *          start (plane p of d_minus is global plane z0-k+p).
 *   finalize: ids -> float sdf for the slab.
 * VP_ALGO_NAIVE serves any such buffers (the direct kernel: one thread per voxel -- the independent form the tile kernels are tested
 * against, pass by pass).  VP_ALGO_TILED: any buffers as well -- the tile kernel where the plain ids ARE a window (4-byte ids, n <= 1024,
 * and the three buffers ONE run of consecutive planes: d_minus + k planes == d_in, d_plus == d_in + the slab -- whole grids, and slabs
 * with their halo planes right below / above them), the table kernel below n = 96, the direct kernel for everything else (8-byte ids,
 * halo buffers of their own): same ids bit for bit, but not the tile kernel's speed -- hand such state over as a window for that. */
int vp_jfa_init(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words,
                const uint32_t* d_plane_below, const uint32_t* d_plane_above, void* d_ids);
int vp_jfa_pass(vp_ctx* ctx, const vp_frame* f, uint32_t k, const void* d_in,
                const void* d_minus, const void* d_plus, void* d_out, int algo);
int vp_jfa_finalize(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const void* d_ids,
                    float fill_unset, float* d_sdf);
/* The last pass (step k = 1) and the finalize in one call: where the kernel supports it the pass writes
 * the sdf directly and the id volume is neither written nor re-read; d_scratch (one id volume) is used
 * only when it does not.  Same result as vp_jfa_pass(k = 1) + vp_jfa_finalize. */
int vp_jfa_last_pass(vp_ctx* ctx, const vp_frame* f, const void* d_in, const void* d_minus,
                     const void* d_plus, void* d_scratch, const uint32_t* d_words, float fill_unset,
                     float* d_sdf, int algo);

/* Id WINDOWS: the slab form of the tile kernels (VP_ALGO_TILED, n >= 96) -- what the multi-GPU pipelines run (cuda_mesh_voxelization_amd/slab.py,
 * vp_multi_* below), and what vp_jfa itself runs on its workspace.  A window is a buffer of `planes` id planes in the library's layout:
 * vp_jfa_window_bytes(f, planes) bytes -- 4-byte ids up to n = 1024; above that `planes` planes of 32-bit words followed by `planes`
 * planes of bytes (5 instead of 8 bytes per voxel in memory, per pass and on the wire).  A call names a frame f (the planes [z0, z1) it
 * produces) and says where plane z0 sits in the window (`at`); the planes around it are the halo the pass reads.  Nothing else is
 * assumed about which global planes a window holds: a ghost-plane pipeline keeps whole volumes (planes = n, at = z0), a hybrid one the
 * planes a rank touches, a halo pipeline its slab with room for the halos on both sides.
 *   stride  where the planes z - k and z + k of a plane z are found: `stride` planes below / above it.  stride = k for a window of
 *           consecutive planes.  A pass whose step spans whole slabs (k >= z1 - z0: the wide passes of a halo pipeline) keeps
 *           [slab holding z - k | own slab | slab holding z + k] and passes stride = the slab height: the tile kernel then runs on the
 *           received slabs where they landed.
 *   vp_jfa_window_span     where the planes [p0, p1) of a window live, for whoever moves them (halo exchange): one or two byte ranges
 *                          relative to d_ids (bytes[1] = 0 for 4-byte ids)
 *   vp_jfa_window_clear    every id := "none" (a pipeline whose regions are rounded outwards to whole tiles reads planes nobody
 *                          produced: cleared once, they hold ids of the window's own layout -- never stale bytes of another one)
 *   vp_jfa_window_init     seeding: ids of the planes of f from its bitmask (halo planes as in vp_jfa_init)
 *   vp_jfa_window_first_pass   the pass k = n/2 of the planes of f straight from the border bitmask of the WHOLE grid (vp_surface on
 *                          a whole-grid frame): no init ids are written or read (jfa/sequential.cpp:55-60: before any pass a border
 *                          voxel's seed is itself and nothing else has one).  n % 128 == 0 (vp_jfa_can_start_from_mask).
 *   vp_jfa_window_first_two    the passes k = n/2 AND k = n/4 of a WHOLE grid in one launch from its border bitmask; whole-grid frame,
 *                          a window of n planes, at = 0 (vp_jfa_can_fuse_first_two: any n >= 96)
 *   vp_jfa_window_pass     one pass with step k over the planes of f: reads `in` (the planes of f and `stride` planes on each side of
 *                          them, as far as the grid goes), writes the planes of f in `out` (same planes / at as `in`)
 *   vp_jfa_window_last_pass    step 1 fused with the id -> sdf conversion; d_words_region / d_sdf_region hold the planes [z0, z1) only
 * Same results as the plain-id calls, bit for bit. */
typedef struct vp_window {
    void*    d_ids;       /* the buffer, 16-byte aligned */
    size_t   bytes;       /* its size: at least vp_jfa_window_bytes(f, planes) -- checked by every call (VP_ERR_INVALID) */
    uint32_t planes;      /* id planes the buffer holds (the layout depends on it: above n = 1024 the byte planes follow `planes` word planes) */
    uint32_t at;          /* index inside the buffer of plane z0 of the frame given with it */
} vp_window;
size_t vp_jfa_window_bytes(const vp_frame* f, uint32_t planes);
int vp_jfa_window_span(const vp_frame* f, uint32_t planes, uint32_t p0, uint32_t p1, size_t offset[2], size_t bytes[2]);
int vp_jfa_window_clear(vp_ctx* ctx, const vp_frame* f, const vp_window* w);
int vp_jfa_window_init(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, const uint32_t* d_plane_below,
                       const uint32_t* d_plane_above, const vp_window* out);
int vp_jfa_can_start_from_mask(const vp_frame* f, int algo);
int vp_jfa_window_first_pass(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_border_grid, const vp_window* out);
int vp_jfa_can_fuse_first_two(const vp_frame* f, int algo);
int vp_jfa_window_first_two(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_border_grid, const vp_window* out);
int vp_jfa_window_pass(vp_ctx* ctx, const vp_frame* f, uint32_t k, const vp_window* in, const vp_window* out, uint32_t stride);
int vp_jfa_window_last_pass(vp_ctx* ctx, const vp_frame* f, const vp_window* in, const vp_window* scratch, uint32_t stride,
                            const uint32_t* d_words_region, float fill_unset, float* d_sdf_region);

/* CYCLIC plane distribution -- the first phase of the transposed multi-GPU pipeline (VP_MULTI_TRANSPOSE below).
 * The reference's pass with step k reads, for a voxel of plane z, the planes z - k, z, z + k and nothing else (jfa/sequential.cpp:72: k = n/2
 * .. 1; :86-94: neighbours at -+k).  With the planes dealt cyclically over G ranks -- plane z on rank z mod G, kept at index z / G of that
 * rank's window of n / G planes -- every pass whose step is a multiple of G finds all three planes on the rank that owns z: no exchange at
 * all, chains of full length, and each rank does exactly 1/G of the pass.  G a power of two, n / G a multiple of 8 planes.
 *   vp_jfa_cyclic_passes            how many passes of the sequence n/2, n/4, ... have such a step, counted from the first (0: none, or fewer
 *                                   than the two the fused start produces -- use another pipeline)
 *   vp_jfa_window_first_two_cyclic  the passes k = n/2 and k = n/4 of rank `rank`'s planes from the border bitmask of the WHOLE grid
 *                                   (vp_jfa_window_first_two restricted to the tiles of the rank's z residues); whole-grid frame, a window of
 *                                   n / ranks planes, at = 0
 *   vp_jfa_window_pass_cyclic       one pass with step k (a multiple of `ranks`, one of the first vp_jfa_cyclic_passes steps) over rank `rank`'s
 *                                   planes; whole-grid frame, two windows of n / ranks planes, at = 0.  Ids hold global coordinates, so the
 *                                   planes can be handed to the slab form of the calls above as they are
 *   vp_jfa_window_interleave        the re-deal into slabs: `in` holds `ranks` chunks of `count` planes, chunk s = the planes b0 + s, b0 + s +
 *                                   ranks, ... of some run of ranks * count consecutive planes as rank s kept them (what an all-to-all of
 *                                   contiguous plane ranges delivers); plane out->at + j * ranks + s of `out` := plane s * count + j of `in`.
 *                                   `in` is a window of exactly ranks * count planes (in->at ignored)
 * Same results as the consecutive-plane calls, id for id. */
int vp_jfa_cyclic_passes(const vp_frame* f, uint32_t ranks);
int vp_jfa_window_first_two_cyclic(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_border_grid, const vp_window* out, uint32_t ranks, uint32_t rank);
int vp_jfa_window_pass_cyclic(vp_ctx* ctx, const vp_frame* f, uint32_t k, const vp_window* in, const vp_window* out, uint32_t ranks, uint32_t rank);
int vp_jfa_window_interleave(vp_ctx* ctx, const vp_frame* f, const vp_window* in, const vp_window* out, uint32_t ranks, uint32_t count);

/* "Surface" output (README.md:9): the border-voxel mask that JFA seeds
 * from (jfa/sequential.cpp:24-64), as a bitmask with the grid's layout. */
int vp_surface(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words,
               const uint32_t* d_plane_below, const uint32_t* d_plane_above, uint32_t* d_border_words);

/* ---- export: ordered compaction of the grid into voxel records --------------------------------
 * The reference's exporters walk all n^3 voxels on the CPU (vplib/src/mesh/grid_to_mesh.cpp:10-201); this is the
 * accelerated front end: the walk is a GPU stream and the host only sees the voxels it will emit, in the exporter's own
 * scan order (z, y, x), so the files it writes are byte-identical.  Whole-grid frames only.
 *   mode VP_EXTRACT_SET      every set voxel (point cloud, sdf cubes: grid_to_mesh.cpp:133-201)
 *   mode VP_EXTRACT_EXPOSED  set voxels with a face towards an unset voxel or the outside of the grid, with the mask of
 *                            those faces (visible-surface mesh)
 *   mode VP_EXTRACT_FACES    every set voxel, with that mask: VoxelsGridToMeshCompressed (grid_to_mesh.cpp:10-60, grid_to_mesh.h:25-92)
 *                            emits every face of every set voxel ONCE, interior faces included -- the three faces on a voxel's plus sides
 *                            always, a face on a minus side iff the voxel behind it is unset (else that voxel emitted it already)
 *   record = linear voxel index x + n (y + n z) in bits 0..39 | face mask << 40 (bit = axis * 2 + side; X, Y, Z; 0 = minus)
 * vp_extract_count runs the counting pass and returns the number of records (blocking); vp_extract then writes up to
 * `capacity` records (and, when d_sdf and d_values are given, the sdf value of each voxel) -- it must follow a count call for
 * the same grid and mode, else VP_ERR_INVALID.  "Same grid" means same contents: the count is forgotten as soon as any part of
 * d_words is written through this ABI -- the rule stated at vp_jfa_start: any output of any call of this ABI whose byte range
 * overlaps the grid's, vp_extract's own d_records / d_values included --, freed, or handed out again by vp_ctx_workspace; a caller
 * that writes the buffer with its own kernels must count again itself. */
enum { VP_EXTRACT_SET = 0, VP_EXTRACT_EXPOSED = 1, VP_EXTRACT_FACES = 2 };
int vp_extract_count(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int mode, uint64_t* h_count);
int vp_extract(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int mode, const float* d_sdf,
               uint64_t* d_records, float* d_values, size_t capacity);

/* ---- several GPUs of one node: Z-slabs -------------------------------------------------------
 * Replaces the reference's hard-wired device 0 (apps/cli/main.cpp:22-23) when more than one device is given: ONE process,
 * one context per device, rank r owns the planes [r n/G, (r+1) n/G) of the grid and of the sdf; G must divide n
 * into slabs of a multiple of 8 planes.  The stages are the slab forms of the calls above (vp_frame.z0 / z1); the JFA state of a rank
 * lives in two id windows (vp_jfa_window_*):
 *   voxelize / CSG   no exchange (columns and words are independent)
 *   JFA              VP_MULTI_HALO : windows of 3 n/G planes, [slab holding z - k | own slab | slab holding z + k].  Bitmask planes z0-1 /
 *                                    z1 before the seeding and, before the pass with step k, the id planes [z0-k, min(z0, z1-k)),
 *                                    [max(z1, z0+k), z1+k) travel device to device (hipMemcpyPeerAsync behind stream events; no host
 *                                    synchronisation inside the JFA): next to the slab for k <= n/2G, a slab height away for the steps
 *                                    that span whole slabs (stride = n/G, see vp_jfa_window_pass)
 *                    VP_MULTI_GHOST: the bitmask slabs are all-gathered once (n^3/8 bytes) and every device recomputes the
 *                                    ghost planes its later passes reach: no exchange between passes, two windows of the whole grid
 *                                    per device
 *                    VP_MULTI_HYBRID: ghost planes for the passes with k > nz/2 (as far as the later such passes reach), halo
 *                                    planes from the two adjacent devices for the passes with k <= nz/2; the windows hold only
 *                                    the planes a device touches (vp_multi_window): capacity, not speed
 *                    VP_MULTI_TRANSPOSE: the planes are dealt cyclically (plane z on device z mod G) for every pass whose step is a multiple
 *                                    of G -- no exchange, no ghost planes, 1/G of each pass per device (vp_jfa_window_*_cyclic) -- then ONE
 *                                    re-deal into slabs widened by the reach of the remaining log2 G passes: one peer copy per pair of
 *                                    devices, n^3 S / G + margins bytes into each device per job (0.49 GiB at n = 1024, G = 8, against
 *                                    3.5 GiB of halos), compute per device ~ 1 / G of one device's.  G a power of two; where no step is a
 *                                    multiple of G it is the ghost mode
 * Results are bit-identical to the single-device calls for any G.  The sharded forms run the tile kernels whatever `algo` says (both
 * algorithms give the same sdf); grids below their range (n < 96) are not sharded: every device computes the whole grid with `algo`
 * and keeps its slab.  `devices` may name one device several times (several
 * contexts on it): that is how the parity tests run on a one-GPU box.  Grid, sdf and mesh stay resident on the devices
 * between calls; host arrays are whole-grid arrays in the reference's layout. */
typedef struct vp_multi vp_multi;
enum { VP_MULTI_HALO = 0, VP_MULTI_GHOST = 1, VP_MULTI_HYBRID = 2, VP_MULTI_TRANSPOSE = 3 };
int vp_multi_create(const int* devices, int ndev, vp_multi** out);
int vp_multi_destroy(vp_multi* m);
int vp_multi_count(const vp_multi* m);
vp_ctx* vp_multi_ctx(vp_multi* m, int rank);                      /* the context of a rank (timers, stream) */
int vp_multi_sync(vp_multi* m);
/* broadcast of the mesh to every device (blocking) -- Mesh::Coords / Mesh::FacesCoords as in vp_voxelize */
int vp_multi_set_mesh(vp_multi* m, const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris);
/* every device rasterises the resident mesh into its slab of a fresh grid with frame f (async) */
int vp_multi_voxelize(vp_multi* m, const vp_frame* f, int algo);
/* scatter a host grid into the slabs / gather the slabs (blocking) */
int vp_multi_set_grid(vp_multi* m, const vp_frame* f, const uint32_t* h_words);
int vp_multi_get_grid(vp_multi* m, uint32_t* h_words);
/* resident grid = resident grid op h_other (CSG::Compute's "result in the first grid", csg/naive.cu:62); blocking.
 * nwords = words of h_other; must equal the resident grid's (the reference requires equal grids, csg/naive.cu:30-33). */
int vp_multi_csg(vp_multi* m, const uint32_t* h_other, size_t nwords, int op);
/* JFA of the resident grid into the resident slab sdfs (async); vp_multi_get_sdf gathers them (blocking) */
int vp_multi_jfa(vp_multi* m, float fill_unset, int algo, int mode);
int vp_multi_get_sdf(vp_multi* m, float* h_sdf);
/* device-to-device bytes the last vp_multi_jfa enqueued (halo planes / the bitmask all-gather) */
uint64_t vp_multi_bytes_moved(const vp_multi* m);
/* JFA state a rank held during the last vp_multi_jfa: the global planes [lo, hi) its two id windows are addressed by -- the whole grid with
 * VP_MULTI_GHOST, the slab with VP_MULTI_HALO (its windows also hold the two slabs received from z -+ k), the planes the rank touches
 * with VP_MULTI_HYBRID, the widened slab of the second phase with VP_MULTI_TRANSPOSE -- and the bytes of device memory in the id windows
 * THAT job used (not those an earlier job of another side or mode left allocated; 0 below n = 96, where the grid is not sharded and no id
 * window is used).  Any out pointer may be NULL. */
int vp_multi_window(const vp_multi* m, int rank, uint32_t* lo, uint32_t* hi, uint64_t* id_bytes);

/* ---- host-in / host-out conveniences (the reference's Compute() calling convention) -------
 * Upload, run, download, synchronise -- what every reference Compute<NAIVE|TILED> does
 * (vox/tiled.cu:504-575, csg/naive.cu:38-63, jfa/tiled.cu:254-336).  Whole-grid frames only. */
int vp_voxelize_host(vp_ctx* ctx, const vp_frame* f, uint32_t* h_words,
                     const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris, int algo);
int vp_csg_host(vp_ctx* ctx, uint32_t* h_a, const uint32_t* h_b, size_t nwords, int op);
int vp_jfa_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, float fill_unset,
                float* h_sdf, int algo);
/* vp_voxelize_conservative with the convention above (whole-grid frame, overwrite) */
int vp_voxelize_conservative_host(vp_ctx* ctx, const vp_frame* f, uint32_t* h_words,
                                  const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris, int algo);
/* vp_fill_interior with the convention above (whole-grid frame); staged through workspace slots, so h_out may equal h_words */
int vp_fill_interior_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out);

/* vp_morph with the convention above (whole-grid frame); staged through workspace slots, so h_out may equal h_words */
int vp_morph_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out, int op, uint32_t radius, int algo);

/* vp_components_label / vp_components_filter with the convention above (whole-grid frame); staged through workspace slots.  h_labels holds
 * n^3 uint32; h_out may equal h_words. */
int vp_components_label_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_labels, int connectivity, int algo,
                             uint32_t* h_count);
int vp_components_filter_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out, int connectivity, int mode,
                              uint32_t param, int algo, uint32_t* h_count, uint64_t* h_kept);

/* vp_surfnets_count + vp_surfnets (VP_ALGO_TILED) with the convention above (whole-grid frame); staged through workspace slots.
 * *h_vertices = V and *h_quads_out = Q always; h_cells = h_xyz = h_quads = NULL: counts only; otherwise all three are written, and a
 * capacity below V / Q is VP_ERR_INVALID (the counts are not stored then). */
int vp_surfnets_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t iterations, uint64_t* h_cells, float* h_xyz,
                     uint32_t* h_quads, size_t vertex_capacity, size_t quad_capacity, uint64_t* h_vertices, uint64_t* h_quads_out);

/* vp_edt / vp_edt_sdf / vp_edt_morph with the convention above (whole-grid frame); staged through workspace slots.  h_dist2 and h_sdf hold
 * n^3 values; h_out may equal h_words. */
int vp_edt_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, int seeds, uint32_t* h_dist2, int algo);
int vp_edt_sdf_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, float fill_unset, float* h_sdf, int algo);
int vp_edt_morph_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t* h_out, int op, uint32_t radius, int algo);

/* vp_mesh_distance with the convention above (whole-grid frame): mesh and sign grid up, the field and the nearest faces down; staged
 * through workspace slots.  h_sign_words and h_nearest may be NULL; h_dist2 and h_nearest hold n^3 values. */
int vp_mesh_distance_host(vp_ctx* ctx, const vp_frame* f, const float* h_xyz, size_t nverts, const uint32_t* h_tri, size_t ntris,
                          const uint32_t* h_sign_words, uint32_t band, float* h_dist2, uint32_t* h_nearest, int algo);

/* ---- per-kernel timing (PROFILING_SCOPE equivalent for device time, vplib/src/profiling.h:8-33)
 * When enabled, every kernel launch is bracketed by hipEvents on the context's stream. */
enum {
    VP_K_VOX_SETUP = 0, VP_K_VOX_SCAN, VP_K_VOX_SCATTER, VP_K_VOX_TILE, VP_K_VOX_NAIVE,
    VP_K_VOX_FILL, VP_K_CSG, VP_K_JFA_INIT,
    VP_K_JFA_PASS,      /* direct kernel (VP_ALGO_NAIVE) and the small-grid table kernel (n < 96) */
    VP_K_JFA_FINAL, VP_K_SURFACE,
    /* the tile kernels of VP_ALGO_TILED (n >= 96), one key per variant -- their algorithmic bytes differ: */
    VP_K_JFA_FIRST,     /* k = n/2 straight from the border mask: 4 n^3 + n^3/8 bytes (S = 4) */
    VP_K_JFA_SPARSE,    /* k >= n/4: 2 S n^3 */
    VP_K_JFA_DENSE,     /* k <  n/4: 2 S n^3 */
    VP_K_JFA_LAST,      /* k = 1 fused with the id -> sdf conversion: S n^3 + 4 n^3 + n^3/8 */
    VP_K_EXTRACT,       /* vp_extract_count / vp_extract: 2 n^3/8 + records */
    VP_K_VOX_ZERO,      /* the voxelizer's zero-fill of the toggle grid (+ the tile histogram): n^3/8 */
    VP_K_JFA_REDEAL,    /* vp_jfa_window_interleave: 2 S x the planes woven */
    /* vp_voxelize_conservative: */
    VP_K_CVOX_ZERO,     /* zero-fill of the grid (overwrite) and of the large-triangle counter: n^3/8 */
    VP_K_CVOX_SETUP,    /* TILED: triangle setup, small triangles rasterised */
    VP_K_CVOX_SCAN,     /* TILED: row scan of the large-triangle list */
    VP_K_CVOX_ROWS,     /* TILED: the rows of the large triangles */
    VP_K_CVOX_NAIVE,    /* NAIVE: one thread per triangle */
    /* vp_fill_interior (per round; rounds after convergence return at once): */
    VP_K_FILL_X,        /* x sweep (round 0: seeds the six faces): 2 n^3/8 read + n^3/8 written */
    VP_K_FILL_Y,        /* y sweep: three walks over each column segment, 6 n^3/8 read + up to 2 n^3/8 written */
    VP_K_FILL_Z,        /* z sweep: as y */
    VP_K_FILL_FINAL,    /* out = NOT exterior: 2 n^3/8 */
    /* vp_morph (open and close book two launches): */
    VP_K_MORPH,         /* VP_ALGO_TILED, one dilate or erode pass: 2 n^3/8 algorithmic bytes */
    VP_K_MORPH_NAIVE,   /* VP_ALGO_NAIVE, one pass */
    /* vp_components_label (the first seven) and vp_components_sizes / vp_components_filter: */
    VP_K_COMP_INIT,         /* TILED: every set voxel points at the start of its x run: n^3/8 read + 4 n^3 written */
    VP_K_COMP_MERGE,        /* TILED: one union per pair of adjacent runs: up to 5 n^3/8 read + the unions (data-dependent) */
    VP_K_COMP_INIT_NAIVE,   /* NAIVE: P[v] = v: n^3/8 + 4 n^3 */
    VP_K_COMP_MERGE_NAIVE,  /* NAIVE: one union per set voxel and set backward neighbour: n^3/8 + the unions */
    VP_K_COMP_FLATTEN,      /* every set voxel takes its root, roots counted per 8192 voxels: 4 n^3 read + up to 4 n^3 written */
    VP_K_COMP_RANK,         /* scan of the n^3/8192 counts + the roots take their rank: 4 n^3 read + 4 K written */
    VP_K_COMP_RELABEL,      /* ranks -> labels: 4 n^3 read + 4 n^3 written + one gather per set voxel */
    VP_K_COMP_SIZES,        /* 4 n^3 read + the adds */
    VP_K_COMP_SELECT,       /* MIN_VOXELS: 5 K; KEEP_LARGEST m: min(m, K) rounds of 4 K */
    VP_K_COMP_WRITE,        /* 4 n^3 read + n^3/8 written + one gather per set voxel */
    VP_K_COUNT
};
/* the keys of vp_surfnets_count / vp_surfnets follow the enum above (bit i of vp_prof_select = key i, 64 at the most) */
enum {
    VP_K_SN_CELLS = VP_K_COUNT, /* TILED, count: corner words -> active-cell bits + block counts: about 2 n^3/8 */
    VP_K_SN_SCAN,               /* both algos: one-workgroup scan of the two block-count arrays */
    VP_K_SN_VERTS,              /* TILED: per-word exclusive counts, records, starting positions: n^3/8 read, n^3/8 + 20 V written */
    VP_K_SN_QUADS,              /* TILED: n^3/8 read + four rank gathers per quad, 16 Q written */
    VP_K_SN_RELAX,              /* TILED, one Jacobi step: 20 V read + up to six gathers per vertex, 12 V written */
    VP_K_SN_CELLS_NAIVE,        /* NAIVE, count: eight bit reads per cell */
    VP_K_SN_VERTS_NAIVE,        /* NAIVE: index volume 4 (n+1)^3 written + 20 V */
    VP_K_SN_QUADS_NAIVE,        /* NAIVE: four index reads per quad, 16 Q written */
    VP_K_SN_RELAX_NAIVE,        /* NAIVE, one Jacobi step */
    VP_K_TOTAL
};
/* the keys of vp_edt / vp_edt_sdf / vp_edt_morph follow the second enum (all three together: 64 keys at the most) */
enum {
    VP_K_EDT_X = VP_K_TOTAL,    /* both algos: bit words -> dx^2: n^3/8 read + 4 n^3 written */
    VP_K_EDT_Y,                 /* TILED, y pass in place: 4 n^3 read + up to 4 n^3 written (bundles without a seed write nothing) */
    VP_K_EDT_Z,                 /* TILED, z pass in place: as y */
    VP_K_EDT_Y_NAIVE,           /* NAIVE, y pass into the second volume: 8 n^3 + the search */
    VP_K_EDT_Z_NAIVE,           /* NAIVE, z pass back: as y */
    VP_K_EDT_SDF,               /* D -> sdf in place: n^3/8 + 4 n^3 read, 4 n^3 written */
    VP_K_EDT_THRESH,            /* D -> bit words: 4 n^3 read, n^3/8 written */
    VP_K_END
};
/* the keys of vp_mesh_distance follow the third enum.  THE MASK IS NOW FULL: the four enums together hold exactly 64 keys, the width of
 * vp_prof_select's mask (md_offsets and md_plane_sums already share the keys of md_scan and md_count for that reason).  The next kernel
 * that wants a key of its own needs a wider mask, i.e. a new vp_prof_select and a new VP_ABI_VERSION; until then it shares a key. */
enum {
    VP_K_MD_SETUP = VP_K_END,   /* TILED: triangle records, brick ranges and row counts: 36 T read + 100 T written (T triangles) */
    VP_K_MD_SCAN,               /* TILED: one-workgroup scans that read their counts twice: the triangles' row counts (8 T read + 8 T written); per z range the brick counts (8 B read + 8 B written per brick) */
    VP_K_MD_COUNT,              /* TILED: brick test per (triangle, brick) of every brick row, one add per listed pair; + the plane sums (4 B per brick) */
    VP_K_MD_WRITE,              /* TILED: the same walk, 4 B written per list entry L */
    VP_K_MD_BRICK,              /* TILED: 4 L + 96 L read (records, mostly from L2), 4 or 8 B written per voxel of a listed brick */
    VP_K_MD_FILL,               /* both algos: bricks without a list (ntris = 0: all): n^3/8 sign bits read, 4 or 8 B per voxel written */
    VP_K_MD_PREFILL,            /* NAIVE: 8 n^3 written */
    VP_K_MD_NAIVE,              /* NAIVE: 36 T read + one 8-byte atomic per accepted pair */
    VP_K_MD_SPLIT,              /* NAIVE: 8 n^3 + n^3/8 read, 4 or 8 n^3 written */
    VP_K_ALL
};
int vp_prof_enable(vp_ctx* ctx, int on);
/* Restricts the bracketing to the keys whose bit is set (bit i = key i; default: all).  An event pair costs ~3 us of stream
 * time (0.11 ms over the 18 launches of a 512^3 step, 3 %): a caller that times ONE kernel inside a wall-clock region
 * selects just that key. */
int vp_prof_select(vp_ctx* ctx, uint64_t kernel_mask);
int vp_prof_reset(vp_ctx* ctx);
/* Synchronises the stream, folds pending events in, returns total ms and launch count. */
int vp_prof_get(vp_ctx* ctx, int kernel, double* total_ms, uint64_t* launches);
const char* vp_prof_name(int kernel);

#ifdef __cplusplus
}
#endif
#endif /* VPHIP_H */
