"""ctypes binding of libvphip.so (include/vphip.h) -- the only way the Python harness reaches
the HIP kernels.  There is no fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# VPHIP_LIB: another build of the library -- dev experiments (tools/exp_build.sh) and the tests that need libvphip_hooks.so
LIB_PATH = os.environ.get("VPHIP_LIB") or os.path.join(PKG, "libvphip.so")
HOOKS_LIB_PATH = os.path.join(PKG, "libvphip_hooks.so")

ALGO_NAIVE, ALGO_TILED = 1, 2
OP_VOID, OP_UNION, OP_INTERSECTION, OP_DIFFERENCE = 0, 1, 2, 3
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3     # vp_morph: ball morphology
EDT_SEEDS_SET, EDT_SEEDS_UNSET, EDT_SEEDS_BORDER = 0, 1, 2              # vp_edt: which voxels the distances are measured to
EDT_NONE = 0xFFFFFFFF                                               # vp_edt: "the grid has no seed"
MESH_NONE = 0xFFFFFFFF                                              # vp_mesh_distance: "no triangle within the band"
ISO_LINEAR, ISO_SIGNED_SQUARE = 0, 1                                # vp_isonets: the field as it is / sign(v) sqrt|v| (every sdf of the library)
CONN_6, CONN_26 = 6, 26                                             # vp_components_*: face / face + edge + corner neighbours
SKEL_KERNEL, SKEL_CURVE = 0, 1                                      # vp_skeleton: the homotopy kernel / the centre line (line ends stay)
GEO_6, GEO_26, GEO_CHAMFER = 0, 1, 2                                # vp_geodesic: face steps / all 26 steps at cost 1 / at cost 3, 4, 5
REC_DILATION, REC_EROSION = 0, 1                                    # vp_reconstruct: by dilation (raise the marker under the mask) / by erosion
EXT_MAXIMA, EXT_MINIMA = 0, 1                                       # vp_extrema: h-maxima / h-minima
EXT_LINEAR, EXT_SQRT16 = 0, 1                                       # vp_extrema: the values as they are / floor(sqrt(256 v))
WS_ASCENDING, WS_DESCENDING = 0, 1                                  # vp_watershed: flood from low / from high priority
WS_LABEL_MAX, WS_MAX_SPAN = 0xFFFFF, 16384                          # vp_watershed: the largest marker label, the bound of the level span
REGION_WORDS, REGIONS_MAX = 26, 0xFFFFF                             # vp_regions: uint64 words per record, the largest label count
GEO_NONE = 0xFFFFFFFF                                               # vp_geodesic: "no path from a seed arrives here"
COMP_KEEP_LARGEST, COMP_MIN_VOXELS = 0, 1                           # vp_components_filter modes
EXTRACT_SET, EXTRACT_EXPOSED, EXTRACT_FACES = 0, 1, 2
MULTI_HALO, MULTI_GHOST, MULTI_HYBRID, MULTI_TRANSPOSE = 0, 1, 2, 3

KERNELS = ["vox_setup", "vox_scan", "vox_scatter", "vox_tile", "vox_naive", "vox_fill",
           "csg_words", "jfa_init", "jfa_pass", "jfa_final", "surface", "jfa_first", "jfa_sparse", "jfa_dense", "jfa_last", "extract", "vox_zero", "jfa_redeal",
           "cvox_zero", "cvox_setup", "cvox_scan", "cvox_rows", "cvox_naive",
           "fill_x", "fill_y", "fill_z", "fill_final",
           "morph", "morph_naive"]
# the timing keys of vp_components_* follow those of KERNELS in the header's enum (PROF_KEYS is the whole enum, in its order)
COMP_KERNELS = ["comp_init", "comp_merge", "comp_init_naive", "comp_merge_naive", "comp_flatten", "comp_rank", "comp_relabel", "comp_sizes",
                "comp_select", "comp_write"]
PROF_KEYS = KERNELS + COMP_KERNELS
# the timing keys of vp_surfnets_* are a second enum of the header that starts where the first ends (= VP_K_COUNT): ALL_PROF_KEYS is
# every key in its numbering, the list prof() and prof_select() look names up in
SURFNETS_KERNELS = ["sn_cells", "sn_scan", "sn_verts", "sn_quads", "sn_relax", "sn_cells_naive", "sn_verts_naive", "sn_quads_naive",
                    "sn_relax_naive"]
ALL_PROF_KEYS = PROF_KEYS + SURFNETS_KERNELS
# the timing keys of vp_edt* are a third enum that starts where the second ends (= VP_K_TOTAL): EVERY_PROF_KEY is every key of the header
# (VP_K_END of them) in its numbering -- what prof() and prof_select() look names up in
EDT_KERNELS = ["edt_x", "edt_y", "edt_z", "edt_y_naive", "edt_z_naive", "edt_sdf", "edt_thresh"]
EVERY_PROF_KEY = ALL_PROF_KEYS + EDT_KERNELS
# the keys of vp_mesh_distance are a fourth enum behind the third (= VP_K_END); HEADER_PROF_KEYS is every key of the header, VP_K_ALL of them
MESHDIST_KERNELS = ["md_setup", "md_scan", "md_count", "md_write", "md_brick", "md_fill", "md_prefill", "md_naive", "md_split"]
HEADER_PROF_KEYS = EVERY_PROF_KEY + MESHDIST_KERNELS
JFA_PASS_KEYS = ("jfa_pass", "jfa_first", "jfa_sparse", "jfa_dense", "jfa_last")

# every symbol include/vphip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "vp_device_count", "vp_ctx_create", "vp_ctx_destroy", "vp_ctx_set_stream", "vp_ctx_sync", "vp_last_error", "vp_abi_version",
    "vp_malloc", "vp_free", "vp_memset", "vp_memcpy_d2d", "vp_stream_copy", "vp_ctx_workspace", "vp_ctx_release", "vp_upload", "vp_download",
    "vp_grid_words", "vp_grid_voxels",
    "vp_voxelize", "vp_csg", "vp_jfa_workspace_bytes", "vp_jfa_id_bytes", "vp_jfa_state_bytes", "vp_jfa_last_shapes", "vp_jfa", "vp_jfa_start", "vp_jfa_run", "vp_jfa_init", "vp_jfa_pass",
    "vp_jfa_finalize", "vp_jfa_last_pass", "vp_jfa_can_start_from_mask", "vp_jfa_can_fuse_first_two",
    "vp_jfa_window_bytes", "vp_jfa_window_span", "vp_jfa_window_clear", "vp_jfa_window_init", "vp_jfa_window_first_pass", "vp_jfa_window_first_two",
    "vp_jfa_window_pass", "vp_jfa_window_last_pass",
    "vp_jfa_cyclic_passes", "vp_jfa_window_first_two_cyclic", "vp_jfa_window_pass_cyclic", "vp_jfa_window_interleave",
    "vp_surface", "vp_extract_count", "vp_extract", "vp_voxelize_host", "vp_csg_host", "vp_jfa_host",
    "vp_prof_enable", "vp_prof_select", "vp_prof_reset", "vp_prof_get", "vp_prof_name",
    "vp_multi_create", "vp_multi_destroy", "vp_multi_count", "vp_multi_ctx", "vp_multi_sync", "vp_multi_set_mesh", "vp_multi_voxelize",
    "vp_multi_set_grid", "vp_multi_get_grid", "vp_multi_csg", "vp_multi_jfa", "vp_multi_get_sdf", "vp_multi_bytes_moved", "vp_multi_window",
    "vp_voxelize_conservative", "vp_voxelize_conservative_host",
    "vp_fill_interior", "vp_fill_interior_host",
    "vp_morph", "vp_morph_host",
    "vp_components_label", "vp_components_sizes", "vp_components_filter", "vp_components_label_host", "vp_components_filter_host",
    "vp_surfnets_count", "vp_surfnets", "vp_surfnets_host", "vp_isonets", "vp_isonets_result", "vp_isonets_host",
    "vp_edt", "vp_edt_sdf", "vp_edt_morph", "vp_edt_host", "vp_edt_sdf_host", "vp_edt_morph_host",
    "vp_mesh_distance", "vp_mesh_distance_host", "vp_mesh_distance_stats",
    "vp_winding", "vp_winding_result", "vp_winding_host",
    "vp_thickness", "vp_thickness_result", "vp_thickness_host",
    "vp_octree", "vp_octree_result", "vp_octree_expand", "vp_octree_expand_result", "vp_octree_host", "vp_octree_expand_host", "vp_octree_validate_host",
    "vp_skeleton", "vp_skeleton_result", "vp_skeleton_host", "vp_skeleton_table_host",
    "vp_geodesic", "vp_geodesic_result", "vp_geodesic_host",
    "vp_watershed", "vp_watershed_result", "vp_watershed_host",
    "vp_regions", "vp_regions_result", "vp_regions_host",
    "vp_reconstruct", "vp_reconstruct_result", "vp_reconstruct_host",
    "vp_extrema", "vp_extrema_result", "vp_extrema_host",
]


class VPError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libvphip error %d: %s" % (code, msg))
        self.code = code


class Frame(ctypes.Structure):
    """vp_frame: global grid side n, voxel size, origin, Z-slab [z0, z1)."""
    _fields_ = [("n", ctypes.c_uint32), ("voxel_size", ctypes.c_float), ("origin", ctypes.c_float * 3),
                ("z0", ctypes.c_uint32), ("z1", ctypes.c_uint32)]

    @classmethod
    def make(cls, n, voxel_size, origin, z0=0, z1=None):
        f = cls()
        f.n = int(n)
        f.voxel_size = float(voxel_size)
        f.origin[0], f.origin[1], f.origin[2] = float(origin[0]), float(origin[1]), float(origin[2])
        f.z0 = int(z0)
        f.z1 = int(n if z1 is None else z1)
        return f

    @property
    def nz(self):
        return self.z1 - self.z0

    @property
    def words(self):
        return self.n * self.n * self.nz // 32

    @property
    def voxels(self):
        return self.n * self.n * self.nz

    def slab(self, z0, z1):
        return Frame.make(self.n, self.voxel_size, self.origin, z0, z1)


class Window(ctypes.Structure):
    """vp_window: an id buffer in the library's layout -- `planes` id planes, plane z0 of the frame a call is made with at index `at`."""
    _fields_ = [("d_ids", ctypes.c_void_p), ("bytes", ctypes.c_size_t), ("planes", ctypes.c_uint32), ("at", ctypes.c_uint32)]

    @classmethod
    def make(cls, d_ids, nbytes, planes, at):
        """nbytes: the size of the buffer (every call checks it against vp_jfa_window_bytes of `planes` planes)"""
        w = cls()
        w.d_ids, w.bytes, w.planes, w.at = int(d_ids), int(nbytes), int(planes), int(at)
        return w


class JfaShape(ctypes.Structure):
    """vp_jfa_shape: one tile-kernel launch of the most recent pass call (vp_jfa_last_shapes; measurement and tests only)."""
    _fields_ = [(name, ctypes.c_uint32) for name in ("id_format", "rows", "planes", "threads", "final_pass", "pair_mode", "closed", "full",
                                                      "cyclic", "tiles", "split")]


_lib = None
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


def lib():
    """Load libvphip.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libvphip.so is missing at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
    # Load order: torch ships its own libamdhip64.so, libvphip.so is linked against the one of /opt/rocm.  Whichever is mapped first serves
    # both (same SONAME); if libvphip.so comes first and torch initialises the GPU afterwards, the process ends up with two HIP runtimes
    # and vp_ctx_create finds no device (seen on the GPU box with `python __graft_entry__.py smoke`, which builds -- and loads -- first).
    # The harness always runs beside torch, so torch goes first here.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    fp = ctypes.POINTER(Frame)
    wp = ctypes.POINTER(Window)
    sig = {
        "vp_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "vp_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
        "vp_ctx_destroy": (ctypes.c_int, [_vp]),
        "vp_ctx_set_stream": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
        "vp_ctx_sync": (ctypes.c_int, [_vp]),
        "vp_last_error": (ctypes.c_char_p, []),
        "vp_abi_version": (ctypes.c_int, []),
        "vp_malloc": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(_vp)]),
        "vp_free": (ctypes.c_int, [_vp, _vp]),
        "vp_memset": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _sz]),
        "vp_memcpy_d2d": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
        "vp_stream_copy": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
        "vp_ctx_workspace": (ctypes.c_int, [_vp, ctypes.c_int, _sz, ctypes.POINTER(_vp)]),
        "vp_ctx_release": (ctypes.c_int, [_vp]),
        "vp_upload": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
        "vp_download": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
        "vp_grid_words": (_sz, [fp]),
        "vp_grid_voxels": (_sz, [fp]),
        "vp_voxelize": (ctypes.c_int, [_vp, fp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int, ctypes.c_int]),
        "vp_voxelize_conservative": (ctypes.c_int, [_vp, fp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int, ctypes.c_int]),
        "vp_voxelize_conservative_host": (ctypes.c_int, [_vp, fp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int]),
        "vp_fill_interior": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_fill_interior_host": (ctypes.c_int, [_vp, fp, _vp, _vp]),
        "vp_morph": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]),
        "vp_morph_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]),
        "vp_components_label": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_components_sizes": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint32, _vp]),
        "vp_components_filter": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_components_label_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_components_filter_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                                     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_surfnets_count": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_surfnets": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, ctypes.c_uint32, _vp, _vp, _vp, _sz, _sz]),
        "vp_surfnets_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _sz, _sz,
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_isonets": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, ctypes.c_float, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_isonets_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_isonets_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, ctypes.c_float, ctypes.c_uint32, ctypes.c_int, _vp, _vp, _vp, _vp, _sz, _sz,
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_edt": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, _vp, ctypes.c_int]),
        "vp_edt_sdf": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_float, _vp, ctypes.c_int]),
        "vp_edt_morph": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]),
        "vp_edt_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, _vp, ctypes.c_int]),
        "vp_edt_sdf_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_float, _vp, ctypes.c_int]),
        "vp_edt_morph_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]),
        "vp_mesh_distance": (ctypes.c_int, [_vp, fp, _vp, _sz, _vp, _sz, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_int]),
        "vp_mesh_distance_host": (ctypes.c_int, [_vp, fp, _vp, _sz, _vp, _sz, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_int]),
        "vp_mesh_distance_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
        "vp_winding": (ctypes.c_int, [_vp, fp, _vp, _sz, _vp, _sz, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
        "vp_winding_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint32)]),
        "vp_winding_host": (ctypes.c_int, [_vp, fp, _vp, _sz, _vp, _sz, ctypes.c_float, ctypes.c_float, ctypes.c_int, _vp, _vp,
                                           ctypes.POINTER(ctypes.c_uint64)]),
        "vp_thickness": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
        "vp_thickness_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint32)]),
        "vp_thickness_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, _vp, _vp, ctypes.POINTER(ctypes.c_uint64)]),
        "vp_octree": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
        "vp_octree_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint64), _vp, _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_octree_expand": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint64, ctypes.c_int]),
        "vp_octree_expand_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint32)]),
        "vp_octree_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, _vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), _vp, _vp]),
        "vp_octree_expand_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint64, ctypes.c_int, _vp]),
        "vp_octree_validate_host": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32]),
        "vp_skeleton": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, _vp]),
        "vp_skeleton_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_skeleton_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, _vp, _vp]),
        "vp_skeleton_table_host": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
        "vp_geodesic": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
        "vp_geodesic_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_geodesic_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
        "vp_reconstruct": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
        "vp_reconstruct_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_reconstruct_host": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
        "vp_extrema": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, _vp]),
        "vp_extrema_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_extrema_host": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp]),
        "vp_watershed": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, _vp]),
        "vp_watershed_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_watershed_host": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
        "vp_regions": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, _vp]),
        "vp_regions_result": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint32), _vp, ctypes.POINTER(ctypes.c_uint32)]),
        "vp_regions_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, _vp, _vp]),
        "vp_csg": (ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_int]),
        "vp_jfa_workspace_bytes": (_sz, [fp]),
        "vp_jfa_id_bytes": (_sz, [fp]),
        "vp_jfa_state_bytes": (_sz, [fp, ctypes.c_int]),
        "vp_jfa_last_shapes": (ctypes.c_int, [_vp, ctypes.POINTER(JfaShape), ctypes.c_int]),
        "vp_jfa": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_float, _vp, _vp, _sz, ctypes.c_int]),
        "vp_jfa_start": (ctypes.c_int, [_vp, fp, _vp, _vp, _sz, ctypes.c_int]),
        "vp_jfa_run": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_float, _vp, _vp, _sz, ctypes.c_int]),
        "vp_jfa_init": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, _vp]),
        "vp_jfa_pass": (ctypes.c_int, [_vp, fp, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_int]),
        "vp_jfa_finalize": (ctypes.c_int, [_vp, fp, _vp, _vp, ctypes.c_float, _vp]),
        "vp_jfa_last_pass": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, ctypes.c_int]),
        "vp_jfa_can_start_from_mask": (ctypes.c_int, [fp, ctypes.c_int]),
        "vp_jfa_can_fuse_first_two": (ctypes.c_int, [fp, ctypes.c_int]),
        "vp_jfa_window_bytes": (_sz, [fp, ctypes.c_uint32]),
        "vp_jfa_window_span": (ctypes.c_int, [fp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
        "vp_jfa_window_clear": (ctypes.c_int, [_vp, fp, wp]),
        "vp_jfa_window_init": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, wp]),
        "vp_jfa_window_first_pass": (ctypes.c_int, [_vp, fp, _vp, wp]),
        "vp_jfa_window_first_two": (ctypes.c_int, [_vp, fp, _vp, wp]),
        "vp_jfa_window_pass": (ctypes.c_int, [_vp, fp, ctypes.c_uint32, wp, wp, ctypes.c_uint32]),
        "vp_jfa_window_last_pass": (ctypes.c_int, [_vp, fp, wp, wp, ctypes.c_uint32, _vp, ctypes.c_float, _vp]),
        "vp_jfa_cyclic_passes": (ctypes.c_int, [fp, ctypes.c_uint32]),
        "vp_jfa_window_first_two_cyclic": (ctypes.c_int, [_vp, fp, _vp, wp, ctypes.c_uint32, ctypes.c_uint32]),
        "vp_jfa_window_pass_cyclic": (ctypes.c_int, [_vp, fp, ctypes.c_uint32, wp, wp, ctypes.c_uint32, ctypes.c_uint32]),
        "vp_jfa_window_interleave": (ctypes.c_int, [_vp, fp, wp, wp, ctypes.c_uint32, ctypes.c_uint32]),
        "vp_surface": (ctypes.c_int, [_vp, fp, _vp, _vp, _vp, _vp]),
        "vp_extract_count": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
        "vp_extract": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_int, _vp, _vp, _vp, _sz]),
        "vp_voxelize_host": (ctypes.c_int, [_vp, fp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int]),
        "vp_csg_host": (ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_int]),
        "vp_jfa_host": (ctypes.c_int, [_vp, fp, _vp, ctypes.c_float, _vp, ctypes.c_int]),
        "vp_prof_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
        "vp_prof_select": (ctypes.c_int, [_vp, ctypes.c_uint64]),
        "vp_prof_reset": (ctypes.c_int, [_vp]),
        "vp_prof_get": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
        "vp_prof_name": (ctypes.c_char_p, [ctypes.c_int]),
        "vp_multi_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_vp)]),
        "vp_multi_destroy": (ctypes.c_int, [_vp]),
        "vp_multi_count": (ctypes.c_int, [_vp]),
        "vp_multi_ctx": (_vp, [_vp, ctypes.c_int]),
        "vp_multi_sync": (ctypes.c_int, [_vp]),
        "vp_multi_set_mesh": (ctypes.c_int, [_vp, _vp, _sz, _vp, _sz]),
        "vp_multi_voxelize": (ctypes.c_int, [_vp, fp, ctypes.c_int]),
        "vp_multi_set_grid": (ctypes.c_int, [_vp, fp, _vp]),
        "vp_multi_get_grid": (ctypes.c_int, [_vp, _vp]),
        "vp_multi_csg": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int]),
        "vp_multi_jfa": (ctypes.c_int, [_vp, ctypes.c_float, ctypes.c_int, ctypes.c_int]),
        "vp_multi_get_sdf": (ctypes.c_int, [_vp, _vp]),
        "vp_multi_bytes_moved": (ctypes.c_uint64, [_vp]),
        "vp_multi_window": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise VPError(rc, (lib().vp_last_error() or b"").decode("utf-8", "replace"))


def skeleton_table(algo: int = ALGO_TILED, _ctx=None):
    """uint32[2^21]: bit c = simple(m) for the neighbourhood m = (c & 0x1FFF) | (c >> 13) << 14 (include/vphip.h, vp_skeleton), computed on the
    CPU -- ALGO_NAIVE by the plain form of the test, ALGO_TILED by the shift form.  No GPU needed."""
    np = __import__("numpy")
    t = np.empty(1 << 21, np.uint32)
    check(lib().vp_skeleton_table_host(_ctx, algo, t.ctypes.data_as(_vp)))
    return t


REGION_DTYPE = [("label", "<u4"), ("voxels", "<u8"), ("volume", "<f8"), ("centroid", "<f8", 3), ("box_min", "<f8", 3), ("box_max", "<f8", 3),
                ("covariance", "<f8", (3, 3)), ("eigenvalues", "<f8", 3), ("radii", "<f8", 3), ("surface", "<f8"), ("contact_area", "<f8"),
                ("sphericity", "<f8"), ("euler", "<i8"), ("value_mean", "<f8"), ("value_min", "<f8"), ("value_max", "<f8"), ("first", "<u4", 3)]


def region_table(raw, frame: Frame):
    """The derived quantities of a vp_regions table (uint64, K x 26) in float64, a numpy structured array of K rows (REGION_DTYPE), in the
    world units of `frame`: the volume V vs^3; the centroid (sum / V + 0.5) vs + origin; the bounding box (the low corner of the lowest
    voxel, the high corner of the highest); the covariance matrix of the voxel centres plus 1/12 per axis for the voxel's own extent, times
    vs^2; its eigenvalues in ascending order and the radii sqrt(5 lambda) of the ellipsoid with the same moments; the surface estimate
    S = (2 / 3) F vs^2 from the exposed faces F of the three axis directions (Crofton: anisotropic, a few per cent on round shapes -- DESIGN.md
    section 23); the contact area (contact faces x vs^2); the sphericity pi^(1/3) (6 volume)^(2/3) / S; the Euler number
    n0 - n1 + (6 V + F) / 2 - V of the closed-cube complex (26-connected); mean / min / max of the value field; the first voxel (x, y, z).
    An empty label (V = 0) reads zero everywhere.  These floats are NOT part of the byte contract: only the uint64 table is."""
    np = __import__("numpy")
    t = np.ascontiguousarray(raw).view(np.uint64).reshape(-1, REGION_WORDS).astype(np.int64)
    out = np.zeros(t.shape[0], REGION_DTYPE)
    n, vs = int(frame.n), float(frame.voxel_size)
    origin = np.array([frame.origin[0], frame.origin[1], frame.origin[2]], np.float64)
    v = t[:, 0]
    some = v > 0
    d = np.maximum(v, 1).astype(np.float64)
    out["label"] = np.arange(1, t.shape[0] + 1)
    out["voxels"] = v
    out["volume"] = v * vs ** 3
    out["centroid"] = np.where(some[:, None], (t[:, 7:10] / d[:, None] + 0.5) * vs + origin, 0.0)
    out["box_min"] = np.where(some[:, None], t[:, 1:4] * vs + origin, 0.0)
    out["box_max"] = np.where(some[:, None], (t[:, 4:7] + 1) * vs + origin, 0.0)
    # second moments about an integer point near the middle of the box first, in exact int64 arithmetic (every term < 2^53): what is left for
    # float64 is small numbers, so the subtraction of the squared mean loses nothing that matters
    c = (t[:, 1:4] + t[:, 4:7]) // 2
    s1 = t[:, 7:10] - c * v[:, None]
    cov = np.zeros((t.shape[0], 3, 3), np.float64)
    for a, b, word in ((0, 0, 10), (1, 1, 11), (2, 2, 12), (0, 1, 13), (0, 2, 14), (1, 2, 15)):
        s2 = t[:, word] - c[:, a] * t[:, 7 + b] - c[:, b] * t[:, 7 + a] + c[:, a] * c[:, b] * v
        cov[:, a, b] = cov[:, b, a] = s2 / d - (s1[:, a] / d) * (s1[:, b] / d) + (1.0 / 12.0 if a == b else 0.0)
    cov[~some] = 0.0
    out["covariance"] = cov * vs * vs
    out["eigenvalues"] = np.linalg.eigvalsh(out["covariance"]) if t.shape[0] else 0.0
    out["radii"] = np.sqrt(5.0 * np.maximum(out["eigenvalues"], 0.0))
    faces = t[:, 16] + t[:, 17] + t[:, 18]
    out["surface"] = (2.0 / 3.0) * faces * vs * vs
    out["contact_area"] = t[:, 19] * vs * vs
    out["sphericity"] = np.where(some, np.pi ** (1.0 / 3.0) * (6.0 * out["volume"]) ** (2.0 / 3.0) / np.maximum(out["surface"], 1e-300), 0.0)
    out["euler"] = t[:, 20] - t[:, 21] + (6 * v + faces) // 2 - v
    u = np.ascontiguousarray(raw).view(np.uint64).reshape(-1, REGION_WORDS)
    out["value_mean"] = np.where(some, u[:, 22].astype(np.float64) / d, 0.0)
    out["value_min"] = u[:, 23]
    out["value_max"] = u[:, 24]
    out["first"] = np.stack([t[:, 25] % n, (t[:, 25] // n) % n, t[:, 25] // (n * n)], 1)
    return out


class Context:
    """vp_ctx wrapper.  Device pointers are plain ints (e.g. torch.Tensor.data_ptr())."""

    def __init__(self, device: int = 0):
        self._h = _vp()
        check(lib().vp_ctx_create(device, ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            lib().vp_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing
    def set_stream(self, hip_stream, external: bool = True):
        """external=True: run on the caller's stream handle (0 = the null stream = torch's default stream)."""
        check(lib().vp_ctx_set_stream(self._h, _vp(hip_stream) if hip_stream else None, 1 if external else 0))

    def sync(self):
        check(lib().vp_ctx_sync(self._h))

    def malloc(self, nbytes: int) -> int:
        p = _vp()
        check(lib().vp_malloc(self._h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, ptr: int):
        check(lib().vp_free(self._h, _vp(ptr)))

    def memset(self, ptr: int, value: int, nbytes: int):
        check(lib().vp_memset(self._h, _vp(ptr), value, nbytes))

    def upload(self, dptr: int, host_array):
        check(lib().vp_upload(self._h, _vp(dptr), host_array.ctypes.data_as(_vp), host_array.nbytes))

    def download(self, host_array, dptr: int):
        check(lib().vp_download(self._h, host_array.ctypes.data_as(_vp), _vp(dptr), host_array.nbytes))

    # -- device-resident stages
    def voxelize(self, frame: Frame, d_words: int, d_xyz: int, nverts: int, d_tri: int, ntris: int,
                 algo: int = ALGO_TILED, accumulate: bool = False):
        check(lib().vp_voxelize(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_xyz), nverts, _vp(d_tri), ntris,
                                algo, 1 if accumulate else 0))

    def voxelize_conservative(self, frame: Frame, d_words: int, d_xyz: int, nverts: int, d_tri: int, ntris: int,
                              algo: int = ALGO_TILED, accumulate: bool = False):
        """Conservative surface voxelization (closed voxel box overlaps closed triangle); accumulate ORs into d_words."""
        check(lib().vp_voxelize_conservative(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_xyz), nverts, _vp(d_tri), ntris,
                                             algo, 1 if accumulate else 0))

    def fill_interior(self, frame: Frame, d_words: int, d_out: int) -> int:
        """Interior fill (6-connected exterior flood from the grid boundary): d_out = d_words plus every enclosed empty voxel.
        Blocking; returns the number of propagation rounds that ran."""
        rounds = ctypes.c_uint32(0)
        check(lib().vp_fill_interior(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_out), ctypes.byref(rounds)))
        return rounds.value

    def morph(self, frame: Frame, d_words: int, d_out: int, op: int, radius: int, algo: int = ALGO_TILED):
        """Ball morphology (MORPH_DILATE / ERODE / OPEN / CLOSE, integer radius 0 .. 32): d_out = op(d_words).  Enqueues only."""
        check(lib().vp_morph(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_out), op, radius, algo))

    def edt(self, frame: Frame, d_words: int, d_dist2: int, seeds: int = EDT_SEEDS_SET, algo: int = ALGO_TILED):
        """Exact squared voxel distance to the nearest seed (EDT_SEEDS_SET / UNSET / BORDER): d_dist2 takes one uint32 per voxel, x fastest;
        EDT_NONE everywhere if the grid has no seed.  Enqueues only."""
        check(lib().vp_edt(self._h, ctypes.byref(frame), _vp(d_words), seeds, _vp(d_dist2), algo))

    def edt_sdf(self, frame: Frame, d_words: int, fill: float, d_sdf: int, algo: int = ALGO_TILED):
        """The exact counterpart of jfa(): signed squared distance to the border voxels, +inside, -outside.  Enqueues only."""
        check(lib().vp_edt_sdf(self._h, ctypes.byref(frame), _vp(d_words), fill, _vp(d_sdf), algo))

    def edt_morph(self, frame: Frame, d_words: int, d_out: int, op: int, radius: int, algo: int = ALGO_TILED):
        """morph() through the distance transform: any integer radius 0 .. 65535.  Enqueues only."""
        check(lib().vp_edt_morph(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_out), op, radius, algo))

    def mesh_distance(self, frame: Frame, d_xyz: int, nverts: int, d_tri: int, ntris: int, band: int, d_dist2: int, d_nearest: int = 0,
                      d_sign_words: int = 0, algo: int = ALGO_TILED):
        """Narrow-band squared distance from every voxel centre to the triangles of the mesh, band = 1 .. 32 voxels: d_dist2 takes one
        float32 per voxel (min(B2, .), signed by d_sign_words if given: + on set voxels, - on unset ones), d_nearest (optional) the index
        of the nearest face or MESH_NONE.  ALGO_TILED reads the list lengths back once (blocking); ALGO_NAIVE enqueues only."""
        check(lib().vp_mesh_distance(self._h, ctypes.byref(frame), _vp(d_xyz), nverts, _vp(d_tri), ntris, _vp(d_sign_words) if d_sign_words else None,
                                     band, _vp(d_dist2), _vp(d_nearest) if d_nearest else None, algo))

    def mesh_distance_list_entries(self) -> int:
        """(triangle, brick) pairs the last ALGO_TILED mesh_distance of this context listed."""
        n = ctypes.c_uint64()
        check(lib().vp_mesh_distance_stats(self._h, ctypes.byref(n)))
        return int(n.value)

    def components_label(self, frame: Frame, d_words: int, d_labels: int, conn: int = CONN_26, algo: int = ALGO_TILED) -> int:
        """Connected components of the set voxels (CONN_6 / CONN_26): d_labels takes one uint32 per voxel, 0 = background, components
        1 .. K in the order of their lowest voxel index (= scipy.ndimage.label).  Blocking; returns K."""
        count = ctypes.c_uint32()
        check(lib().vp_components_label(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_labels), conn, algo, ctypes.byref(count)))
        return count.value

    def components_sizes(self, frame: Frame, d_labels: int, count: int, d_sizes: int):
        """d_sizes[k - 1] = voxels of component k of a label volume with `count` components.  Blocking."""
        check(lib().vp_components_sizes(self._h, ctypes.byref(frame), _vp(d_labels), count, _vp(d_sizes or None)))

    def components_filter(self, frame: Frame, d_words: int, d_out: int, mode: int, param: int, conn: int = CONN_26, algo: int = ALGO_TILED):
        """d_out = the components of d_words that pass COMP_KEEP_LARGEST (param = m largest, 1 .. 16) or COMP_MIN_VOXELS (param = least
        size).  Blocking; returns (K, kept voxels)."""
        count, kept = ctypes.c_uint32(), ctypes.c_uint64()
        check(lib().vp_components_filter(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_out), conn, mode, param, algo,
                                         ctypes.byref(count), ctypes.byref(kept)))
        return count.value, kept.value

    def csg(self, d_a: int, d_b: int, nwords: int, op: int):
        check(lib().vp_csg(self._h, _vp(d_a), _vp(d_b), nwords, op))

    def jfa_workspace_bytes(self, frame: Frame) -> int:
        return int(lib().vp_jfa_workspace_bytes(ctypes.byref(frame)))

    def jfa_id_bytes(self, frame: Frame) -> int:
        """Bytes of a PLAIN id (the caller-addressed planes of vp_jfa_init / vp_jfa_pass): 4 for n <= 1024, 8 for n <= 2048."""
        return int(lib().vp_jfa_id_bytes(ctypes.byref(frame)))

    def jfa_state_bytes(self, frame: Frame, algo: int = ALGO_TILED) -> int:
        """Bytes of id state per voxel vp_jfa streams per pass (whole grid): 4, 5 (windows above n = 1024) or 8 (VP_ALGO_NAIVE there)."""
        return int(lib().vp_jfa_state_bytes(ctypes.byref(frame), algo))

    def jfa_last_shapes(self):
        """The tile kernels the most recent pass call of this context launched, in launch order: one dict per launch with the fields of
        vp_jfa_shape (empty after a call that was refused or served by another kernel).  Measurement and tests only."""
        buf = (JfaShape * 4)()
        count = int(lib().vp_jfa_last_shapes(self._h, buf, 4))
        return [{name: int(getattr(buf[i], name)) for name, _ in JfaShape._fields_} for i in range(min(count, 4))]

    def jfa(self, frame: Frame, d_words: int, fill: float, d_sdf: int, d_work=None, work_bytes: int = 0,
            algo: int = ALGO_TILED):
        """d_work = None: the context's own grow-only workspace."""
        check(lib().vp_jfa(self._h, ctypes.byref(frame), _vp(d_words), fill, _vp(d_sdf), _vp(d_work or None), work_bytes, algo))

    def jfa_start(self, frame: Frame, d_words: int, d_work=None, work_bytes: int = 0, algo: int = ALGO_TILED):
        check(lib().vp_jfa_start(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_work or None), work_bytes, algo))

    def jfa_run(self, frame: Frame, d_words: int, fill: float, d_sdf: int, d_work=None, work_bytes: int = 0, algo: int = ALGO_TILED):
        check(lib().vp_jfa_run(self._h, ctypes.byref(frame), _vp(d_words), fill, _vp(d_sdf), _vp(d_work or None), work_bytes, algo))

    def memcpy_d2d(self, dst: int, src: int, nbytes: int):
        check(lib().vp_memcpy_d2d(self._h, _vp(dst), _vp(src), nbytes))

    def stream_copy(self, dst: int, src: int, nbytes: int):
        """the 16-bytes-per-lane copy kernel bench.py measures the box's HBM copy rate with"""
        check(lib().vp_stream_copy(self._h, _vp(dst), _vp(src), nbytes))

    def workspace(self, slot: int, nbytes: int) -> int:
        p = _vp()
        check(lib().vp_ctx_workspace(self._h, slot, nbytes, ctypes.byref(p)))
        return p.value

    def release(self):
        check(lib().vp_ctx_release(self._h))

    def jfa_init(self, frame: Frame, d_words: int, d_below, d_above, d_ids: int):
        check(lib().vp_jfa_init(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_below or None),
                                _vp(d_above or None), _vp(d_ids)))

    def jfa_pass(self, frame: Frame, k: int, d_in: int, d_minus, d_plus, d_out: int, algo: int = ALGO_TILED):
        check(lib().vp_jfa_pass(self._h, ctypes.byref(frame), k, _vp(d_in), _vp(d_minus or None),
                                _vp(d_plus or None), _vp(d_out), algo))

    def jfa_finalize(self, frame: Frame, d_words: int, d_ids: int, fill: float, d_sdf: int):
        check(lib().vp_jfa_finalize(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_ids), fill, _vp(d_sdf)))

    def jfa_last_pass(self, frame: Frame, d_in: int, d_minus, d_plus, d_scratch: int, d_words: int, fill: float, d_sdf: int,
                      algo: int = ALGO_TILED):
        check(lib().vp_jfa_last_pass(self._h, ctypes.byref(frame), _vp(d_in), _vp(d_minus or None), _vp(d_plus or None),
                                     _vp(d_scratch), _vp(d_words), fill, _vp(d_sdf), algo))

    def jfa_can_start_from_mask(self, frame: Frame, algo: int = ALGO_TILED) -> bool:
        return bool(lib().vp_jfa_can_start_from_mask(ctypes.byref(frame), algo))

    def jfa_can_fuse_first_two(self, frame: Frame, algo: int = ALGO_TILED) -> bool:
        return bool(lib().vp_jfa_can_fuse_first_two(ctypes.byref(frame), algo))

    # -- id windows (vp_jfa_window_*): the slab form of the tile kernels; the layout inside a window is the library's
    def jfa_window_bytes(self, frame: Frame, planes: int) -> int:
        return int(lib().vp_jfa_window_bytes(ctypes.byref(frame), planes))

    def jfa_window_span(self, frame: Frame, planes: int, p0: int, p1: int):
        """[(byte offset, bytes), ...]: where the planes [p0, p1) of a window of `planes` planes live (one range, two above n = 1024)"""
        off, nb = (_sz * 2)(), (_sz * 2)()
        check(lib().vp_jfa_window_span(ctypes.byref(frame), planes, p0, p1, off, nb))
        return [(int(off[i]), int(nb[i])) for i in range(2) if nb[i]]

    def jfa_window_clear(self, frame: Frame, win: Window):
        check(lib().vp_jfa_window_clear(self._h, ctypes.byref(frame), ctypes.byref(win)))

    def jfa_window_init(self, frame: Frame, d_words: int, d_below, d_above, win: Window):
        check(lib().vp_jfa_window_init(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_below or None), _vp(d_above or None), ctypes.byref(win)))

    def jfa_window_first_pass(self, frame: Frame, d_border_grid: int, win: Window):
        check(lib().vp_jfa_window_first_pass(self._h, ctypes.byref(frame), _vp(d_border_grid), ctypes.byref(win)))

    def jfa_window_first_two(self, frame: Frame, d_border_grid: int, win: Window):
        """passes n/2 and n/4 of a whole grid in one launch from its border mask"""
        check(lib().vp_jfa_window_first_two(self._h, ctypes.byref(frame), _vp(d_border_grid), ctypes.byref(win)))

    def jfa_window_pass(self, frame: Frame, k: int, win_in: Window, win_out: Window, stride=None):
        check(lib().vp_jfa_window_pass(self._h, ctypes.byref(frame), k, ctypes.byref(win_in), ctypes.byref(win_out), k if stride is None else stride))

    def jfa_window_last_pass(self, frame: Frame, win_in: Window, win_scratch: Window, d_words_region: int, fill: float, d_sdf_region: int, stride: int = 1):
        check(lib().vp_jfa_window_last_pass(self._h, ctypes.byref(frame), ctypes.byref(win_in), ctypes.byref(win_scratch), stride,
                                            _vp(d_words_region), fill, _vp(d_sdf_region)))

    # -- cyclic plane distribution (the first phase of the transposed multi-GPU pipeline)
    @staticmethod
    def jfa_cyclic_passes(frame: Frame, ranks: int) -> int:
        """passes of the sequence n/2, n/4, ... whose step is a multiple of `ranks`, counted from the first (0: the grid cannot be dealt cyclically)"""
        return int(lib().vp_jfa_cyclic_passes(ctypes.byref(frame), ranks))

    def jfa_window_first_two_cyclic(self, frame: Frame, d_border_grid: int, win: Window, ranks: int, rank: int):
        check(lib().vp_jfa_window_first_two_cyclic(self._h, ctypes.byref(frame), _vp(d_border_grid), ctypes.byref(win), ranks, rank))

    def jfa_window_pass_cyclic(self, frame: Frame, k: int, win_in: Window, win_out: Window, ranks: int, rank: int):
        check(lib().vp_jfa_window_pass_cyclic(self._h, ctypes.byref(frame), k, ctypes.byref(win_in), ctypes.byref(win_out), ranks, rank))

    def jfa_window_interleave(self, frame: Frame, win_in: Window, win_out: Window, ranks: int, count: int):
        check(lib().vp_jfa_window_interleave(self._h, ctypes.byref(frame), ctypes.byref(win_in), ctypes.byref(win_out), ranks, count))

    def surface(self, frame: Frame, d_words: int, d_below, d_above, d_border: int):
        check(lib().vp_surface(self._h, ctypes.byref(frame), _vp(d_words), _vp(d_below or None),
                               _vp(d_above or None), _vp(d_border)))

    def extract_count(self, frame: Frame, d_words: int, mode: int) -> int:
        n = ctypes.c_uint64()
        check(lib().vp_extract_count(self._h, ctypes.byref(frame), _vp(d_words), mode, ctypes.byref(n)))
        return int(n.value)

    def extract(self, frame: Frame, d_words: int, mode: int, d_sdf, d_records: int, d_values, capacity: int):
        check(lib().vp_extract(self._h, ctypes.byref(frame), _vp(d_words), mode, _vp(d_sdf or None), _vp(d_records),
                               _vp(d_values or None), capacity))

    def surfnets_count(self, frame: Frame, d_words: int, algo: int = ALGO_TILED):
        """Vertices and quads of the surface-nets mesh of a whole grid: (V, Q).  Blocking."""
        nv, nq = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().vp_surfnets_count(self._h, ctypes.byref(frame), _vp(d_words), algo, ctypes.byref(nv), ctypes.byref(nq)))
        return int(nv.value), int(nq.value)

    def surfnets(self, frame: Frame, d_words: int, algo: int, iterations: int, d_cells: int, d_xyz: int, d_quads: int,
                 vertex_capacity: int, quad_capacity: int):
        """After surfnets_count of the same grid and algo: V records (uint64), V x 3 float32 lattice positions after `iterations` (0 .. 64)
        relaxation steps and Q x 4 uint32 vertex indices.  Enqueues only."""
        check(lib().vp_surfnets(self._h, ctypes.byref(frame), _vp(d_words), algo, iterations, _vp(d_cells or None), _vp(d_xyz or None),
                                _vp(d_quads or None), vertex_capacity, quad_capacity))

    def isonets(self, frame: Frame, d_field: int, transform: int = ISO_SIGNED_SQUARE, iso: float = 0.0, iterations: int = 0,
                normals: bool = False, algo: int = ALGO_TILED):
        """Surface nets of a float field (n^3 values, x fastest) at level `iso`, built into buffers the context owns: (V, Q).  Blocking;
        drops a pending surfnets_count.  isonets_result() hands the buffers out."""
        nv, nq = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().vp_isonets(self._h, ctypes.byref(frame), _vp(d_field or None), transform, iso, iterations, 1 if normals else 0, algo,
                               ctypes.byref(nv), ctypes.byref(nq)))
        return int(nv.value), int(nq.value)

    def isonets_result(self):
        """(d_cells, d_xyz, d_normals, d_quads, V, Q) of the last isonets(): device pointers as ints, 0 where there is none.  Valid until
        the next isonets(), release() or close()."""
        c, x, m, q = _vp(), _vp(), _vp(), _vp()
        nv, nq = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().vp_isonets_result(self._h, ctypes.byref(c), ctypes.byref(x), ctypes.byref(m), ctypes.byref(q), ctypes.byref(nv),
                                      ctypes.byref(nq)))
        return c.value or 0, x.value or 0, m.value or 0, q.value or 0, int(nv.value), int(nq.value)

    def winding(self, frame: Frame, d_xyz: int, nverts: int, d_tri: int, ntris: int, beta: float = 2.0, level: float = 0.5,
                algo: int = ALGO_TILED, count: bool = False):
        """Generalized winding number of the mesh at the voxel centres and its inside grid (w >= level), built into buffers the context
        owns; winding_result() hands them out.  beta = 0: brute force; 1 .. 64: the far-field opening parameter.  Enqueues only, unless
        count=True: then it blocks and returns the number of inside voxels."""
        c = ctypes.c_uint64()
        check(lib().vp_winding(self._h, ctypes.byref(frame), _vp(d_xyz or None), nverts, _vp(d_tri or None), ntris, beta, level, algo,
                               ctypes.byref(c) if count else None))
        return int(c.value) if count else None

    def winding_result(self):
        """(d_w, d_inside, n) of the last winding(): device pointers as ints (0 where there is none) and the side they are for.  Valid until
        the next winding(), release() or close()."""
        w, g, n = _vp(), _vp(), ctypes.c_uint32()
        check(lib().vp_winding_result(self._h, ctypes.byref(w), ctypes.byref(g), ctypes.byref(n)))
        return w.value or 0, g.value or 0, int(n.value)

    def thickness(self, frame: Frame, d_words: int, rmax: int, thin2: int = 0, algo: int = ALGO_TILED, count: bool = False):
        """Local thickness of a whole grid in a band of rmax = 1 .. 32 voxels -- T2, the squared radius of the largest inscribed ball through
        every set voxel -- and the grid of the set voxels with T2 < thin2, built into buffers the context owns; thickness_result() hands
        them out.  Enqueues only, unless count=True: then it blocks and returns the number of thin voxels."""
        c = ctypes.c_uint64()
        check(lib().vp_thickness(self._h, ctypes.byref(frame), _vp(d_words or None), rmax, thin2, algo, ctypes.byref(c) if count else None))
        return int(c.value) if count else None

    def thickness_result(self):
        """(d_t2, d_thin, n) of the last thickness(): device pointers as ints (0 where there is none) and the side they are for.  Valid
        until the next thickness(), release() or close()."""
        t, g, n = _vp(), _vp(), ctypes.c_uint32()
        check(lib().vp_thickness_result(self._h, ctypes.byref(t), ctypes.byref(g), ctypes.byref(n)))
        return t.value or 0, g.value or 0, int(n.value)

    def octree(self, frame: Frame, d_words: int, algo: int = ALGO_TILED) -> int:
        """Sparse voxel octree of a whole grid (n <= 1024) into buffers the context owns; octree_result() hands them out.  Blocks once (the
        node count is read back) and returns it."""
        m = ctypes.c_uint64()
        check(lib().vp_octree(self._h, ctypes.byref(frame), _vp(d_words or None), algo, ctypes.byref(m)))
        return int(m.value)

    def octree_result(self):
        """(d_nodes, M, level_offset, full_leaves, n) of the last octree(): the device pointer as an int (0 where there is none), the node
        count, two lists of 11 and the side they are for.  Valid until the next octree(), release() or close()."""
        d, m, n = _vp(), ctypes.c_uint64(), ctypes.c_uint32()
        lo, fl = (ctypes.c_uint32 * 11)(), (ctypes.c_uint32 * 11)()
        check(lib().vp_octree_result(self._h, ctypes.byref(d), ctypes.byref(m), lo, fl, ctypes.byref(n)))
        return d.value or 0, int(m.value), list(lo), list(fl), int(n.value)

    def octree_expand(self, frame: Frame, d_nodes: int, nodes: int, algo: int = ALGO_TILED):
        """A tree of `nodes` records back into the bit grid of the frame, a grid the context owns; octree_expand_result() hands it out.
        Enqueues only, once the grid has grown."""
        check(lib().vp_octree_expand(self._h, ctypes.byref(frame), _vp(d_nodes or None), nodes, algo))

    def octree_expand_result(self):
        """(d_words, n) of the last octree_expand(): the device pointer as an int (0 where there is none) and the side it is for"""
        d, n = _vp(), ctypes.c_uint32()
        check(lib().vp_octree_expand_result(self._h, ctypes.byref(d), ctypes.byref(n)))
        return d.value or 0, int(n.value)

    def skeleton(self, frame: Frame, d_words: int, mode: int = SKEL_CURVE, max_iters: int = 0, d_anchor: int = 0, algo: int = ALGO_TILED):
        """Topological thinning of a whole grid (n <= 1024) into a grid the context owns; skeleton_result() hands it out.  Blocks (the
        deleted count of every iteration is read back) and returns (voxels left, iterations, voxels deleted)."""
        s = (ctypes.c_uint64 * 3)()
        check(lib().vp_skeleton(self._h, ctypes.byref(frame), _vp(d_words or None), _vp(d_anchor or None), mode, max_iters, algo, s))
        return tuple(int(v) for v in s)

    def skeleton_result(self):
        """(d_skel, stats, n) of the last skeleton(): the device pointer as an int (0 where there is none), (voxels left, iterations, voxels
        deleted) and the side they are for.  Valid until the next skeleton(), release() or close()."""
        d, s, n = _vp(), (ctypes.c_uint64 * 3)(), ctypes.c_uint32()
        check(lib().vp_skeleton_result(self._h, ctypes.byref(d), s, ctypes.byref(n)))
        return d.value or 0, tuple(int(v) for v in s), int(n.value)

    def geodesic(self, frame: Frame, d_mask: int, d_seeds: int, metric: int = GEO_CHAMFER, algo: int = ALGO_TILED):
        """Geodesic distance inside the mask from the seed voxels of a whole grid (n <= 1024) into buffers the context owns;
        geodesic_result() hands them out.  Blocks (convergence is read back) and returns (seeds used, voxels reached, largest finite
        distance, lowest linear index that attains it)."""
        s = (ctypes.c_uint64 * 4)()
        check(lib().vp_geodesic(self._h, ctypes.byref(frame), _vp(d_mask or None), _vp(d_seeds or None), metric, algo, s))
        return tuple(int(v) for v in s)

    def geodesic_result(self):
        """(d_dist, d_reach, stats, n) of the last geodesic(): the device pointers as ints (0 where there is none), the four statistics
        and the side they are for.  Valid until the next geodesic(), release() or close()."""
        d, r, s, n = _vp(), _vp(), (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        check(lib().vp_geodesic_result(self._h, ctypes.byref(d), ctypes.byref(r), s, ctypes.byref(n)))
        return d.value or 0, r.value or 0, tuple(int(v) for v in s), int(n.value)

    def watershed(self, frame: Frame, d_mask: int, d_markers: int, d_priority: int = 0, order: int = WS_DESCENDING, quantum: int = 1,
                  connectivity: int = CONN_6, algo: int = ALGO_TILED):
        """Seeded watershed of the mask from the marker volume (uint32 per voxel, 0 = none) over the priority field (uint32 per voxel;
        0: none -- the geodesic influence zones) of a whole grid (n <= 1024) into buffers the context owns; watershed_result() hands them
        out.  Blocks (a pre-pass and the convergence of every level are read back) and returns (markers used, voxels labelled, levels
        present, voxels cut)."""
        s = (ctypes.c_uint64 * 4)()
        check(lib().vp_watershed(self._h, ctypes.byref(frame), _vp(d_mask or None), _vp(d_markers or None), _vp(d_priority or None), order, quantum,
                                 connectivity, algo, s))
        return tuple(int(v) for v in s)

    def watershed_result(self):
        """(d_labels, d_cut, stats, n) of the last watershed(): the device pointers as ints (0 where there is none), the four statistics
        and the side they are for.  Valid until the next watershed(), release() or close()."""
        d, r, s, n = _vp(), _vp(), (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        check(lib().vp_watershed_result(self._h, ctypes.byref(d), ctypes.byref(r), s, ctypes.byref(n)))
        return d.value or 0, r.value or 0, tuple(int(v) for v in s), int(n.value)

    def reconstruct(self, frame: Frame, d_marker: int, d_mask: int, d_domain: int = 0, mode: int = REC_DILATION, connectivity: int = CONN_6,
                    algo: int = ALGO_TILED):
        """Grayscale reconstruction of the marker field under the mask field (uint32 per voxel) on the domain (a bit grid; 0: every voxel)
        of a whole grid (n <= 1024) into a buffer the context owns; reconstruct_result() hands it out.  Blocks (convergence is read back)
        and returns (domain voxels, voxels that changed, sum of R, largest R -- REC_EROSION: the smallest)."""
        s = (ctypes.c_uint64 * 4)()
        check(lib().vp_reconstruct(self._h, ctypes.byref(frame), _vp(d_domain or None), _vp(d_marker or None), _vp(d_mask or None), mode,
                                   connectivity, algo, s))
        return tuple(int(v) for v in s)

    def reconstruct_result(self):
        """(d_field, stats, n) of the last reconstruct(): the device pointer as an int (0 where there is none), the four statistics and
        the side they are for.  Valid until the next reconstruct(), release() or close()."""
        d, s, n = _vp(), (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        check(lib().vp_reconstruct_result(self._h, ctypes.byref(d), s, ctypes.byref(n)))
        return d.value or 0, tuple(int(v) for v in s), int(n.value)

    def extrema(self, frame: Frame, d_values: int, d_domain: int = 0, kind: int = EXT_MAXIMA, scale: int = EXT_LINEAR, h: int = 0,
                connectivity: int = CONN_6, algo: int = ALGO_TILED):
        """h-maxima / h-minima and the extended extrema of a value field (uint32 per voxel) on the domain (a bit grid; 0: every voxel) of a
        whole grid (n <= 1024) into buffers the context owns; extrema_result() hands them out.  Blocks and returns (domain voxels, extrema
        voxels, largest H -- EXT_MINIMA: the smallest --, voxels with H != V)."""
        s = (ctypes.c_uint64 * 4)()
        check(lib().vp_extrema(self._h, ctypes.byref(frame), _vp(d_domain or None), _vp(d_values or None), kind, scale, h, connectivity, algo, s))
        return tuple(int(v) for v in s)

    def extrema_result(self):
        """(d_scaled, d_flat, d_extrema, stats, n) of the last extrema(): the device pointers as ints (0 where there is none), the four
        statistics and the side they are for.  Valid until the next extrema(), release() or close()."""
        v, f, e, s, n = _vp(), _vp(), _vp(), (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        check(lib().vp_extrema_result(self._h, ctypes.byref(v), ctypes.byref(f), ctypes.byref(e), s, ctypes.byref(n)))
        return v.value or 0, f.value or 0, e.value or 0, tuple(int(x) for x in s), int(n.value)

    def regions(self, frame: Frame, d_labels: int, count: int, d_values: int = 0, algo: int = ALGO_TILED):
        """Region analysis of a label volume (uint32 per voxel; labels 1 .. count, anything above is ignored) of a whole grid (n <= 1024),
        with an optional value field (uint32 per voxel; 0: none), into a table the context owns: count records of REGION_WORDS uint64
        (include/vphip.h, vp_regions); regions_result() hands it out.  Blocks (the totals are read back) and returns (sum of V, labels
        with V > 0, voxels ignored, interfaces)."""
        s = (ctypes.c_uint64 * 4)()
        check(lib().vp_regions(self._h, ctypes.byref(frame), _vp(d_labels or None), count, _vp(d_values or None), algo, s))
        return tuple(int(v) for v in s)

    def regions_result(self):
        """(d_table, count, stats, n) of the last regions(): the device pointer as an int (0 where there is none), the number of records,
        the four statistics and the side they are for.  Valid until the next regions(), release() or close()."""
        d, k, s, n = _vp(), ctypes.c_uint32(), (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        check(lib().vp_regions_result(self._h, ctypes.byref(d), ctypes.byref(k), s, ctypes.byref(n)))
        return d.value or 0, int(k.value), tuple(int(v) for v in s), int(n.value)

    # -- host-in / host-out (numpy arrays), the reference's Compute() convention
    def regions_host(self, frame: Frame, h_labels, count: int, h_values=None, algo: int = ALGO_TILED, want=(True, True)):
        """numpy in, numpy out: (table uint64[count, 26], statistics); want = which of the two are asked for (the other goes in as NULL and
        comes back as None)."""
        np = __import__("numpy")
        t = np.zeros((count, REGION_WORDS), np.uint64) if want[0] else None
        s = (ctypes.c_uint64 * 4)() if want[1] else None
        check(lib().vp_regions_host(self._h, ctypes.byref(frame), h_labels.ctypes.data_as(_vp), count,
                                    None if h_values is None else h_values.ctypes.data_as(_vp), algo,
                                    None if t is None else t.ctypes.data_as(_vp), s))
        return t, None if s is None else tuple(int(v) for v in s)

    def reconstruct_host(self, frame: Frame, h_marker, h_mask, h_domain=None, mode: int = REC_DILATION, connectivity: int = CONN_6,
                         algo: int = ALGO_TILED, want=(True, True)):
        """numpy in, numpy out: (field uint32[n^3], statistics); want = which of the two are asked for (the other goes in as NULL and comes
        back as None)."""
        np = __import__("numpy")
        r = np.empty(frame.voxels, np.uint32) if want[0] else None
        s = (ctypes.c_uint64 * 4)() if want[1] else None
        check(lib().vp_reconstruct_host(self._h, ctypes.byref(frame), None if h_domain is None else h_domain.ctypes.data_as(_vp),
                                        h_marker.ctypes.data_as(_vp), h_mask.ctypes.data_as(_vp), mode, connectivity, algo,
                                        None if r is None else r.ctypes.data_as(_vp), s))
        return r, None if s is None else tuple(int(v) for v in s)

    def extrema_host(self, frame: Frame, h_values, h_domain=None, kind: int = EXT_MAXIMA, scale: int = EXT_LINEAR, h: int = 0,
                     connectivity: int = CONN_6, algo: int = ALGO_TILED, want=(True, True, True, True)):
        """numpy in, numpy out: (scaled uint32[n^3], flat uint32[n^3], extrema words uint32[n^3 / 32], statistics); want = which of the four
        are asked for (the others go in as NULL and come back as None)."""
        np = __import__("numpy")
        v = np.empty(frame.voxels, np.uint32) if want[0] else None
        f = np.empty(frame.voxels, np.uint32) if want[1] else None
        e = np.empty(frame.voxels // 32, np.uint32) if want[2] else None
        s = (ctypes.c_uint64 * 4)() if want[3] else None
        p = lambda a: None if a is None else a.ctypes.data_as(_vp)
        check(lib().vp_extrema_host(self._h, ctypes.byref(frame), p(h_domain), h_values.ctypes.data_as(_vp), kind, scale, h, connectivity, algo,
                                    p(v), p(f), p(e), s))
        return v, f, e, None if s is None else tuple(int(x) for x in s)

    def watershed_host(self, frame: Frame, h_mask, h_markers, h_priority=None, order: int = WS_DESCENDING, quantum: int = 1,
                       connectivity: int = CONN_6, algo: int = ALGO_TILED, want=(True, True, True)):
        """numpy in, numpy out: (labels uint32[n^3], cut words uint32[n^3 / 32], statistics); want = which of the three are asked for (the
        others go in as NULL and come back as None)."""
        np = __import__("numpy")
        w = np.empty(frame.voxels, np.uint32) if want[0] else None
        c = np.empty(frame.voxels // 32, np.uint32) if want[1] else None
        s = (ctypes.c_uint64 * 4)() if want[2] else None
        check(lib().vp_watershed_host(self._h, ctypes.byref(frame), h_mask.ctypes.data_as(_vp), h_markers.ctypes.data_as(_vp),
                                      None if h_priority is None else h_priority.ctypes.data_as(_vp), order, quantum, connectivity, algo,
                                      None if w is None else w.ctypes.data_as(_vp), None if c is None else c.ctypes.data_as(_vp), s))
        return w, c, None if s is None else tuple(int(v) for v in s)

    def geodesic_host(self, frame: Frame, h_mask, h_seeds, metric: int = GEO_CHAMFER, algo: int = ALGO_TILED, want=(True, True, True)):
        """numpy in, numpy out: (dist uint32[n^3], reach words uint32[n^3 / 32], statistics); want = which of the three are asked for (the
        others go in as NULL and come back as None)."""
        np = __import__("numpy")
        d = np.empty(frame.voxels, np.uint32) if want[0] else None
        r = np.empty(frame.voxels // 32, np.uint32) if want[1] else None
        s = (ctypes.c_uint64 * 4)() if want[2] else None
        check(lib().vp_geodesic_host(self._h, ctypes.byref(frame), h_mask.ctypes.data_as(_vp), h_seeds.ctypes.data_as(_vp), metric, algo,
                                     None if d is None else d.ctypes.data_as(_vp), None if r is None else r.ctypes.data_as(_vp), s))
        return d, r, None if s is None else tuple(int(v) for v in s)

    def skeleton_host(self, frame: Frame, h_words, mode: int = SKEL_CURVE, max_iters: int = 0, h_anchor=None, algo: int = ALGO_TILED):
        """numpy in, numpy out: (skeleton words uint32[n^3 / 32], (voxels left, iterations, voxels deleted))."""
        np = __import__("numpy")
        g, s = np.empty(frame.voxels // 32, np.uint32), (ctypes.c_uint64 * 3)()
        check(lib().vp_skeleton_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), None if h_anchor is None else h_anchor.ctypes.data_as(_vp),
                                     mode, max_iters, algo, g.ctypes.data_as(_vp), s))
        return g, tuple(int(v) for v in s)

    def skeleton_table_host(self, algo: int = ALGO_TILED):
        """The table of the simple neighbourhoods computed on the device: uint32[2^21], bit c = simple(c) (skeleton_table() without a
        context computes it on the CPU)."""
        return skeleton_table(algo, self._h)

    def octree_host(self, frame: Frame, h_words, algo: int = ALGO_TILED, capacity=None):
        """numpy in, numpy out: (nodes uint32[M, 2], level_offset uint32[11], full_leaves uint32[11]).  The first call asks for the count
        (capacity 0 is refused with the count stored); `capacity` overrides the second call's room."""
        np = __import__("numpy")
        m = ctypes.c_uint64()
        lo, fl = np.zeros(11, np.uint32), np.zeros(11, np.uint32)
        if capacity is None:
            rc = lib().vp_octree_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), algo, None, 0, ctypes.byref(m), None, None)
            if rc != 10001 or m.value == 0:                     # VP_ERR_INVALID with the count stored: the capacity
                check(rc)
            capacity = int(m.value)
        nodes = np.zeros((capacity, 2), np.uint32)
        check(lib().vp_octree_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), algo, nodes.ctypes.data_as(_vp), capacity,
                                   ctypes.byref(m), lo.ctypes.data_as(_vp), fl.ctypes.data_as(_vp)))
        return nodes[:int(m.value)], lo, fl

    def octree_expand_host(self, frame: Frame, h_nodes, algo: int = ALGO_TILED):
        """numpy in, numpy out: the grid words of the frame; the tree is validated on the host first."""
        np = __import__("numpy")
        h_nodes = np.ascontiguousarray(h_nodes, np.uint32)
        words = np.empty(frame.voxels // 32, np.uint32)
        check(lib().vp_octree_expand_host(self._h, ctypes.byref(frame), h_nodes.ctypes.data_as(_vp), h_nodes.size // 2, algo,
                                          words.ctypes.data_as(_vp)))
        return words

    def thickness_host(self, frame: Frame, h_words, rmax: int, thin2: int = 0, algo: int = ALGO_TILED):
        """numpy in, numpy out: (T2 uint32[n^3], thin words uint32[n^3 / 32], thin count)."""
        np = __import__("numpy")
        t, g, c = np.empty(frame.voxels, np.uint32), np.empty(frame.voxels // 32, np.uint32), ctypes.c_uint64()
        check(lib().vp_thickness_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), rmax, thin2, algo, t.ctypes.data_as(_vp),
                                      g.ctypes.data_as(_vp), ctypes.byref(c)))
        return t, g, int(c.value)

    def winding_host(self, frame: Frame, h_xyz, h_tri, beta: float = 2.0, level: float = 0.5, algo: int = ALGO_TILED):
        """numpy in, numpy out: (w float32[n^3], inside words uint32[n^3 / 32], inside count)."""
        np = __import__("numpy")
        w, g, c = np.empty(frame.voxels, np.float32), np.empty(frame.voxels // 32, np.uint32), ctypes.c_uint64()
        check(lib().vp_winding_host(self._h, ctypes.byref(frame), h_xyz.ctypes.data_as(_vp), h_xyz.shape[0], h_tri.ctypes.data_as(_vp),
                                    h_tri.shape[0], beta, level, algo, w.ctypes.data_as(_vp), g.ctypes.data_as(_vp), ctypes.byref(c)))
        return w, g, int(c.value)

    def voxelize_host(self, frame: Frame, h_words, h_xyz, h_tri, algo: int = ALGO_TILED):
        check(lib().vp_voxelize_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp),
                                     h_xyz.ctypes.data_as(_vp), h_xyz.shape[0], h_tri.ctypes.data_as(_vp),
                                     h_tri.shape[0], algo))

    def voxelize_conservative_host(self, frame: Frame, h_words, h_xyz, h_tri, algo: int = ALGO_TILED):
        check(lib().vp_voxelize_conservative_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp),
                                                  h_xyz.ctypes.data_as(_vp), h_xyz.shape[0], h_tri.ctypes.data_as(_vp),
                                                  h_tri.shape[0], algo))

    def fill_interior_host(self, frame: Frame, h_words, h_out):
        check(lib().vp_fill_interior_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), h_out.ctypes.data_as(_vp)))

    def morph_host(self, frame: Frame, h_words, h_out, op: int, radius: int, algo: int = ALGO_TILED):
        check(lib().vp_morph_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), h_out.ctypes.data_as(_vp), op, radius, algo))

    def edt_host(self, frame: Frame, h_words, h_dist2, seeds: int = EDT_SEEDS_SET, algo: int = ALGO_TILED):
        check(lib().vp_edt_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), seeds, h_dist2.ctypes.data_as(_vp), algo))

    def edt_sdf_host(self, frame: Frame, h_words, fill: float, h_sdf, algo: int = ALGO_TILED):
        check(lib().vp_edt_sdf_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), fill, h_sdf.ctypes.data_as(_vp), algo))

    def edt_morph_host(self, frame: Frame, h_words, h_out, op: int, radius: int, algo: int = ALGO_TILED):
        check(lib().vp_edt_morph_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), h_out.ctypes.data_as(_vp), op, radius, algo))

    def mesh_distance_host(self, frame: Frame, h_xyz, h_tri, band: int, h_sign_words=None, want_nearest: bool = True, algo: int = ALGO_TILED):
        """numpy in, numpy out: (dist2 float32[n^3], nearest uint32[n^3] or None)."""
        np = __import__("numpy")
        dist = np.empty(frame.voxels, np.float32)
        near = np.empty(frame.voxels, np.uint32) if want_nearest else None
        check(lib().vp_mesh_distance_host(self._h, ctypes.byref(frame), h_xyz.ctypes.data_as(_vp), h_xyz.shape[0], h_tri.ctypes.data_as(_vp),
                                          h_tri.shape[0], h_sign_words.ctypes.data_as(_vp) if h_sign_words is not None else None, band,
                                          dist.ctypes.data_as(_vp), near.ctypes.data_as(_vp) if want_nearest else None, algo))
        return dist, near

    def components_label_host(self, frame: Frame, h_words, h_labels, conn: int = CONN_26, algo: int = ALGO_TILED) -> int:
        count = ctypes.c_uint32()
        check(lib().vp_components_label_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), h_labels.ctypes.data_as(_vp), conn, algo,
                                             ctypes.byref(count)))
        return count.value

    def components_filter_host(self, frame: Frame, h_words, h_out, mode: int, param: int, conn: int = CONN_26, algo: int = ALGO_TILED):
        count, kept = ctypes.c_uint32(), ctypes.c_uint64()
        check(lib().vp_components_filter_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), h_out.ctypes.data_as(_vp), conn, mode,
                                              param, algo, ctypes.byref(count), ctypes.byref(kept)))
        return count.value, kept.value

    def surfnets_host(self, frame: Frame, h_words, iterations: int = 0, counts_only: bool = False):
        """numpy in, numpy out: (cells uint64[V], xyz float32[V, 3], quads uint32[Q, 4]), or (V, Q) with counts_only."""
        np = __import__("numpy")
        nv, nq = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().vp_surfnets_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), iterations, None, None, None, 0, 0,
                                     ctypes.byref(nv), ctypes.byref(nq)))
        if counts_only:
            return int(nv.value), int(nq.value)
        cells, xyz, quads = np.empty(nv.value, np.uint64), np.empty((nv.value, 3), np.float32), np.empty((nq.value, 4), np.uint32)
        check(lib().vp_surfnets_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), iterations, cells.ctypes.data_as(_vp),
                                     xyz.ctypes.data_as(_vp), quads.ctypes.data_as(_vp), cells.size, quads.shape[0],
                                     ctypes.byref(nv), ctypes.byref(nq)))
        return cells, xyz, quads

    def isonets_host(self, frame: Frame, h_field, transform: int = ISO_SIGNED_SQUARE, iso: float = 0.0, iterations: int = 0,
                     normals: bool = False, algo: int = ALGO_TILED, counts_only: bool = False):
        """numpy in, numpy out: (cells uint64[V], xyz float32[V, 3], normals float32[V, 3] or None, quads uint32[Q, 4]), or (V, Q)."""
        np = __import__("numpy")
        nv, nq = ctypes.c_uint64(), ctypes.c_uint64()
        head = (self._h, ctypes.byref(frame), h_field.ctypes.data_as(_vp), transform, iso, iterations, algo)
        check(lib().vp_isonets_host(*head, None, None, None, None, 0, 0, ctypes.byref(nv), ctypes.byref(nq)))
        if counts_only:
            return int(nv.value), int(nq.value)
        cells, xyz, quads = np.empty(nv.value, np.uint64), np.empty((nv.value, 3), np.float32), np.empty((nq.value, 4), np.uint32)
        nrm = np.empty((nv.value, 3), np.float32) if normals else None
        check(lib().vp_isonets_host(*head, cells.ctypes.data_as(_vp), xyz.ctypes.data_as(_vp), nrm.ctypes.data_as(_vp) if normals else None,
                                    quads.ctypes.data_as(_vp), cells.size, quads.shape[0], ctypes.byref(nv), ctypes.byref(nq)))
        return cells, xyz, nrm, quads

    def csg_host(self, h_a, h_b, op: int):
        check(lib().vp_csg_host(self._h, h_a.ctypes.data_as(_vp), h_b.ctypes.data_as(_vp), h_a.size, op))

    def jfa_host(self, frame: Frame, h_words, fill: float, h_sdf, algo: int = ALGO_TILED):
        check(lib().vp_jfa_host(self._h, ctypes.byref(frame), h_words.ctypes.data_as(_vp), fill,
                                h_sdf.ctypes.data_as(_vp), algo))

    # -- per-kernel device timing
    def prof_enable(self, on: bool = True):
        check(lib().vp_prof_enable(self._h, 1 if on else 0))

    def prof_select(self, names=None):
        """Time only the kernels whose timing keys are named (None = all): every event pair costs stream time."""
        mask = (1 << 64) - 1 if names is None else sum(1 << HEADER_PROF_KEYS.index(k) for k in names)
        check(lib().vp_prof_select(self._h, mask))

    def prof_reset(self):
        check(lib().vp_prof_reset(self._h))

    def prof(self):
        out = {}
        for i, name in enumerate(HEADER_PROF_KEYS):
            ms = ctypes.c_double()
            n = ctypes.c_uint64()
            check(lib().vp_prof_get(self._h, i, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[name] = {"ms": ms.value, "launches": int(n.value)}
        return out


class Multi:
    """vp_multi: one process, several devices (or several contexts on one device), Z-slabs.  Host arrays are numpy."""

    def __init__(self, devices):
        import numpy as np
        self._np = np
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self._h = _vp()
        check(lib().vp_multi_create(devs, len(devices), ctypes.byref(self._h)))
        self.frame = None

    def close(self):
        if self._h:
            lib().vp_multi_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def count(self):
        return lib().vp_multi_count(self._h)

    def set_mesh(self, xyz, tri):
        np = self._np
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        tri = np.ascontiguousarray(tri, dtype=np.uint32)
        check(lib().vp_multi_set_mesh(self._h, xyz.ctypes.data, xyz.shape[0], tri.ctypes.data, tri.shape[0]))

    def voxelize(self, frame: Frame, algo=ALGO_TILED):
        check(lib().vp_multi_voxelize(self._h, ctypes.byref(frame), algo))
        self.frame = frame                                         # only once the driver has taken it

    def set_grid(self, frame: Frame, words):
        np = self._np
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.size == frame.words
        check(lib().vp_multi_set_grid(self._h, ctypes.byref(frame), words.ctypes.data))
        self.frame = frame

    def get_grid(self):
        out = self._np.empty(self.frame.words, dtype=self._np.uint32)
        check(lib().vp_multi_get_grid(self._h, out.ctypes.data))
        return out

    def csg(self, other, op):
        other = self._np.ascontiguousarray(other, dtype=self._np.uint32)
        check(lib().vp_multi_csg(self._h, other.ctypes.data, other.size, op))

    def jfa(self, fill=float("-inf"), algo=ALGO_TILED, mode=MULTI_HALO):
        check(lib().vp_multi_jfa(self._h, fill, algo, mode))

    def get_sdf(self):
        out = self._np.empty(self.frame.voxels, dtype=self._np.float32)
        check(lib().vp_multi_get_sdf(self._h, out.ctypes.data))
        return out

    def sync(self):
        check(lib().vp_multi_sync(self._h))

    @property
    def bytes_moved(self):
        return int(lib().vp_multi_bytes_moved(self._h))

    def window(self, rank: int):
        """(lo, hi, id_bytes): global planes the rank's id volumes covered during the last jfa, and the bytes of all its id buffers"""
        lo, hi, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        check(lib().vp_multi_window(self._h, rank, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(nb)))
        return int(lo.value), int(hi.value), int(nb.value)
