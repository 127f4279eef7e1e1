"""Device-resident voxelize -> CSG -> JFA pipeline on one GPU.

torch is plumbing only (device memory + stream); every computation goes through the C ABI
(capi.Context -> libvphip.so).  Mirrors the flow of the reference CLI
(/root/reference/apps/cli/main.cpp:62-218): one frame shared by all meshes, one grid per mesh,
CSG accumulated into grid 0, JFA on grid 0 with an -inf pre-fill.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import capi
from .capi import ALGO_NAIVE, ALGO_TILED, Frame  # noqa: F401


class _DeviceView:
    """A buffer of the context as an array for torch.as_tensor (no copy); `owner` keeps the engine alive with it."""

    def __init__(self, ptr: int, count: int, typestr: str, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}


class Engine:
    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("Engine needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.ctx = capi.Context(device)
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream, external=True)
        self._work = None

    # -- buffers ---------------------------------------------------------------------------
    def to_device(self, arr, dtype):
        t = torch.from_numpy(np.array(arr, dtype=dtype, order="C", copy=True).view(np.int32 if dtype == np.uint32 else dtype))
        return t.to(self.device)

    def mesh_to_device(self, xyz, tri):
        return self.to_device(xyz, np.float32), self.to_device(tri, np.uint32)

    def new_grid(self, frame: Frame):
        return torch.empty(frame.words, dtype=torch.int32, device=self.device)

    def _workspace(self, nbytes: int):
        if self._work is None or self._work.numel() < nbytes:
            self._work = None
            self._work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._work

    # -- stages ----------------------------------------------------------------------------
    def voxelize(self, frame: Frame, d_xyz, d_tri, out=None, algo=ALGO_TILED, accumulate=False):
        if out is None:
            out = self.new_grid(frame)
            if accumulate:
                out.zero_()
        self.ctx.voxelize(frame, out.data_ptr(), d_xyz.data_ptr(), d_xyz.shape[0], d_tri.data_ptr(), d_tri.shape[0],
                          algo, accumulate)
        return out

    def voxelize_conservative(self, frame: Frame, d_xyz, d_tri, out=None, algo=ALGO_TILED, accumulate=False):
        """Surface grid: every voxel whose closed box overlaps a triangle (any mesh, open or closed).  accumulate ORs into `out`."""
        if out is None:
            out = self.new_grid(frame)
            if accumulate:
                out.zero_()
        self.ctx.voxelize_conservative(frame, out.data_ptr(), d_xyz.data_ptr(), d_xyz.shape[0], d_tri.data_ptr(), d_tri.shape[0],
                                       algo, accumulate)
        return out

    def fill_interior(self, frame: Frame, words, out=None):
        """Solid from any grid: `words` plus every empty voxel that no 6-connected path of empty voxels joins to the grid boundary.
        Blocking; returns (out, rounds)."""
        if out is None:
            out = self.new_grid(frame)
        rounds = self.ctx.fill_interior(frame, words.data_ptr(), out.data_ptr())
        return out, rounds

    def morph(self, frame: Frame, words, op: int, radius: int, out=None, algo: int = ALGO_TILED):
        """Ball morphology of a whole grid: out = dilate / erode / open / close (capi.MORPH_*) of `words` by the integer ball of `radius`
        (0 .. 32).  `out` must not be `words`.  Enqueues only; returns out."""
        if out is None:
            out = self.new_grid(frame)
        self.ctx.morph(frame, words.data_ptr(), out.data_ptr(), op, radius, algo)
        return out

    def edt(self, frame: Frame, words, seeds: int = capi.EDT_SEEDS_SET, out=None, algo: int = ALGO_TILED):
        """Exact Euclidean distance transform of a whole grid (n <= 1024): an int32 tensor of n^3 squared voxel distances, x fastest, to
        the nearest seed -- capi.EDT_SEEDS_SET (set voxels), EDT_SEEDS_UNSET (unset voxels) or EDT_SEEDS_BORDER (the JFA's seeds).  A grid
        without seeds gives capi.EDT_NONE (-1 as int32) everywhere.  Enqueues only; returns out."""
        if out is None:
            out = torch.empty(frame.voxels, dtype=torch.int32, device=self.device)
        self.ctx.edt(frame, words.data_ptr(), out.data_ptr(), seeds, algo)
        return out

    def edt_sdf(self, frame: Frame, words, out=None, fill=-math.inf, algo: int = ALGO_TILED):
        """jfa() without its error: +-(squared distance to the nearest border voxel), exact.  Enqueues only; returns out."""
        if out is None:
            out = torch.empty(frame.voxels, dtype=torch.float32, device=self.device)
        self.ctx.edt_sdf(frame, words.data_ptr(), fill, out.data_ptr(), algo)
        return out

    def edt_morph(self, frame: Frame, words, op: int, radius: int, out=None, algo: int = ALGO_TILED):
        """morph() for any integer radius 0 .. 65535, through the distance transform.  `out` must not be `words`.  Enqueues only."""
        if out is None:
            out = self.new_grid(frame)
        self.ctx.edt_morph(frame, words.data_ptr(), out.data_ptr(), op, radius, algo)
        return out

    def mesh_distance(self, frame: Frame, d_xyz, d_tri, band: int, sign_words=None, want_nearest: bool = False, out=None, algo: int = ALGO_TILED):
        """Narrow-band distance field to the triangles themselves (n <= 1024, band = 1 .. 32 voxels): a float32 tensor of n^3 values
        min(B2, squared distance from the voxel centre to the nearest triangle), B = band * voxel size, x fastest; signed by `sign_words`
        (a grid: + on set voxels, - on unset ones) if given.  want_nearest: also an int32 tensor with the index of the nearest face,
        capi.MESH_NONE (-1 as int32) outside the band.  `out` = dist2, or (dist2, nearest).  Returns dist2, or (dist2, nearest)."""
        dist, nearest = out if isinstance(out, (tuple, list)) else (out, None)
        if dist is None:
            dist = torch.empty(frame.voxels, dtype=torch.float32, device=self.device)
        if want_nearest and nearest is None:
            nearest = torch.empty(frame.voxels, dtype=torch.int32, device=self.device)
        self.ctx.mesh_distance(frame, d_xyz.data_ptr(), d_xyz.shape[0], d_tri.data_ptr(), d_tri.shape[0], band, dist.data_ptr(),
                               nearest.data_ptr() if want_nearest else 0, sign_words.data_ptr() if sign_words is not None else 0, algo)
        return (dist, nearest) if want_nearest else dist

    def components_label(self, frame: Frame, words, conn: int = capi.CONN_26, algo: int = ALGO_TILED, out=None):
        """Connected components of the set voxels of a whole grid (capi.CONN_6 / CONN_26).  Returns (labels, K): an int32 tensor of n^3
        labels, x fastest, 0 = background, components 1 .. K in the order of their lowest voxel index -- scipy.ndimage.label's
        numbering.  Blocking."""
        if out is None:
            out = torch.empty(frame.voxels, dtype=torch.int32, device=self.device)
        count = self.ctx.components_label(frame, words.data_ptr(), out.data_ptr(), conn, algo)
        return out, count

    def components_sizes(self, frame: Frame, labels, count: int):
        """Voxels per component: an int32 tensor of `count` sizes, sizes[k - 1] for label k.  Blocking."""
        sizes = torch.empty(max(count, 1), dtype=torch.int32, device=self.device)[:count]
        self.ctx.components_sizes(frame, labels.data_ptr(), count, sizes.data_ptr() if count else 0)
        return sizes

    def components_filter(self, frame: Frame, words, mode: int, param: int, conn: int = capi.CONN_26, out=None, algo: int = ALGO_TILED):
        """Size filter: capi.COMP_KEEP_LARGEST keeps the `param` (1 .. 16) largest components (ties: the lower label), capi.COMP_MIN_VOXELS
        those with at least `param` voxels.  `out` must not be `words`.  Blocking; returns (out, K, kept voxels)."""
        if out is None:
            out = self.new_grid(frame)
        count, kept = self.ctx.components_filter(frame, words.data_ptr(), out.data_ptr(), mode, param, conn, algo)
        return out, count, kept

    def surface_nets(self, frame: Frame, words, iterations: int = 0, algo: int = ALGO_TILED):
        """Surface-nets mesh of a whole grid (n <= 1024): one vertex per boundary cell, one quad per exposed voxel face, closed.  Returns
        device tensors (cells int64[V]: cell index | corner mask << 40; xyz float32[V, 3]: lattice coordinates after `iterations` (0 .. 64)
        relaxation steps; quads int32[Q, 4]: vertex indices, outward winding).  Blocking (the counts size the tensors)."""
        nv, nq = self.ctx.surfnets_count(frame, words.data_ptr(), algo)
        cells = torch.empty(nv, dtype=torch.int64, device=self.device)
        xyz = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
        quads = torch.empty((nq, 4), dtype=torch.int32, device=self.device)
        self.ctx.surfnets(frame, words.data_ptr(), algo, iterations, cells.data_ptr() if nv else 0, xyz.data_ptr() if nv else 0,
                          quads.data_ptr() if nq else 0, nv, nq)
        return cells, xyz, quads

    def iso_nets(self, frame: Frame, field, iso: float = 0.0, transform: int = capi.ISO_SIGNED_SQUARE, iterations: int = 0,
                 normals: bool = False, algo: int = ALGO_TILED):
        """Surface nets of a float32 field tensor (n^3 values, x fastest; n <= 1024) at level `iso`: vertices at the field's edge crossings,
        the topology of surface_nets() on the inside set {h >= +0}, h = field - iso (capi.ISO_LINEAR) or sign(field) sqrt|field| - iso
        (capi.ISO_SIGNED_SQUARE, the convention of jfa() / edt_sdf() / mesh_distance()).  Returns (cells int64[V], xyz float32[V, 3],
        normals float32[V, 3] or None, quads int32[Q, 4]): tensors of the caller, copied out of the context's buffers.  Blocking."""
        nv, nq = self.ctx.isonets(frame, field.data_ptr(), transform, iso, iterations, normals, algo)
        dc, dx, dn, dq, _, _ = self.ctx.isonets_result()
        cells = torch.empty(nv, dtype=torch.int64, device=self.device)
        xyz = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
        nrm = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if normals else None
        quads = torch.empty((nq, 4), dtype=torch.int32, device=self.device)
        if nv:
            self.ctx.memcpy_d2d(cells.data_ptr(), dc, nv * 8)
            self.ctx.memcpy_d2d(xyz.data_ptr(), dx, nv * 12)
            if normals:
                self.ctx.memcpy_d2d(nrm.data_ptr(), dn, nv * 12)
            self.ctx.memcpy_d2d(quads.data_ptr(), dq, nq * 16)
        return cells, xyz, nrm, quads

    def winding(self, frame: Frame, d_xyz, d_tri, beta: float = 2.0, level: float = 0.5, algo: int = ALGO_TILED):
        """Generalized winding number of the mesh at the voxel centres (n <= 1024): returns (w, inside) -- a float32 tensor of n^3 values, x
        fastest (1 inside a closed outward-oriented mesh, 0 outside, smooth through open boundaries), and the grid of the voxels with
        w >= level in the library's bit layout, ready for mesh_distance(sign_words=...), csg(), morph(), surface_nets() ...  beta = 0 sums
        every triangle exactly, beta = 1 .. 64 opens the far field (2 is the usual choice).  Both tensors are VIEWS of buffers the context
        owns: they are overwritten by the next winding() and die with release() / close() -- clone() what has to live longer.  Enqueues only."""
        self.ctx.winding(frame, d_xyz.data_ptr(), d_xyz.shape[0], d_tri.data_ptr(), d_tri.shape[0], beta, level, algo)
        dw, dg, _ = self.ctx.winding_result()
        return (torch.as_tensor(_DeviceView(dw, frame.voxels, "<f4", self), device=self.device),
                torch.as_tensor(_DeviceView(dg, frame.voxels // 32, "<i4", self), device=self.device))

    def thickness(self, frame: Frame, words, rmax: int, thin2: int = 0, algo: int = ALGO_TILED):
        """Local thickness of a grid (n <= 1024) in a band of rmax = 1 .. 32 voxels: returns (t2, thin) -- a tensor of n^3 values, x fastest,
        the squared radius of the largest ball that fits inside the solid and contains the voxel (0 on unset voxels, rmax^2 where the part
        is thicker than 2 rmax; the thickness in voxels is 2 sqrt(t2)), and the grid of the set voxels with t2 < thin2 in the library's bit
        layout, ready for components(), morph(), surface_nets() ...  Pore or channel width is the same call on ~words.  Both tensors are
        VIEWS of buffers the context owns: they are overwritten by the next thickness() and die with release() / close() -- clone() what
        has to live longer (the thin grid too, before it goes back in as `words`).  Enqueues only."""
        self.ctx.thickness(frame, words.data_ptr(), rmax, thin2, algo)
        dt, dg, _ = self.ctx.thickness_result()
        return (torch.as_tensor(_DeviceView(dt, frame.voxels, "<i4", self), device=self.device),
                torch.as_tensor(_DeviceView(dg, frame.voxels // 32, "<i4", self), device=self.device))

    def skeleton(self, frame: Frame, words, mode: int = capi.SKEL_CURVE, max_iters: int = 0, anchor=None, algo: int = ALGO_TILED):
        """Topological thinning of a grid (n <= 1024): returns (skel, stats) -- the grid of the voxels that are left, in the library's bit
        layout, ready for components(), octree(), surface_nets() ..., and (voxels left, iterations, voxels deleted).  capi.SKEL_CURVE keeps
        line ends and gives the one-voxel-wide centre line, capi.SKEL_KERNEL the homotopy kernel (a ball shrinks to one voxel, a torus to a
        closed loop); both keep the 26-components of the solid and the 6-components of its complement.  `anchor` is an optional grid whose
        voxels are never deleted; max_iters > 0 stops after that many iterations (a partial homotopic erosion).  The grid is a VIEW of a
        buffer the context owns: it is overwritten by the next skeleton() and dies with release() / close() -- clone() what has to live
        longer (also before it goes back in as `words` or `anchor`).  Blocking."""
        stats = self.ctx.skeleton(frame, words.data_ptr(), mode, max_iters, 0 if anchor is None else anchor.data_ptr(), algo)
        dg, _, _ = self.ctx.skeleton_result()
        return torch.as_tensor(_DeviceView(dg, frame.voxels // 32, "<i4", self), device=self.device), stats

    def reconstruct(self, frame: Frame, marker, mask, domain=None, mode: int = capi.REC_DILATION, connectivity: int = capi.CONN_6,
                    algo: int = ALGO_TILED):
        """Grayscale reconstruction of a grid (n <= 1024): returns (field, stats) -- a tensor of n^3 values, x fastest: the marker field
        raised under the mask field along paths inside `domain` (a bit grid in the library's layout; None: every voxel) for
        capi.REC_DILATION, lowered above it for capi.REC_EROSION; off the domain it reads 0 / -1 in the int32 view -- and (domain voxels,
        voxels that changed, sum of the field over the domain, its largest value -- erosion: the smallest).  The tensor is a VIEW of a
        buffer the context owns: it is overwritten by the next reconstruct() and dies with release() / close() -- clone() what has to
        live longer (also before it goes back in as `marker` or `mask`).  Blocking."""
        stats = self.ctx.reconstruct(frame, marker.data_ptr(), mask.data_ptr(), 0 if domain is None else domain.data_ptr(), mode, connectivity, algo)
        dr, _, _ = self.ctx.reconstruct_result()
        return torch.as_tensor(_DeviceView(dr, frame.voxels, "<i4", self), device=self.device), stats

    def extrema(self, frame: Frame, values, domain=None, kind: int = capi.EXT_MAXIMA, scale: int = capi.EXT_LINEAR, h: int = 0,
                connectivity: int = capi.CONN_6, algo: int = ALGO_TILED):
        """h-extrema of a value field of a grid (n <= 1024): returns (scaled, flat, extrema, stats) -- the scaled field V (the values, or
        floor(sqrt(256 v)) for capi.EXT_SQRT16: a squared distance in sixteenths of a voxel), the field H with every maximum (minimum)
        of depth below h flattened, the grid of the extended maxima (minima) in the library's bit layout -- label it with components()
        for the markers of watershed(), and flood V -- and (domain voxels, extrema voxels, largest H -- minima: the smallest --, voxels
        with H != V).  The three tensors are VIEWS of buffers the context owns: they are overwritten by the next extrema() and die with
        release() / close() -- clone() what has to live longer (also before one goes back in).  Blocking."""
        stats = self.ctx.extrema(frame, values.data_ptr(), 0 if domain is None else domain.data_ptr(), kind, scale, h, connectivity, algo)
        dv, df, de, _, _ = self.ctx.extrema_result()
        return (torch.as_tensor(_DeviceView(dv, frame.voxels, "<i4", self), device=self.device),
                torch.as_tensor(_DeviceView(df, frame.voxels, "<i4", self), device=self.device),
                torch.as_tensor(_DeviceView(de, frame.voxels // 32, "<i4", self), device=self.device), stats)

    def geodesic(self, frame: Frame, mask, seeds, metric: int = capi.GEO_CHAMFER, algo: int = ALGO_TILED):
        """Geodesic distance of a grid (n <= 1024): returns (dist, reach, stats) -- a tensor of n^3 values, x fastest, the length of the
        shortest path from a seed voxel that stays inside `mask` (0 at the seeds inside the mask; capi.GEO_NONE, which reads -1 in the
        int32 view, where no path arrives and outside the mask), the grid of the reached voxels in the library's bit layout -- the
        components of the mask that touch a seed, ready for components(), octree() ... -- and (seeds used, voxels reached, largest
        finite distance, lowest linear index that attains it).  A step to a face / edge / corner neighbour costs 1 / - / - (capi.GEO_6),
        1 / 1 / 1 (capi.GEO_26) or 3 / 4 / 5 (capi.GEO_CHAMFER: divide by 3 for voxels).  Both tensors are VIEWS of buffers the context
        owns: they are overwritten by the next geodesic() and die with release() / close() -- clone() what has to live longer (the reach
        grid too, before it goes back in as `mask` or `seeds`).  Blocking."""
        stats = self.ctx.geodesic(frame, mask.data_ptr(), seeds.data_ptr(), metric, algo)
        dd, dr, _, _ = self.ctx.geodesic_result()
        return (torch.as_tensor(_DeviceView(dd, frame.voxels, "<i4", self), device=self.device),
                torch.as_tensor(_DeviceView(dr, frame.voxels // 32, "<i4", self), device=self.device), stats)

    def watershed(self, frame: Frame, mask, markers, priority=None, order: int = capi.WS_DESCENDING, quantum: int = 1,
                  connectivity: int = capi.CONN_6, algo: int = ALGO_TILED):
        """Seeded watershed of a grid (n <= 1024): returns (labels, cut, stats) -- a tensor of n^3 labels, x fastest (0 where no marker
        arrives and outside `mask`), the cut grid in the library's bit layout -- the labelled voxels that no neighbour with a larger
        label touches: the parts, separated, ready for components(), thickness(), octree(), surface_nets() ... -- and (marker voxels used,
        voxels labelled, levels present, voxels cut).  `markers` is an int32 tensor of n^3 labels (0 = none, 1 .. capi.WS_LABEL_MAX), as
        components_label() writes it; `priority` an int32 tensor of n^3 values read as uint32, as edt() writes it, flooded in levels
        priority // quantum from the high end (capi.WS_DESCENDING: what a distance map needs) or the low end (capi.WS_ASCENDING).
        priority = None gives the geodesic influence zones of the markers: every voxel takes the label of the marker that is nearest
        through the mask, the smaller label at equal hops.  Both tensors are VIEWS of buffers the context owns: they are overwritten by
        the next watershed() and die with release() / close() -- clone() what has to live longer (also before one goes back in).
        Blocking."""
        stats = self.ctx.watershed(frame, mask.data_ptr(), markers.data_ptr(), 0 if priority is None else priority.data_ptr(), order, quantum,
                                   connectivity, algo)
        dl, dc, _, _ = self.ctx.watershed_result()
        return (torch.as_tensor(_DeviceView(dl, frame.voxels, "<i4", self), device=self.device),
                torch.as_tensor(_DeviceView(dc, frame.voxels // 32, "<i4", self), device=self.device), stats)

    def regions(self, frame: Frame, labels, count: int, values=None, algo: int = ALGO_TILED):
        """Region analysis of a label volume (n <= 1024): returns (table, stats) -- an int64 tensor (count, 26), one record per label
        1 .. count as include/vphip.h lays it out (read the words as uint64: voxels, bounding box, first and second moments, exposed and
        contact faces, lattice points and edges, sum / min / max of `values`, first voxel; capi.region_table(table.cpu().numpy(), frame)
        derives centroid, ellipsoid, surface, Euler number ...), and (sum of V, labels with V > 0, voxels ignored, interfaces).  `labels` is
        an int32 tensor of n^3 labels as components_label() and watershed() write it (labels above `count` are ignored), `values` an
        optional int32 tensor of n^3 values read as uint32, as edt() writes it.  The tensor is a VIEW of a buffer the context owns: it is
        overwritten by the next regions() and dies with release() / close() -- clone() what has to live longer.  Blocking."""
        stats = self.ctx.regions(frame, labels.data_ptr(), count, 0 if values is None else values.data_ptr(), algo)
        dt, k, _, _ = self.ctx.regions_result()
        if k == 0:
            return torch.zeros((0, capi.REGION_WORDS), dtype=torch.int64, device=self.device), stats
        return torch.as_tensor(_DeviceView(dt, k * capi.REGION_WORDS, "<i8", self), device=self.device).view(k, capi.REGION_WORDS), stats

    def octree(self, frame: Frame, words, algo: int = ALGO_TILED):
        """Sparse voxel octree of a grid (n <= 1024): returns (nodes, level_offset, full_leaves) -- an int32 tensor of M x 2 words, the
        records (valid | full << 8, index of the first mixed child) breadth-first and in Morton order within a level, and two lists of 11:
        the running sums of the per-level node counts and the full children per level (include/vphip.h, vp_octree).  `nodes` is a VIEW of
        a buffer the context owns: it is overwritten by the next octree() and dies with release() / close() -- clone() what has to live
        longer.  Blocks once: the node count is read back."""
        m = self.ctx.octree(frame, words.data_ptr(), algo)
        d, _, lo, fl, _ = self.ctx.octree_result()
        return torch.as_tensor(_DeviceView(d, 2 * m, "<i4", self), device=self.device).view(m, 2), lo, fl

    def octree_expand(self, frame: Frame, nodes, algo: int = ALGO_TILED):
        """The bit grid of the frame from a tree (a tensor of M x 2 words, as octree() returns it or uploaded from a validated file), ready
        for components(), morph(), surface_nets() ...  A VIEW of a grid the context owns: it is overwritten by the next octree_expand() and
        dies with release() / close() -- clone() what has to live longer.  Enqueues only."""
        self.ctx.octree_expand(frame, nodes.data_ptr(), nodes.numel() // 2, algo)
        d, _ = self.ctx.octree_expand_result()
        return torch.as_tensor(_DeviceView(d, frame.voxels // 32, "<i4", self), device=self.device)

    def csg(self, a, b, op: int):
        self.ctx.csg(a.data_ptr(), b.data_ptr(), a.numel(), op)
        return a

    def jfa(self, frame: Frame, words, out=None, fill=-math.inf, algo=ALGO_TILED):
        if out is None:
            out = torch.empty(frame.voxels, dtype=torch.float32, device=self.device)
        nb = self.ctx.jfa_workspace_bytes(frame)
        work = self._workspace(nb)
        self.ctx.jfa(frame, words.data_ptr(), fill, out.data_ptr(), work.data_ptr(), nb, algo)
        return out

    def surface(self, frame: Frame, words, out=None):
        if out is None:
            out = self.new_grid(frame)
        self.ctx.surface(frame, words.data_ptr(), None, None, out.data_ptr())
        return out

    def sync(self):
        self.ctx.sync()

    @staticmethod
    def words_to_numpy(t):
        return t.detach().cpu().numpy().view(np.uint32)
