"""ctypes loader for the in-tree native libraries.

``libflimo_hip.so``  -- HIP kernels + C ABI declared in ``include/flimo_c.h`` (the drop-in boundary)
``libfast_limo.so``  -- host C++ mirror of the reference's Localizer / Mapper / esekf on top of it

There is no Python or CPU fallback: if a library is missing or no gfx950 device is present the
calls raise (``FlimoError``).  The structures and the functions' signatures are in ``_abi``.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

from . import _abi
# (every structure stays a name of this module: callers and tests say _lib.MatchCfg, _lib.Frame, ...)
from ._abi import (CHAIN_MAX_PASSES, CarveCfg, ChainIO, ChainPass, ClusterCfg, ClusterStats, CorrCfg, CorrGraphCfg, FilterCfg, FpfhCfg, Frame,
                   GicpCfg, GicpInfo, KeypointCfg, MapCfg, MatchCfg, NdtCfg, NdtInfo, OutlierCfg, OutlierStats, PlaneCfg, PlaneSel, RegionCfg, RegionStats, ScCfg, ScMatchCfg, VoxelCfg, VoxelStats,
                   f32p, f64p, i32p)

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)


class FlimoError(RuntimeError):
    pass


RADIUS_SORTED = 1      # FLIMO_RADIUS_SORTED


def carve_cfg(res=256, win=1, margin=0.2, rel_margin=0.02, max_depth=float("inf")) -> CarveCfg:
    """The documented defaults: a 256-pixel cube face, a 3 x 3 window, 0.2 m + 2 % of the depth, no depth bound."""
    return CarveCfg(int(res), int(win), float(margin), float(rel_margin), float(max_depth))


def outlier_cfg(k=8, max_dist=float("inf"), min_pts=0, std_mul=1.0) -> OutlierCfg:
    """PCL's StatisticalOutlierRemoval with 8 neighbours and one sigma unless told otherwise: no gate, no count rule."""
    return OutlierCfg(int(k), float(max_dist), int(min_pts), float(std_mul))


def fpfh_cfg(k=32, max_dist=float("inf"), normal_k=10, normal_max_dist=float("inf"), normal_min_pts=3, viewpoint=None) -> FpfhCfg:
    """A feature neighbourhood of 32 and normals from 10 neighbours unless told otherwise: no gates, the normals' own orientation."""
    vp = (0.0, 0.0, 0.0) if viewpoint is None else tuple(float(v) for v in np.asarray(viewpoint, dtype=np.float32).reshape(3))
    return FpfhCfg(int(k), float(max_dist), int(normal_k), float(normal_max_dist), int(normal_min_pts), 0 if viewpoint is None else 1,
                   (C.c_float * 3)(*vp))


def keypoint_cfg(k=32, max_dist=float("inf"), min_pts=5, gamma21=0.975, gamma32=0.975, nms_k=32, nms_max_dist=float("inf")) -> KeypointCfg:
    """PCL's ISSKeypoint3D thresholds (0.975, 0.975, 5 neighbours) over neighbourhoods of 32 unless told otherwise: no gates."""
    return KeypointCfg(int(k), float(max_dist), int(min_pts), float(gamma21), float(gamma32), int(nms_k), float(nms_max_dist))


def cluster_cfg(tol=0.5, min_size=1, max_size=0) -> ClusterCfg:
    """Half a metre, every component selected unless told otherwise (``max_size`` 0: no upper bound)."""
    return ClusterCfg(float(tol), int(min_size), int(max_size))


CORR_OK, CORR_DEGENERATE, CORR_REJECTED = 0, 1, 2      # FLIMO_CORR_*: the status of a hypothesis


def corr_cfg(edge_sim=0.9, min_edge=0.0, max_dist=float("inf")) -> CorrCfg:
    """PCL's SampleConsensusPrerejective similarity threshold of 0.9 unless told otherwise: no shortest edge, no inlier gate."""
    return CorrCfg(float(edge_sim), float(min_edge), float(max_dist))


PLANE_OK, PLANE_DEGENERATE, PLANE_REJECTED = 0, 1, 2      # FLIMO_PLANE_*: the status of a hypothesis
PLANE_SLAB = 8192      # FLIMO_PLANE_SLAB


def plane_cfg(dist=0.05, min_edge=0.0, min_sin=0.0, axis=(0.0, 0.0, 1.0), min_cos=0.0) -> PlaneCfg:
    """A 5 cm gate unless told otherwise: no shortest edge, no collinearity test, no axis constraint."""
    ax = np.asarray(axis, np.float32).reshape(3)
    return PlaneCfg(float(dist), float(min_edge), float(min_sin), (C.c_float * 3)(*[float(v) for v in ax]), float(min_cos))


def plane_sel(normal, anchor, dist=0.05, side=0) -> PlaneSel:
    """The plane of float32 ``normal`` through ``anchor`` with the gate ``dist``; side 0: |t| < dist, -1: t < dist, +1: t > -dist."""
    nf = np.asarray(normal, np.float32).reshape(3)
    an = np.asarray(anchor, np.float32).reshape(3)
    return PlaneSel((C.c_float * 3)(*[float(v) for v in nf]), (C.c_float * 3)(*[float(v) for v in an]), float(dist), int(side))


def _as_plane_sel(sel, kw):
    if isinstance(sel, PlaneSel):
        if kw:
            raise ValueError("plane: give a PlaneSel or the fields of plane_sel, not both")
        return sel
    if sel is not None:
        raise ValueError("plane: sel must be a PlaneSel")
    return plane_sel(**kw)


VOXEL_KEEP_FIRST, VOXEL_KEEP_NEAREST = 0, 1      # FLIMO_VOXEL_KEEP_*
VOXEL_RUN = 64                                   # FLIMO_VOXEL_RUN
VOXEL_HALF = 1 << 20                             # FLIMO_VOXEL_HALF
VOXEL_OUTPUTS = (("ijk", np.int32, 3), ("count", np.int32, 1), ("first", np.int32, 1), ("rep", np.int32, 1),
                 ("centroid", np.float64, 3), ("cov", np.float64, 6))


def voxel_cfg(leaf=0.25, keep=VOXEL_KEEP_FIRST, max_pts=1) -> VoxelCfg:
    """A 25 cm leaf that keeps the oldest point of a voxel unless told otherwise."""
    return VoxelCfg(float(leaf), int(keep), int(max_pts))


REGION_OUTPUTS = (("label", np.int32, 1), ("count", np.int32, 1), ("first", np.int32, 1), ("centroid", np.float64, 3), ("cov", np.float64, 6))
REGION_LIST_CAP = 1024      # regions the first call of ``map_region_list`` has room for


def region_cfg(tol=0.5, normal_k=16, normal_max_dist=float("inf"), normal_min_pts=3, min_cos=0.93969262, max_curv=0.05, border=1, min_size=1,
               max_size=0) -> RegionCfg:
    """Half a metre, normals of 16 neighbours within 20 degrees of each other (``min_cos`` is the cosine), curvature up to 0.05,
    border points attached, every region selected unless told otherwise (``max_size`` 0: no upper bound)."""
    return RegionCfg(float(tol), int(normal_k), float(normal_max_dist), int(normal_min_pts), float(min_cos), float(max_curv), int(border),
                     int(min_size), int(max_size))


CORR_GRAPH_MAX_M = 32768      # FLIMO_CORR_GRAPH_MAX_M


def corr_graph_cfg(tol=0.05, min_edge=0.0, edge_sim=0.0) -> CorrGraphCfg:
    """Edge lengths within 5 cm of each other unless told otherwise: no shortest edge, no polygon test."""
    return CorrGraphCfg(float(tol), float(min_edge), float(edge_sim))


DESC_MAX_DIM, DESC_MAX_K = 64, 8      # FLIMO_DESC_MAX_DIM / FLIMO_DESC_MAX_K


def desc_rows(desc):
    """A descriptor array as the calls take it: C-contiguous float32 [n, dim] (a 1-D array is one column)."""
    d = np.ascontiguousarray(desc, dtype=np.float32)
    return d.reshape(-1, 1) if d.ndim == 1 else d.reshape(d.shape[0], int(np.prod(d.shape[1:])))


SC_MAX_RINGS, SC_MAX_SECTORS, SC_MAX_K = 32, 64, 8      # FLIMO_SC_MAX_*


def sc_cfg(rings=20, sectors=60, min_range=0.0, max_range=80.0, z_offset=2.0) -> ScCfg:
    """Scan Context's published shape unless told otherwise: 20 rings x 60 sectors out to 80 m, the sensor 2 m above the ground."""
    return ScCfg(int(rings), int(sectors), float(min_range), float(max_range), float(z_offset))


def _as_sc_cfg(cfg, kw):
    if isinstance(cfg, ScCfg):
        if kw:
            raise ValueError("scan context: give a ScCfg or the fields of sc_cfg, not both")
        return cfg
    if cfg is not None:
        raise ValueError("scan context: cfg must be a ScCfg")
    return sc_cfg(**kw)


def _frame12(frame12):
    """A row-major 3 x 4 transform as the calls take it: float32 [12], None for none."""
    return None if frame12 is None else np.ascontiguousarray(frame12, dtype=np.float32).reshape(12)


def sc_rows(desc):
    """Descriptors as the calls take them: C-contiguous float32 [n, rings, sectors] (a 2-D array is one descriptor)."""
    d = np.ascontiguousarray(desc, dtype=np.float32)
    if d.ndim == 2:
        d = d.reshape(1, *d.shape)
    if d.ndim != 3:
        raise ValueError("scan context: descriptors are [n, rings, sectors]")
    return d


MATCH_REC_DTYPE = np.dtype([
    ("H", np.float32, 12), ("h", np.float32), ("valid", np.float32), ("n", np.float32, 4),
    ("p_global", np.float32, 3), ("sqd", np.float32, 5), ("nbr", np.int32, 5), ("n_nbr", np.int32)])

FRAME_DTYPE = np.dtype([
    ("p", np.float32, 3), ("q", np.float32, 4), ("v", np.float32, 3), ("g", np.float32, 3), ("w", np.float32, 3),
    ("a", np.float32, 3), ("bg", np.float32, 3), ("ba", np.float32, 3), ("_pad", np.float32), ("time", np.float64)])

HIP_SYMBOLS = _abi.HIP_SYMBOLS      # every symbol include/flimo_c.h and include/flimo_dev.h declare (tests check the .so exports each one)

_hip = None


def hip_lib_path() -> str:
    # FLIMO_HIP_LIB: developer override (e.g. the phase-stamp build libflimo_hip_trace.so)
    return os.environ.get("FLIMO_HIP_LIB") or os.path.join(_PKG, "libflimo_hip.so")


def load_hip():
    """Load libflimo_hip.so and declare the C ABI.  Raises FlimoError when the library is absent."""
    global _hip
    if _hip is not None:
        return _hip
    path = hip_lib_path()
    if not os.path.exists(path):
        raise FlimoError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` first")
    L = C.CDLL(path)
    _abi.declare(L, 0)
    _hip = L
    return L


_ERRS = {-1: "no gfx950 device", -2: "invalid argument", -3: "HIP error", -4: "no map", -5: "too large",
         -6: "unsupported", -7: "TIMEOUT"}

# ---- the entries a HipCtx and an api.Localizer share ----
# The outputs of an entry that fills one row per point, query or listed item: (name, dtype, width), in the order of the call's
# arguments (VOXEL_OUTPUTS and REGION_OUTPUTS above are two more).
_OUTLIER_OUTPUTS = (("mask", np.uint8, 1), ("mean_dist", np.float64, 1), ("cnt", np.int32, 1))
_FPFH_OUTPUTS = (("fpfh", np.float32, 33), ("spfh", np.uint8, 33), ("cnt", np.int32, 1))
_KEYPOINT_OUTPUTS = (("mask", np.uint8, 1), ("saliency", np.float64, 1), ("cnt", np.int32, 1))
_COMPONENT_OUTPUTS = (("label", np.int32, 1), ("size", np.int32, 1), ("mask", np.uint8, 1))      # clusters and regions
_VOXEL_MASK_OUTPUTS = (("voxel", np.int32, 1), ("mask", np.uint8, 1))
_NORMAL_OUTPUTS = (("normal", np.float32, 4), ("cnt", np.int32, 1), ("centroid", np.float64, 3), ("cov", np.float64, 6), ("eig", np.float64, 6))

NDT_CELL_OUTPUTS = (("ijk", np.int32, 3), ("count", np.int32, 1), ("mean", np.float64, 3), ("evec", np.float64, 9), ("wgt", np.float64, 3),
                    ("eval", np.float64, 3))
NDT_SLOTS = 4          # FLIMO_NDT_SLOTS
GICP_PLANE, GICP_CLAMP = 0, 1      # FLIMO_GICP_PLANE, FLIMO_GICP_CLAMP: the rules of gicp_build / api.gicp_regularize_host

_NONE = C.create_string_buffer(8)


def _ptr(a):
    """The address of an array as a call takes it.  None -- an output left out -- stays None; an array of no element, which may
    have no address, points at eight spare bytes: the calls want their required pointers non-null."""
    return None if a is None else (a.ctypes.data if a.size else C.addressof(_NONE))


def _outputs(what, table, want, rows, always=()):
    """The zeroed output arrays of an entry by name, ``rows`` long each: those of ``table`` that are in ``always`` or named in
    ``want``.  A name in ``want`` that is none of the entry's optional outputs raises."""
    unknown = set(want) - {name for name, _, _ in table if name not in always}
    if unknown:
        raise ValueError(f"{what}: unknown outputs {sorted(unknown)}")
    return {name: np.zeros((rows, w) if w > 1 else rows, dt) for name, dt, w in table if name in always or name in want}


def _ptrs(arr, table):
    return [_ptr(arr.get(name)) for name, _, _ in table]


def _result(arr, stats=None, rows=None):
    """What the method returns: the arrays -- copies of their first ``rows`` rows where the call said how many it filled --,
    ``mask`` as bool, and ``stats`` as a dict."""
    out = dict(arr) if rows is None else {name: a[:rows].copy() for name, a in arr.items()}
    if "mask" in out:
        out["mask"] = out["mask"].astype(bool)
    if stats is not None:
        out["stats"] = stats.as_dict()
    return out


def _poses(x26s):
    return np.ascontiguousarray(x26s, dtype=np.float64).reshape(-1, 26)


def _pairs(what, src, dst):
    s = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dst, dtype=np.float32).reshape(-1, 3)
    if s.shape != d.shape:
        raise ValueError(f"{what}: src and dst must hold the same number of points")
    return s, d


def seg_mats(T):
    """Matrices of ``map_correct`` as float64 [S, 12]: from [S, 12], [S, 3, 4], [S, 4, 4] (the last row is dropped) or one such."""
    m = np.asarray(T, dtype=np.float64)
    if m.ndim >= 2 and m.shape[-2:] == (4, 4):
        m = m[..., :3, :]
    if m.size == 0 or m.size % 12:
        raise ValueError("segment matrices: 12 entries each, at least one")
    return np.ascontiguousarray(m.reshape(-1, 12))


class _SharedEntries:
    """The methods ``HipCtx`` and ``api.Localizer`` share, once; an entry is named by its symbol in libflimo_hip.so (a row of
    ``_abi.PAIRED``).  A class supplies ``_L`` and ``_h`` (library and handle), ``_symbol(entry)`` (the symbol it calls for the
    entry), ``_fail(entry, rc)`` (raise for a non-zero code), ``map_size()`` and ``_scan_size()`` (points of the resident
    scan).  Through a ``Localizer`` every one of them first waits for an insert, a crop or a carve still running behind
    the last sweep (the ``flimo_loc_*`` forwarder does)."""

    def _code(self, entry, *args):
        return getattr(self._L, self._symbol(entry))(self._h, *args)

    def _entry(self, entry, *args):
        rc = self._code(entry, *args)
        if rc != 0:
            self._fail(entry, rc)

    def _range(self, first, n):
        """(first, n) of a range entry; ``n`` None: up to the map's end."""
        first = int(first)
        return first, max(self.map_size() - first, 0) if n is None else int(n)

    def _remove(self, entry, first, n, k, stats):
        """The tail of the entries that forget the points of a range by a cfg: (points removed, stats)."""
        first, n = self._range(first, n)
        removed = C.c_size_t(0)
        self._entry(entry, first, n, C.byref(k), C.byref(removed), C.byref(stats))
        return int(removed.value), stats.as_dict()

    def map_seen_through(self, x26, sensor, want_mask=True, **cfg):
        """The stored points that the resident scan, moved to the world frame by ``x26``, looks through from ``sensor`` (world
        frame) -- flimo_map_seen_through; ``cfg``: the fields of ``carve_cfg``.  Returns (mask [map size] bool in insertion order,
        count); changes nothing.  A ``Localizer`` first waits for an insert, a crop or a carve still running behind the last sweep;
        its resident scan is the last sweep's (``pc2match()``)."""
        x = np.ascontiguousarray(x26, dtype=np.float64).reshape(26)
        s = np.ascontiguousarray(sensor, dtype=np.float32).reshape(3)
        k = carve_cfg(**cfg)
        n = self.map_size()
        mask = np.zeros(n, np.uint8) if want_mask else None
        count = C.c_size_t(0)
        self._entry("flimo_map_seen_through", x.ctypes.data, s.ctypes.data, C.byref(k), _ptr(mask), n, C.byref(count))
        return (mask.astype(bool) if want_mask else None), int(count.value)

    def map_carve(self, x26, sensor, box=None, **cfg) -> int:
        """Forget the stored points the resident scan looks through (``map_seen_through``) and, with ``box`` = (lo, hi), those outside
        it, in one pass -- flimo_map_carve; afterwards the map is as after ``map_crop_box``.  Returns the number of points removed.
        A ``Localizer`` first waits for an insert, a crop or a carve still running behind the last sweep."""
        x = np.ascontiguousarray(x26, dtype=np.float64).reshape(26)
        s = np.ascontiguousarray(sensor, dtype=np.float32).reshape(3)
        k = carve_cfg(**cfg)
        lo = hi = None
        if box is not None:
            lo = np.ascontiguousarray(box[0], dtype=np.float32).reshape(3)
            hi = np.ascontiguousarray(box[1], dtype=np.float32).reshape(3)
        removed = C.c_size_t(0)
        self._entry("flimo_map_carve", x.ctypes.data, s.ctypes.data, C.byref(k), _ptr(lo), _ptr(hi), C.byref(removed))
        return int(removed.value)

    def map_outliers(self, first=0, n=None, want=("mask", "mean_dist", "cnt"), **cfg):
        """The stored points first .. first + n - 1 (``n`` None: up to the map's end) that belong to no surface, by the statistics
        of their k nearest neighbours -- flimo_map_outliers; ``cfg``: the fields of ``outlier_cfg``.  Returns a dict: ``mask`` [n]
        bool, ``mean_dist`` [n] float64, ``cnt`` [n] int32 (those named in ``want``) and ``stats``; changes nothing.  A ``Localizer``
        first waits for an insert, a crop or a carve still running behind the last sweep; no policy of its own calls this."""
        first, n = self._range(first, n)
        out, k, st = _outputs("outliers", _OUTLIER_OUTPUTS, want, n), outlier_cfg(**cfg), OutlierStats()
        self._entry("flimo_map_outliers", first, n, C.byref(k), *_ptrs(out, _OUTLIER_OUTPUTS), C.byref(st))
        return _result(out, st)

    def map_remove_outliers(self, first=0, n=None, **cfg):
        """Forget the outliers of ``map_outliers`` -- flimo_map_remove_outliers; afterwards the map is as after ``map_crop_box``.
        Returns (points removed, stats).  A ``Localizer`` first waits for an insert, a crop or a carve still running."""
        return self._remove("flimo_map_remove_outliers", first, n, outlier_cfg(**cfg), OutlierStats())

    def map_fpfh(self, first=0, n=None, want=("spfh", "cnt"), **cfg):
        """FPFH descriptors (pcl::FPFHEstimation: 33 bins) of the stored points first .. first + n - 1 (``n`` None: up to the map's
        end) -- flimo_map_fpfh; ``cfg``: the fields of ``fpfh_cfg`` (k, max_dist, normal_k, normal_max_dist, normal_min_pts,
        viewpoint).  Returns a dict: ``fpfh`` [n, 33] float32, and of ``want`` ``spfh`` [n, 33] uint8, ``cnt`` [n] int32.  The
        normals and the SPFH rows are formed for the whole map whatever the range; changes nothing.  A ``Localizer`` first waits
        for an insert, a crop or a carve still running behind the last sweep; its own update does not use this."""
        first, n = self._range(first, n)
        out, k = _outputs("fpfh", _FPFH_OUTPUTS, want, n, always=("fpfh",)), fpfh_cfg(**cfg)
        self._entry("flimo_map_fpfh", first, n, C.byref(k), *_ptrs(out, _FPFH_OUTPUTS))
        return out

    def map_keypoints(self, first=0, n=None, want=("saliency", "cnt"), **cfg):
        """ISS keypoints (pcl::ISSKeypoint3D with k-bounded neighbourhoods and broken ties) among the stored points first .. first +
        n - 1 (``n`` None: up to the map's end) -- flimo_map_keypoints; ``cfg``: the fields of ``keypoint_cfg`` (k, max_dist, min_pts,
        gamma21, gamma32, nms_k, nms_max_dist).  Returns a dict: ``mask`` [n] bool, ``count``, ``index`` (the ascending int64 indices of
        the ones, relative to ``first``), and of ``want`` ``saliency`` [n] float64 (NaN: not salient), ``cnt`` [n] int32.  The
        saliency is formed for the whole map whatever the range; changes nothing.  A ``Localizer`` first waits for an insert, a
        crop or a carve still running behind the last sweep; its own update does not use this."""
        first, n = self._range(first, n)
        out, k, count = _outputs("keypoints", _KEYPOINT_OUTPUTS, want, n, always=("mask",)), keypoint_cfg(**cfg), C.c_size_t(0)
        self._entry("flimo_map_keypoints", first, n, C.byref(k), *_ptrs(out, _KEYPOINT_OUTPUTS), C.byref(count))
        out = _result(out)
        out["count"] = int(count.value)
        out["index"] = np.flatnonzero(out["mask"]).astype(np.int64)
        return out

    def map_clusters(self, first=0, n=None, want=("label", "size", "mask"), **cfg):
        """Euclidean clusters (pcl::EuclideanClusterExtraction) of the stored points, for the points first .. first + n - 1 (``n``
        None: up to the map's end) -- flimo_map_clusters; ``cfg``: the fields of ``cluster_cfg`` (tol, min_size, max_size).  Returns a
        dict: of ``want`` ``label`` [n] int32 (the smallest insertion index of the point's component), ``size`` [n] int32, ``mask``
        [n] bool (the component is selected), and ``stats``.  The components are the whole map's whatever the range; changes
        nothing.  ``api.cluster_lists`` turns the labels into PCL's index lists.  A ``Localizer`` first waits for an insert, a crop
        or a carve still running behind the last sweep; no policy of its own calls this."""
        first, n = self._range(first, n)
        out, k, st = _outputs("clusters", _COMPONENT_OUTPUTS, want, n), cluster_cfg(**cfg), ClusterStats()
        self._entry("flimo_map_clusters", first, n, C.byref(k), *_ptrs(out, _COMPONENT_OUTPUTS), C.byref(st))
        return _result(out, st)

    def map_remove_clusters(self, first=0, n=None, **cfg):
        """Forget the points of the range whose ``map_clusters`` mask is set -- flimo_map_remove_clusters; afterwards the map is as
        after ``map_crop_box``.  Returns (points removed, stats).  A ``Localizer`` first waits for an insert, a crop or a carve
        still running."""
        return self._remove("flimo_map_remove_clusters", first, n, cluster_cfg(**cfg), ClusterStats())

    def map_planes(self, tri, want=("plane",), **cfg):
        """RANSAC plane hypotheses over the stored points -- flimo_map_planes.  ``tri`` [nh, 3] int32: the samples, three insertion
        indices each (``api.corr_triplets(map_size, nh, seed)`` draws them); ``cfg``: the fields of ``plane_cfg`` (dist, min_edge,
        min_sin, axis, min_cos).  Returns a dict: ``status`` [nh] (PLANE_OK / PLANE_DEGENERATE / PLANE_REJECTED), ``inliers`` [nh]
        over ALL stored points, ``sum_sq`` [nh] float64 and, named in ``want``, ``plane`` [nh, 4] float64 (nx ny nz d; NaN unless
        OK).  Changes nothing.  ``api.plane_consensus`` samples, calls and ranks.  A ``Localizer`` first waits for an insert, a
        crop or a carve still running behind the last sweep; no policy of its own calls this."""
        unknown = set(want) - {"plane"}
        if unknown:
            raise ValueError(f"map_planes: unknown outputs {sorted(unknown)}")
        t = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        nh = t.shape[0]
        k = plane_cfg(**cfg)
        out = {"status": np.zeros(nh, np.int32), "inliers": np.zeros(nh, np.int32), "sum_sq": np.zeros(nh, np.float64)}
        if "plane" in want:
            out["plane"] = np.full((nh, 4), np.nan)
        self._entry("flimo_map_planes", _ptr(t), nh, C.byref(k), _ptr(out["status"]), _ptr(out["inliers"]), _ptr(out["sum_sq"]),
                    _ptr(out.get("plane")))
        return out

    def map_plane_mask(self, sel=None, first=0, n=None, want_mask=True, **kw):
        """The stored points first .. first + n - 1 against one plane -- flimo_map_plane_mask.  ``sel``: a ``PlaneSel``, or its
        fields as keywords (normal, anchor, dist, side).  Returns (mask [n] bool or None, count).  Changes nothing.  A
        ``Localizer`` first waits for an insert, a crop or a carve still running behind the last sweep."""
        first, n = self._range(first, n)
        sel = _as_plane_sel(sel, kw)
        mask = np.zeros(n, np.uint8) if want_mask else None
        count = C.c_size_t(0)
        self._entry("flimo_map_plane_mask", first, n, C.byref(sel), _ptr(mask), C.byref(count))
        return (mask.astype(bool) if want_mask else None), int(count.value)

    def map_remove_plane(self, sel=None, first=0, n=None, **kw):
        """Forget the points of the range whose ``map_plane_mask`` is set -- flimo_map_remove_plane; afterwards the map is as after
        ``map_crop_box``.  Returns the number of points removed.  A ``Localizer`` first waits for an insert, a crop or a carve
        still running."""
        first, n = self._range(first, n)
        sel = _as_plane_sel(sel, kw)
        removed = C.c_size_t(0)
        self._entry("flimo_map_remove_plane", first, n, C.byref(sel), C.byref(removed))
        return int(removed.value)

    def map_voxels(self, want=("ijk", "count", "centroid"), **cfg):
        """The voxels of the stored points on a lattice anchored at the world origin -- flimo_map_voxels.  ``cfg``: the fields of
        ``voxel_cfg`` (leaf, keep, max_pts).  Returns a dict with the outputs named in ``want`` (of ``ijk`` [nv, 3] = (cx, cy, cz),
        ``count``, ``first``, ``rep`` [nv], ``centroid`` [nv, 3] and ``cov`` [nv, 6] float64: xx xy xz yy yz zz), ``nv`` and
        ``stats``; the voxels in ascending (cz, cy, cx).  Changes nothing.  A ``Localizer`` first waits for an insert, a crop or a
        carve still running behind the last sweep; no policy of its own calls this."""
        cap = self.map_size()      # (no more voxels than points: one call)
        arr, k, nv, st = _outputs("map_voxels", VOXEL_OUTPUTS, want, cap), voxel_cfg(**cfg), C.c_size_t(0), VoxelStats()
        self._entry("flimo_map_voxels", C.byref(k), cap, C.byref(nv), *_ptrs(arr, VOXEL_OUTPUTS), C.byref(st))
        out = _result(arr, rows=nv.value)
        out["nv"] = int(nv.value)
        out["stats"] = st.as_dict()
        return out

    def map_voxel_mask(self, first=0, n=None, want=("voxel", "mask"), **cfg):
        """The voxel and the thinning mask of the stored points first .. first + n - 1 -- flimo_map_voxel_mask: a dict with
        ``voxel`` [n] (the position of the point's voxel in ``map_voxels``' listing, -1 outside the lattice), ``mask`` [n] bool
        (True: ``map_thin`` would forget the point) and ``stats``.  Changes nothing.  A ``Localizer`` first waits for an insert, a
        crop or a carve still running behind the last sweep."""
        first, n = self._range(first, n)
        out, k, st = _outputs("map_voxel_mask", _VOXEL_MASK_OUTPUTS, want, n), voxel_cfg(**cfg), VoxelStats()
        self._entry("flimo_map_voxel_mask", first, n, C.byref(k), *_ptrs(out, _VOXEL_MASK_OUTPUTS), C.byref(st))
        return _result(out, st)

    def map_thin(self, first=0, n=None, **cfg):
        """Forget the points of the range ``map_voxel_mask`` marks -- flimo_map_thin; afterwards the map is as after ``map_crop_box``.
        Returns (removed, stats).  A ``Localizer`` first waits for an insert, a crop or a carve still running."""
        return self._remove("flimo_map_thin", first, n, voxel_cfg(**cfg), VoxelStats())

    def map_regions(self, first=0, n=None, want=("label", "size", "mask"), **cfg):
        """Smooth-surface regions (pcl::RegionGrowing without its seed order) of the stored points, for the points first ..
        first + n - 1 (``n`` None: up to the map's end) -- flimo_map_regions; ``cfg``: the fields of ``region_cfg`` (tol, normal_k,
        normal_max_dist, normal_min_pts, min_cos, max_curv, border, min_size, max_size).  Returns a dict: of ``want`` ``label`` [n]
        int32 (the smallest insertion index of the region's smooth points; -1: no region), ``size`` [n] int32, ``mask`` [n] bool (the
        region is selected), and ``stats``.  The regions are the whole map's whatever the range; changes nothing.  A ``Localizer``
        first waits for an insert, a crop or a carve still running behind the last sweep; no policy of its own calls this."""
        first, n = self._range(first, n)
        out, k, st = _outputs("map_regions", _COMPONENT_OUTPUTS, want, n), region_cfg(**cfg), RegionStats()
        self._entry("flimo_map_regions", first, n, C.byref(k), *_ptrs(out, _COMPONENT_OUTPUTS), C.byref(st))
        return _result(out, st)

    def map_region_list(self, want=("label", "count", "centroid", "cov"), **cfg):
        """The selected regions of the stored points in ascending label -- flimo_map_region_list: a dict with the outputs named in
        ``want`` (of ``label``, ``count``, ``first`` [nr], ``centroid`` [nr, 3] and ``cov`` [nr, 6] float64: xx xy xz yy yz zz, in
        ``map_voxels``' summation shape), ``nr`` and ``stats``.  ``api.region_planes`` fits a plane to each.  Changes nothing.
        Selected regions are few: one call with room for ``REGION_LIST_CAP`` of them, and a second with room for ``nr`` only where
        the first answers FLIMO_ERR_TOO_LARGE.  A ``Localizer`` first waits for an insert, a crop or a carve still running."""
        cap, nr, st = REGION_LIST_CAP, C.c_size_t(0), RegionStats()
        while True:
            arr, k = _outputs("map_region_list", REGION_OUTPUTS, want, cap), region_cfg(**cfg)
            rc = self._code("flimo_map_region_list", C.byref(k), cap, C.byref(nr), *_ptrs(arr, REGION_OUTPUTS), C.byref(st))
            if rc == 0:
                break
            if rc != -5 or nr.value <= cap:      # FLIMO_ERR_TOO_LARGE: *nr says how many there are
                self._fail("flimo_map_region_list", rc)
            cap = int(nr.value)
        out = _result(arr, rows=nr.value)
        out["nr"] = int(nr.value)
        out["stats"] = st.as_dict()
        return out

    def map_remove_regions(self, first=0, n=None, **cfg):
        """Forget the points of the range whose ``map_regions`` mask is set -- flimo_map_remove_regions; afterwards the map is as
        after ``map_crop_box``.  Returns (points removed, stats).  A ``Localizer`` first waits for an insert, a crop or a carve
        still running."""
        return self._remove("flimo_map_remove_regions", first, n, region_cfg(**cfg), RegionStats())

    # (HipCtx.knn_k, Localizer.map_knn)
    def _knn_k(self, q, k, max_dist=float("inf"), want_xyz=False):
        """flimo_knn_k (Octree::knn for any k up to 64, with a distance gate): per query the first ``k`` stored points in the order
        (float32 squared-distance bits, insertion index) among those with squared distance < max_dist * max_dist (``inf``: no gate).
        Returns (idx [nq, k], sqd [nq, k], cnt [nq][, xyz [nq, k, 3]]); idx = insertion indices (rows of ``map_points()``), slots
        beyond cnt are idx -1, sqd 0, xyz 0.  A ``Localizer`` first waits for an insert, a crop or a carve still running behind the
        last sweep; changes nothing."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        nq, kk = q.shape[0], max(int(k), 1)
        idx = np.empty((nq, kk), np.int32)
        sqd = np.empty((nq, kk), np.float32)
        cnt = np.empty((nq,), np.int32)
        xyz = np.empty((nq, kk, 3), np.float32) if want_xyz else None
        self._entry("flimo_knn_k", q.ctypes.data if nq else None, nq, int(k), float(max_dist), _ptr(idx), _ptr(sqd), _ptr(xyz), _ptr(cnt))
        return (idx, sqd, cnt, xyz) if want_xyz else (idx, sqd, cnt)

    # (HipCtx.radius_search, Localizer.map_radius_search)
    def _radius_search(self, q, radius, sorted=False, want_xyz=False):
        """flimo_radius_search (Octree::radiusSearch for a batch): the stored points with squared float32 distance < radius * radius.
        Returns (offsets [nq + 1], idx, sqd[, xyz]) in CSR form; idx = insertion indices (rows of ``map_points()``).  Unsorted: an
        order that only a change of the map changes; ``sorted``: ascending by (distance bits, index).  A ``Localizer`` first waits
        for an insert, a crop or a carve still running behind the last sweep; changes nothing."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        nq = q.shape[0]
        off = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        # count, then size the arrays, then fill
        self._entry("flimo_radius_search", q.ctypes.data, nq, float(radius), 0, off.ctypes.data, None, None, None, 0, C.byref(total))
        n = int(total.value)
        idx = np.empty(n, np.int32)
        sqd = np.empty(n, np.float32)
        xyz = np.empty((n, 3), np.float32) if want_xyz else None
        if n > 0:
            self._entry("flimo_radius_search", q.ctypes.data, nq, float(radius), RADIUS_SORTED if sorted else 0, off.ctypes.data,
                        idx.ctypes.data, sqd.ctypes.data, xyz.ctypes.data if want_xyz else None, n, C.byref(total))
        return (off, idx, sqd, xyz) if want_xyz else (off, idx, sqd)

    def _normals_of(self, entry, head, nq, k, max_dist, min_pts, viewpoint, want):
        out = _outputs("normals", _NORMAL_OUTPUTS, want, nq, always=("normal", "cnt"))
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float32).reshape(3)
        self._entry(entry, *head, int(k), float(max_dist), int(min_pts), _ptr(vp), *_ptrs(out, _NORMAL_OUTPUTS))
        return out

    # (HipCtx.normals, Localizer.map_normals)
    def _normals(self, q, k, max_dist=float("inf"), min_pts=3, viewpoint=None, want=("centroid", "cov", "eig")):
        """flimo_map_normals: plane normal and curvature of the neighbourhood ``knn_k(q, k, max_dist)`` of every query, computed on
        the GPU in float64 (mean and covariance of p - q, divided by n; Jacobi eigen-decomposition).  Returns a dict: ``normal``
        [nq, 4] float32 (nx ny nz curvature), ``cnt`` [nq], and of ``want`` ``centroid`` [nq, 3], ``cov`` [nq, 6] (xx xy xz yy yz zz),
        ``eig`` [nq, 6] (l0 <= l1 <= l2, the float64 normal).  ``viewpoint``: the normals face it; None: the component of largest
        magnitude is positive.  Fewer than max(3, min_pts) neighbours: NaN.  A ``Localizer`` first waits for an insert, a crop or a
        carve still running behind the last sweep; changes nothing."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        return self._normals_of("flimo_map_normals", (q.ctypes.data if q.shape[0] else None, q.shape[0]), q.shape[0], k, max_dist, min_pts,
                                viewpoint, want)

    # (HipCtx.normals_range, Localizer.map_normals_range)
    def _normals_range(self, first, n, k, max_dist=float("inf"), min_pts=3, viewpoint=None, want=("centroid", "cov", "eig")):
        """flimo_map_normals_range: ``normals`` of the stored points first .. first + n - 1 themselves (rows of ``map_points()``);
        nothing is uploaded, the bits are those of ``normals(map_points()[first:first + n], ...)``.  A ``Localizer`` first waits
        for an insert, a crop or a carve still running behind the last sweep."""
        return self._normals_of("flimo_map_normals_range", (int(first), int(n)), int(n), k, max_dist, min_pts, viewpoint, want)

    def scan_fitness(self, x26s, max_dist=float("inf"), want_nn=False):
        """flimo_scan_fitness: how well the resident scan fits the map at each pose of ``x26s`` [np, 26] (only pos and rot are read).
        Per pose the nearest stored point of every scan point moved by it (``scan_to_world`` + ``knn_k(k=1, max_dist)``, on the GPU):
        returns (inliers [np] int32: points that have one within the gate, sum_sqd [np] float64: the sum of their squared distances
        [, nn_sqd [np, n] float32: the distance or -1, nn_idx [np, n]: the stored point's insertion index or -1]).  A ``Localizer``
        first waits for an insert, a crop or a carve still running behind the last sweep; its resident scan is that sweep's
        (``pc2match()``)."""
        x = _poses(x26s)
        m, n = x.shape[0], self._scan_size()
        inliers = np.zeros(m, np.int32)
        sum_sqd = np.zeros(m, np.float64)
        nn_sqd = np.full((m, n), -1, np.float32) if want_nn else None
        nn_idx = np.full((m, n), -1, np.int32) if want_nn else None
        self._entry("flimo_scan_fitness", x.ctypes.data if m else None, m, float(max_dist), _ptr(inliers), _ptr(sum_sqd), _ptr(nn_sqd),
                    _ptr(nn_idx))
        return (inliers, sum_sqd, nn_sqd, nn_idx) if want_nn else (inliers, sum_sqd)

    def scan_linearize(self, x26s, k, max_dist, min_pts=3, max_curv=float("inf"), want_rows=False):
        """flimo_scan_linearize: the point-to-plane normal equations of the resident scan against the map at each pose of ``x26s``
        [np, 26] (only pos and rot are read).  Per pose and scan point the plane of ``normals(scan_to_world(x26), k, max_dist,
        min_pts)``, gated by ``max_curv``; returns a dict: valid [np] int32, H [np, 21] (upper triangle, row-major), g [np, 6],
        cost [np][, rows [np, n, 7]: J0..J5, d per pair, NaN when invalid; pair_cnt [np, n]].  The step solves H xi = -g
        (``api.scan_align`` iterates it).  A ``Localizer`` first waits for an insert, a crop or a carve still running behind the
        last sweep; its resident scan is that sweep's (``pc2match()``)."""
        x = _poses(x26s)
        m, n = x.shape[0], self._scan_size()
        out = {"valid": np.zeros(m, np.int32), "H": np.zeros((m, 21)), "g": np.zeros((m, 6)), "cost": np.zeros(m)}
        if want_rows:
            out["rows"] = np.full((m, n, 7), np.nan)
            out["pair_cnt"] = np.zeros((m, n), np.int32)
        self._entry("flimo_scan_linearize", x.ctypes.data if m else None, m, int(k), float(max_dist), int(min_pts), float(max_curv),
                    *(_ptr(out.get(name)) for name in ("valid", "H", "g", "cost", "rows", "pair_cnt")))
        return out

    def ndt_build(self, slot, leaf, min_pts=6, eig_ratio=0.01):
        """flimo_ndt_build: the NDT cell model of slot ``slot`` (0 .. NDT_SLOTS - 1) from the voxels of the whole map at ``leaf``
        -- the voxels of ``map_voxels`` with at least ``min_pts`` points and a covariance that is not zero, their principal axes and
        the weights 1 / max(l, eig_ratio * l2).  A snapshot: later inserts and removals leave it alone (``ndt_info``: stale).
        Returns the number of cells.  A ``Localizer`` first waits for an insert, a crop or a carve still running behind the last
        sweep."""
        k, nc = NdtCfg(float(leaf), int(min_pts), float(eig_ratio)), C.c_size_t(0)
        self._entry("flimo_ndt_build", int(slot), C.byref(k), C.byref(nc))
        return int(nc.value)

    def ndt_info(self, slot):
        """flimo_ndt_info: a dict of the model in ``slot``: cells, map_size_at_build, eig_ratio, leaf, min_pts, stale."""
        info = NdtInfo()
        self._entry("flimo_ndt_info", int(slot), C.byref(info))
        return info.as_dict()

    def ndt_cells(self, slot, want=("ijk", "count", "mean", "evec", "wgt", "eval")):
        """flimo_ndt_cells: the model in ``slot`` as a dict of the arrays named in ``want`` -- ijk [nc, 3] = (cx, cy, cz), count
        [nc], mean [nc, 3], evec [nc, 3, 3] (row k: the unit vector of eigenvalue k), wgt [nc, 3], eval [nc, 3] (ascending, before
        the clamp) -- and ``nc``; the cells in ascending (cz, cy, cx)."""
        nc = C.c_size_t(0)
        self._entry("flimo_ndt_cells", int(slot), 0, C.byref(nc), None, None, None, None, None, None)
        n = int(nc.value)
        arr = _outputs("ndt_cells", NDT_CELL_OUTPUTS, want, n)
        if arr and n:
            self._entry("flimo_ndt_cells", int(slot), n, C.byref(nc), *_ptrs(arr, NDT_CELL_OUTPUTS))
        if "evec" in arr:
            arr["evec"] = arr["evec"].reshape(n, 3, 3)
        out = dict(arr)
        out["nc"] = n
        return out

    def ndt_clear(self, slot=-1):
        """flimo_ndt_clear: free the model in ``slot``; -1: all of them."""
        self._entry("flimo_ndt_clear", int(slot))

    def scan_ndt(self, slot, x26s, d2, hood=7, want_terms=False):
        """flimo_scan_ndt: the NDT score and Gauss-Newton normal equations of the resident scan against the model in ``slot`` at
        each pose of ``x26s`` [np, 26] (only pos and rot are read).  ``hood``: 1 (the point's own cell) or 7 (and its six face
        neighbours); ``d2``: the Gaussian's scale (``api.ndt_params``).  Returns a dict: valid [np] int32 (pairs with a live term),
        cells [np] int64 (live terms), H [np, 21] (upper triangle, row-major), g [np, 6], score [np] (the sum of e)[, terms
        [np, n, 7, 2]: (m, e) per neighbour slot, NaN when absent; term_cell [np, n, 7]: the cell's row in ``ndt_cells``, -1].
        The step solves H xi = -g (``api.ndt_align`` iterates it).  A ``Localizer`` first waits for an insert, a crop or a carve
        still running behind the last sweep; its resident scan is that sweep's (``pc2match()``)."""
        x = _poses(x26s)
        m, n = x.shape[0], self._scan_size()
        out = {"valid": np.zeros(m, np.int32), "cells": np.zeros(m, np.int64), "H": np.zeros((m, 21)), "g": np.zeros((m, 6)),
               "score": np.zeros(m)}
        if want_terms:
            out["terms"] = np.full((m, n, 7, 2), np.nan)
            out["term_cell"] = np.full((m, n, 7), -1, np.int32)
        self._entry("flimo_scan_ndt", int(slot), x.ctypes.data if m else None, m, int(hood), float(d2),
                    *(_ptr(out.get(name)) for name in ("valid", "cells", "H", "g", "score", "terms", "term_cell")))
        return out

    def gicp_build(self, k=20, max_dist=float("inf"), min_pts=3, rule=GICP_PLANE, eps=1e-3):
        """flimo_gicp_build: the GICP model of the context -- per stored point the covariance of ``normals_range(0, map_size(), k,
        max_dist, min_pts)`` (bit for bit, left on the device), regularised by ``rule``: GICP_PLANE (eigenvalues eps, 1, 1: PCL's)
        or GICP_CLAMP (none below eps * l2: the NDT model's).  A snapshot by insertion index: once the stored points change it is
        stale and ``scan_gicp`` refuses it.  Returns the number of points that got a covariance.  A ``Localizer`` first waits for
        an insert, a crop or a carve still running behind the last sweep."""
        cfg, n_cov = GicpCfg(int(k), float(max_dist), int(min_pts), int(rule), float(eps)), C.c_size_t(0)
        self._entry("flimo_gicp_build", C.byref(cfg), C.byref(n_cov))
        return int(n_cov.value)

    def gicp_info(self):
        """flimo_gicp_info: a dict of the model: points, n_cov, eps, k, max_dist, min_pts, rule, stale."""
        info = GicpInfo()
        self._entry("flimo_gicp_info", C.byref(info))
        return info.as_dict()

    def gicp_model(self, first=0, n=None):
        """flimo_gicp_model: rows first .. first + n - 1 of the model (``n`` None: to its end) as float64 [n, 6] = xx xy xz yy yz
        zz; six NaN for a point without a covariance."""
        first = int(first)
        if n is None:
            n = max(self.gicp_info()["points"] - first, 0)
        cov = np.zeros((int(n), 6))
        self._entry("flimo_gicp_model", first, int(n), _ptr(cov))
        return cov

    def gicp_clear(self):
        """flimo_gicp_clear: free the model."""
        self._entry("flimo_gicp_clear")

    def scan_cov_set(self, cov6):
        """flimo_scan_cov_set: one regularised covariance per point of the resident scan, float64 [n, 6], body frame, the scan's
        order (``api.gicp_covs`` computes them); a row with a NaN: that point has none.  None or no row drops them, and so does
        every call that replaces the resident scan."""
        if cov6 is None:
            self._entry("flimo_scan_cov_set", None, 0)
            return
        cov = np.ascontiguousarray(cov6, dtype=np.float64).reshape(-1, 6)
        self._entry("flimo_scan_cov_set", cov.ctypes.data if cov.shape[0] else None, cov.shape[0])

    def scan_gicp(self, x26s, max_dist=1.0, want_pairs=False):
        """flimo_scan_gicp: the GICP (plane-to-plane) normal equations of the resident scan against the map at each pose of
        ``x26s`` [np, 26] (only pos and rot are read): per pair the nearest stored point of ``scan_fitness(max_dist)``, weighed by
        (CB + R CA R^T)^-1 from the model's row (``gicp_build``) and the scan's (``scan_cov_set``).  Returns a dict: valid [np]
        int32, H [np, 21] (upper triangle, row-major), g [np, 6], cost [np] (the sum of m)[, pair_idx [np, n]: the neighbour or -1;
        pair_m [np, n]: m, NaN for an invalid pair].  The step solves H xi = -g (``api.gicp_align`` iterates it).  A ``Localizer``
        first waits for an insert, a crop or a carve still running behind the last sweep."""
        x = _poses(x26s)
        m, n = x.shape[0], self._scan_size()
        out = {"valid": np.zeros(m, np.int32), "H": np.zeros((m, 21)), "g": np.zeros((m, 6)), "cost": np.zeros(m)}
        if want_pairs:
            out["pair_idx"] = np.full((m, n), -1, np.int32)
            out["pair_m"] = np.full((m, n), np.nan)
        self._entry("flimo_scan_gicp", x.ctypes.data if m else None, m, float(max_dist),
                    *(_ptr(out.get(name)) for name in ("valid", "H", "g", "cost", "pair_idx", "pair_m")))
        return out

    def set_gicp_chunk(self, pairs):
        """(pose, point) pairs per chunk of ``scan_gicp`` (flimo_set_gicp_chunk; 0: the default of 2^20), on the map's context."""
        hip = getattr(self, "hip", self)
        hip._chk(hip._L.flimo_set_gicp_chunk(hip._h, int(pairs)))

    def scan_cov_size(self) -> int:
        """flimo_scan_cov_size: the covariances ``scan_cov_set`` left with the resident scan, 0 when there are none."""
        hip = getattr(self, "hip", self)
        return int(hip._L.flimo_scan_cov_size(hip._h))

    def corr_poses(self, src, dst, tri, want=("pose",), **cfg):
        """flimo_corr_poses: pose hypotheses from point correspondences.  ``src`` [m, 3] (body frame) and ``dst`` [m, 3] (map frame)
        are the putative pairs, ``tri`` [nh, 3] the caller's samples of three of them (``api.corr_triplets``); ``cfg``: the fields
        of ``corr_cfg``.  Per sample the polygon pre-rejection, the closed-form pose and the pairs it brings within ``max_dist``.
        Returns a dict: status [nh] (CORR_OK / CORR_DEGENERATE / CORR_REJECTED), inliers [nh] int32, sum_sqd [nh] float64[, pose
        [nh, 7]: t, then the quaternion x y z w -- the first seven entries of an x26 row; NaN unless OK][, pair_sqd [nh, m] float32:
        the squared distance of an inlier pair, -1 otherwise].  Reads neither the map nor the resident scan.  A ``Localizer`` runs
        it on the map's context and first waits for an insert, a crop or a carve still running behind the last sweep."""
        unknown = set(want) - {"pose", "pair_sqd"}
        if unknown:
            raise ValueError(f"corr_poses: unknown outputs {sorted(unknown)}")
        s, d = _pairs("corr_poses", src, dst)
        t = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        m, nh = s.shape[0], t.shape[0]
        k = corr_cfg(**cfg)
        out = {"status": np.zeros(nh, np.int32), "inliers": np.zeros(nh, np.int32), "sum_sqd": np.zeros(nh, np.float64)}
        if "pose" in want:
            out["pose"] = np.full((nh, 7), np.nan)
        if "pair_sqd" in want:
            out["pair_sqd"] = np.full((nh, m), -1, np.float32)
        self._entry("flimo_corr_poses", _ptr(s), _ptr(d), m, _ptr(t), nh, C.byref(k),
                    *(_ptr(out.get(name)) for name in ("status", "inliers", "sum_sqd", "pose", "pair_sqd")))
        return out

    def corr_graph(self, src, dst, want=(), **cfg):
        """flimo_corr_graph: which of the putative pairs ``src`` [m, 3] / ``dst`` [m, 3] can be true together.  Pairs i and j are
        joined when the edge between them is as long in ``src`` as in ``dst`` to within ``tol`` (``cfg``: the fields of
        ``corr_graph_cfg``).  Returns a dict: degree [m] int32, core [m] int32 (the core numbers of that graph), max_core[, adj
        [m, (m + 63) // 64] uint64 when "adj" is in ``want``: bit j & 63 of word j >> 6 of row i].  m at most CORR_GRAPH_MAX_M.
        Reads neither the map nor the resident scan.  A ``Localizer`` runs it on the map's context and first waits for an insert,
        a crop or a carve still running behind the last sweep."""
        unknown = set(want) - {"adj"}
        if unknown:
            raise ValueError(f"corr_graph: unknown outputs {sorted(unknown)}")
        s, d = _pairs("corr_graph", src, dst)
        m = s.shape[0]
        k = corr_graph_cfg(**cfg)
        out = {"degree": np.zeros(m, np.int32), "core": np.zeros(m, np.int32)}
        if "adj" in want:
            out["adj"] = np.zeros((m, (m + 63) // 64), np.uint64)
        top = C.c_int32(0)
        self._entry("flimo_corr_graph", _ptr(s), _ptr(d), m, C.byref(k), _ptr(out["degree"]), _ptr(out["core"]), C.byref(top),
                    _ptr(out.get("adj")))
        out["max_core"] = int(top.value)
        return out

    def desc_ref_set(self, desc):
        """flimo_desc_ref_set: ``desc`` [nr, dim] float32 becomes the context's resident reference set of ``desc_match`` (the map's
        descriptors: set once, matched against many times); it replaces the previous one, no rows clear it.  A ``Localizer`` keeps
        it on the map's context and first waits for an insert, a crop or a carve still running behind the last sweep."""
        d = desc_rows(desc)
        self._entry("flimo_desc_ref_set", d.ctypes.data if d.size else None, d.shape[0], d.shape[1] if d.shape[0] else 0)

    def desc_match(self, q, k=2):
        """flimo_desc_match: per row of ``q`` [nq, dim] the first ``k`` rows of the resident reference set by (bits of the float32
        squared distance, index) -- the distance is include/flimo_c.h's fmaf chain, exact and reproducible.  Returns a dict: idx
        [nq, k] int32 (-1 beyond cnt), dist [nq, k] float32 (0 beyond cnt), cnt [nq].  Rows with a non-finite entry never match.  A
        ``Localizer`` first waits for an insert, a crop or a carve still running behind the last sweep."""
        q = desc_rows(q)
        nq, kk = q.shape[0], max(int(k), 1)
        out = {"idx": np.full((nq, kk), -1, np.int32), "dist": np.zeros((nq, kk), np.float32), "cnt": np.zeros(nq, np.int32)}
        self._entry("flimo_desc_match", _ptr(q), nq, q.shape[1], int(k), _ptr(out["idx"]), _ptr(out["dist"]), _ptr(out["cnt"]))
        return out

    def scan_context(self, cfg=None, frame12=None, **kw):
        """flimo_scan_context: the Scan Context descriptor of the resident scan -- per (ring, sector) bin of the sensor's polar
        grid the largest height of a point in it.  ``cfg``: a ``ScCfg`` or None with the fields of ``sc_cfg`` as keywords;
        ``frame12``: None or a row-major 3 x 4 transform applied to every point first (lidar to base, gravity alignment).  Returns
        (desc [rings, sectors] float32, used: the points that have a bin).  A pending deskew runs first; changes nothing.  A
        ``Localizer`` first waits for an insert, a crop or a carve still running behind the last sweep."""
        k, f = _as_sc_cfg(cfg, kw), _frame12(frame12)
        desc, used = np.zeros((max(k.rings, 0), max(k.sectors, 0)), np.float32), C.c_int32(0)
        self._entry("flimo_scan_context", C.byref(k), _ptr(f), _ptr(desc), C.byref(used))
        return desc, int(used.value)

    def sc_db_add(self, desc):
        """flimo_sc_db_add: append ``desc`` [n, rings, sectors] (or one [rings, sectors]) to the context's resident Scan Context
        database; returns the id of the first (ids count up from 0 in the order added).  The database's shape is that of its first
        entry after a clear; it is independent of the map and of the scan."""
        d = sc_rows(desc)
        first = C.c_size_t(0)
        self._entry("flimo_sc_db_add", _ptr(d), d.shape[0], d.shape[1], d.shape[2], C.byref(first))
        return int(first.value)

    def sc_db_add_scan(self, cfg=None, frame12=None, **kw):
        """flimo_sc_db_add_scan: append ``scan_context``'s descriptor of the resident scan without a round trip; returns its id."""
        k, f, at = _as_sc_cfg(cfg, kw), _frame12(frame12), C.c_size_t(0)
        self._entry("flimo_sc_db_add_scan", C.byref(k), _ptr(f), C.byref(at))
        return int(at.value)

    def sc_db_get(self, first=0, n=None):
        """flimo_sc_db_get: the raw rows of the entries first .. first + n - 1 (``n`` None: to the end) as float32 [n, rings,
        sectors]."""
        hip = getattr(self, "hip", self)
        first, size = int(first), hip.sc_db_size()
        n = max(size - first, 0) if n is None else int(n)
        rings, sectors = hip.sc_db_shape()
        out = np.zeros((n, rings, sectors), np.float32)
        self._entry("flimo_sc_db_get", first, n, _ptr(out))
        return out

    def sc_db_clear(self):
        """flimo_sc_db_clear: forget every entry; the next add sets the shape."""
        self._entry("flimo_sc_db_clear")

    def sc_match(self, q, k=1, min_cols=1, max_dist=float("inf"), first=0, n=None, want_profile=False):
        """flimo_sc_match: per descriptor of ``q`` [nq, rings, sectors] (or one [rings, sectors]) the first ``k`` entries with ids
        in [first, first + n) (``n`` None: to the end) by (bits of the float32 distance, id), the distance the smallest over every
        column shift of 1 - mean cosine of the columns valid in both (at least ``min_cols`` of them), below ``max_dist``.  Returns a
        dict: idx [nq, k] int32 (-1 beyond cnt), dist [nq, k] float32, shift [nq, k] int32 (yaw_query = yaw_entry - shift * 2 pi /
        sectors), cnt [nq][, profile [nq, k, sectors]: the distance at every shift, NaN where excluded].  Exact and reproducible.
        A ``Localizer`` first waits for an insert, a crop or a carve still running behind the last sweep."""
        q = sc_rows(q)
        nq, kk = q.shape[0], max(int(k), 1)
        cfg = ScMatchCfg(int(k), int(min_cols), float(max_dist))
        out = {"idx": np.full((nq, kk), -1, np.int32), "dist": np.zeros((nq, kk), np.float32), "shift": np.full((nq, kk), -1, np.int32),
               "cnt": np.zeros(nq, np.int32)}
        if want_profile:
            out["profile"] = np.full((nq, kk, q.shape[2]), np.nan, np.float32)
        self._entry("flimo_sc_match", _ptr(q), nq, q.shape[1], q.shape[2], int(first), (1 << 62) if n is None else int(n), C.byref(cfg),
                    *(_ptr(out.get(name)) for name in ("idx", "dist", "shift", "cnt", "profile")))
        return out

    def map_segment_mark(self) -> int:
        """flimo_map_segment_mark: close the open segment of the stored points at the current size and open a new one; returns the
        new segment's number.  A segment is a run of insertion indices -- a stretch of the drive; the caller marks segment s right
        before keyframe s's first insert.  FlimoError while the table is stale (``map_segments``).  A ``Localizer`` first waits for
        an insert, a crop or a carve still running behind the last sweep, so the mark lands behind that sweep's points."""
        at = C.c_size_t(0)
        self._entry("flimo_map_segment_mark", C.byref(at))
        return int(at.value)

    def map_segments(self):
        """flimo_map_segments: (begin [S + 1] uint64, stale) -- segment s is the insertion indices [begin[s], begin[s + 1]),
        begin[S] the map's size.  Stale after a removal other than ``map_remove_range`` that removed a point, until
        ``map_segments_reset`` or ``map_clear``."""
        n_seg, stale = C.c_size_t(0), C.c_int(0)
        self._entry("flimo_map_segments", None, 0, C.byref(n_seg), C.byref(stale))
        begin = np.zeros(int(n_seg.value) + 1, np.uint64)
        self._entry("flimo_map_segments", _ptr(begin), begin.size, C.byref(n_seg), C.byref(stale))
        return begin, bool(stale.value)

    def map_segments_reset(self):
        """flimo_map_segments_reset: one segment over every stored point, not stale."""
        self._entry("flimo_map_segments_reset")

    def map_corrected(self, T, first=0, n=None, want_xyz=True):
        """flimo_map_corrected: where the stored points first .. first + n - 1 (``n`` None: up to the map's end) would go under
        ``map_correct(T)``; ``T`` [S, 12] (or [S, 3, 4]) float64.  Returns (xyz [n, 3] float32 or None, changed: how many have
        different bits afterwards); changes nothing."""
        m = seg_mats(T)
        first, n = self._range(first, n)
        xyz, changed = (np.zeros((n, 3), np.float32) if want_xyz else None), C.c_size_t(0)
        self._entry("flimo_map_corrected", _ptr(m), m.shape[0], first, n, _ptr(xyz), C.byref(changed))
        return xyz, int(changed.value)

    def map_correct(self, T) -> int:
        """flimo_map_correct: move every stored point by its segment's matrix -- ``T`` [S, 12] (or [S, 3, 4]) float64, row-major
        3 x 4, new world <- old world (``api.segment_corrections``) -- and rebuild the index once; returns how many points changed
        bits (0: nothing happened at all).  Size, insertion indices, the segment table and the time of the last insert stay; models
        built from the old positions are stale afterwards.  A ``Localizer``'s filter pose is the caller's to set (``set_x``)."""
        m, changed = seg_mats(T), C.c_size_t(0)
        self._entry("flimo_map_correct", _ptr(m), m.shape[0], C.byref(changed))
        return int(changed.value)

    def map_transform(self, T) -> int:
        """flimo_map_transform: ``map_correct`` with the one matrix ``T`` (12 entries, row-major 3 x 4) for every stored point; does
        not read the segment table.  Returns how many points changed bits."""
        m, changed = seg_mats(T), C.c_size_t(0)
        if m.shape[0] != 1:
            raise ValueError("map_transform: one 3 x 4 matrix")
        self._entry("flimo_map_transform", _ptr(m), C.byref(changed))
        return int(changed.value)

    def map_remove_range(self, first, n=None) -> int:
        """flimo_map_remove_range: forget the stored points first .. first + n - 1 (``n`` None: up to the map's end; cut to the
        size) -- forgetting by age; afterwards the map is as after ``map_crop_box`` and the segment table has followed exactly.
        Returns the number of points removed."""
        removed = C.c_size_t(0)
        self._entry("flimo_map_remove_range", int(first), (1 << 62) if n is None else int(n), C.byref(removed))
        return int(removed.value)

    def set_segment_plan(self, slab=0, blocks=0):
        """The launch of ``map_correct`` / ``map_transform`` / ``map_corrected`` (flimo_set_segment_plan, include/flimo_dev.h), on
        the map's context; no result depends on it."""
        hip = getattr(self, "hip", self)
        hip._chk(hip._L.flimo_set_segment_plan(hip._h, int(slab), int(blocks)))


class HipCtx(_SharedEntries):
    """Thin OO wrapper over one ``flimo_ctx`` (one GPU, one map, one stream)."""
    knn_k, radius_search = _SharedEntries._knn_k, _SharedEntries._radius_search
    normals, normals_range = _SharedEntries._normals, _SharedEntries._normals_range

    def __init__(self, device: int = 0):
        L = load_hip()
        h = C.c_void_p()
        rc = L.flimo_ctx_create(device, C.byref(h))
        if rc != 0:
            raise FlimoError(f"flimo_ctx_create({device}) failed: {_ERRS.get(rc, rc)}")
        self._h = h
        self._L = L

    def close(self):
        if getattr(self, "_h", None):
            self._L.flimo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise FlimoError(f"{_ERRS.get(rc, rc)}: {self._L.flimo_last_error(self._h).decode()}")

    def _symbol(self, entry):
        return entry

    def _fail(self, entry, rc):
        self._chk(rc)

    def _scan_size(self):
        return self.scan_size()

    # ---- map ----
    def map_config(self, min_extent=0.2, bucket_size=2, downsample=True, cell_size=0.0):
        cfg = MapCfg(min_extent, bucket_size, int(downsample), cell_size)
        self._chk(self._L.flimo_map_config(self._h, C.byref(cfg)))

    def map_add(self, xyz, stamp=0.0):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n = xyz.shape[0]
        stride = xyz.strides[0] if xyz.ndim == 2 else 12
        self._chk(self._L.flimo_map_add(self._h, xyz.reshape(-1), n, stride, float(stamp)))

    def map_clear(self):
        self._chk(self._L.flimo_map_clear(self._h))

    def map_crop_box(self, lo, hi) -> int:
        """Forget the stored points outside [lo, hi] (inclusive); the map is then clear() + initialize(kept points, in insertion
        order).  Returns the number of points removed."""
        lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(3)
        hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(3)
        removed = C.c_size_t(0)
        self._chk(self._L.flimo_map_crop_box(self._h, lo.ctypes.data, hi.ctypes.data, C.byref(removed)))
        return int(removed.value)

    def map_crop_stats(self):
        o = (C.c_uint64 * 2)()
        self._chk(self._L.flimo_map_crop_stats(self._h, o))
        return dict(crops=int(o[0]), points_removed=int(o[1]))

    def map_carve_stats(self):
        o = (C.c_uint64 * 2)()
        self._chk(self._L.flimo_map_carve_stats(self._h, o))
        return dict(carves=int(o[0]), points_removed=int(o[1]))

    def set_outlier_chunk(self, n):
        """Points per search launch of ``map_outliers`` / ``map_remove_outliers`` (flimo_set_outlier_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_outlier_chunk(self._h, int(n)))

    def set_fpfh_chunk(self, n):
        """Points per search launch of ``map_fpfh`` (flimo_set_fpfh_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_fpfh_chunk(self._h, int(n)))

    def set_keypoints_chunk(self, n):
        """Points per search launch of ``map_keypoints`` (flimo_set_keypoints_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_keypoints_chunk(self._h, int(n)))

    def set_cluster_chunk(self, n):
        """Points per link launch of ``map_clusters`` / ``map_remove_clusters`` (flimo_set_cluster_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_cluster_chunk(self._h, int(n)))

    def set_plane_chunk(self, n):
        """Hypotheses per chunk of ``map_planes`` (flimo_set_plane_chunk; 0: the default of 2^10)."""
        self._chk(self._L.flimo_set_plane_chunk(self._h, int(n)))

    def set_voxel_plan(self, plan):
        """The lane plan of ``map_voxels``' moments (flimo_set_voxel_plan; 0: by the voxel's count, 1..3: groups of 8, 16, 64 lanes,
        4: the many-runs path, + 8: the points written in sorted order first)."""
        self._chk(self._L.flimo_set_voxel_plan(self._h, int(plan)))

    def set_region_chunk(self, n):
        """Points per link launch of ``map_regions`` / ``map_region_list`` / ``map_remove_regions`` (flimo_set_region_chunk; 0: the
        default of 2^20)."""
        self._chk(self._L.flimo_set_region_chunk(self._h, int(n)))

    def map_size(self) -> int:
        return int(self._L.flimo_map_size(self._h))

    def map_points(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._chk(self._L.flimo_map_points(self._h, None, 0, C.byref(n)))
        out = np.empty((max(n.value, 1), 3), dtype=np.float32)
        self._chk(self._L.flimo_map_points(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def knn(self, q, k=5):
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        nq = q.shape[0]
        idx = np.empty((nq, k), np.int32)
        sqd = np.empty((nq, k), np.float32)
        cnt = np.empty((nq,), np.int32)
        self._chk(self._L.flimo_knn(self._h, q.reshape(-1), nq, k, idx.reshape(-1), sqd.reshape(-1), cnt))
        return idx, sqd, cnt

    def set_normals_chunk(self, n):
        """Queries per launch of ``normals`` / ``normals_range`` (flimo_set_normals_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_normals_chunk(self._h, int(n)))

    def knn_k_candidates(self, q, k, max_dist=float("inf")):
        """Stored points each query's search loads and tests (flimo_knn_k_candidates, include/flimo_dev.h)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        cand = np.zeros(q.shape[0], np.uint64)
        self._chk(self._L.flimo_knn_k_candidates(self._h, q.ctypes.data, q.shape[0], int(k), float(max_dist), cand.ctypes.data))
        return cand

    def radius_count(self, q, radius):
        """Results per query of ``radius_search`` (count only: nothing but the offsets comes back)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        off = np.zeros(q.shape[0] + 1, np.uint64)
        self._chk(self._L.flimo_radius_search(self._h, q.ctypes.data, q.shape[0], float(radius), 0, off.ctypes.data, None, None, None, 0, None))
        return np.diff(off).astype(np.int64)

    def radius_candidates(self, q, radius):
        """Stored points each query's walk loads and tests at this radius (flimo_radius_candidates, include/flimo_dev.h)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
        cand = np.zeros(q.shape[0], np.uint64)
        self._chk(self._L.flimo_radius_candidates(self._h, q.reshape(-1), q.shape[0], float(radius), cand.ctypes.data))
        return cand

    # ---- scan ----
    def scan_set(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n = xyz.shape[0]
        stride = xyz.strides[0] if xyz.ndim == 2 else 12
        self._chk(self._L.flimo_scan_set(self._h, xyz.reshape(-1), n, stride))

    def scan_size(self) -> int:
        return int(self._L.flimo_scan_size(self._h))

    def scan_get(self) -> np.ndarray:
        n = self.scan_size()
        out = np.empty((max(n, 1), 3), dtype=np.float32)
        m = C.c_size_t(0)
        self._chk(self._L.flimo_scan_get(self._h, out.ctypes.data, n, C.byref(m)))
        return out[:n]

    def set_fitness_chunk(self, pairs):
        """(pose, point) pairs per chunk of ``scan_fitness`` (flimo_set_fitness_chunk; 0: the default of 2^22)."""
        self._chk(self._L.flimo_set_fitness_chunk(self._h, int(pairs)))

    def set_linearize_chunk(self, pairs):
        """(pose, point) pairs per chunk of ``scan_linearize`` (flimo_set_linearize_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_linearize_chunk(self._h, int(pairs)))

    def set_ndt_chunk(self, pairs):
        """(pose, point) pairs per chunk of ``scan_ndt`` (flimo_set_ndt_chunk; 0: the default of 2^20)."""
        self._chk(self._L.flimo_set_ndt_chunk(self._h, int(pairs)))

    def set_corr_chunk(self, n):
        """Hypotheses per chunk of ``corr_poses`` (flimo_set_corr_chunk; 0: the default of 2^16)."""
        self._chk(self._L.flimo_set_corr_chunk(self._h, int(n)))

    def desc_ref_size(self) -> int:
        return int(self._L.flimo_desc_ref_size(self._h))

    def desc_ref_dim(self) -> int:
        return int(self._L.flimo_desc_ref_dim(self._h))

    def set_desc_chunk(self, queries_per_chunk=0, refs_per_split=0):
        """Queries per chunk of ``desc_match`` and reference rows per split of its grid (flimo_set_desc_chunk; 0: the defaults)."""
        self._chk(self._L.flimo_set_desc_chunk(self._h, int(queries_per_chunk), int(refs_per_split)))

    def desc_last_ms(self) -> float:
        """GPU ms of the last ``desc_match``'s launches (flimo_desc_last_ms; 0 unless ``set_timing`` is on)."""
        return float(self._L.flimo_desc_last_ms(self._h))

    def sc_db_size(self) -> int:
        return int(self._L.flimo_sc_db_size(self._h))

    def sc_db_shape(self):
        """(rings, sectors) of the resident Scan Context database, (0, 0) when it is empty (flimo_sc_db_shape)."""
        r, s = C.c_int(0), C.c_int(0)
        self._chk(self._L.flimo_sc_db_shape(self._h, C.byref(r), C.byref(s)))
        return int(r.value), int(s.value)

    def set_sc_chunk(self, queries_per_chunk=0, entries_per_split=0):
        """Queries per chunk of ``sc_match`` and entries per split of its grid (flimo_set_sc_chunk; 0: the defaults)."""
        self._chk(self._L.flimo_set_sc_chunk(self._h, int(queries_per_chunk), int(entries_per_split)))

    def sc_last_ms(self) -> float:
        """GPU ms of the last ``sc_match``'s launches (flimo_sc_last_ms; 0 unless ``set_timing`` is on)."""
        return float(self._L.flimo_sc_last_ms(self._h))

    def scan_voxel_filter(self, leaf: float) -> int:
        n = C.c_size_t(0)
        self._chk(self._L.flimo_scan_voxel_filter(self._h, float(leaf), C.byref(n)))
        return int(n.value)

    def raw_scan_filter_order_set(self, records, time_order=0, **cfg):
        """flimo_raw_scan_filter_order_set: ``records`` = the sweep as 32-byte PointType records (itemsize 32) or, with bit 2 of
        ``time_order`` set, as 16-byte {x, y, z, time word} records.  Returns (kept, last_stamp, nan_stamp, tied)."""
        fc = FilterCfg()
        for k, v in cfg.items():
            if k in ("crop_min", "crop_max"):
                setattr(fc, k, (C.c_float * 3)(*v))
            else:
                setattr(fc, k, v)
        rec = np.ascontiguousarray(records)
        n = rec.shape[0]
        assert n == 0 or rec.dtype.itemsize * (rec.size // n) == (16 if (time_order & 4) else 32)
        kept, last, nan, tied = C.c_size_t(0), C.c_double(0), C.c_int(0), C.c_int(0)
        self._chk(self._L.flimo_raw_scan_filter_order_set(self._h, rec.ctypes.data, n, C.byref(fc), int(time_order), C.byref(kept),
                                                          C.byref(last), C.byref(nan), C.byref(tied)))
        return int(kept.value), float(last.value), int(nan.value), int(tied.value)

    def raw_scan_order(self):
        n = C.c_size_t(0)
        self._chk(self._L.flimo_raw_scan_order(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self._chk(self._L.flimo_raw_scan_order(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def deskew_resident_offset(self, frames, L2B, last_x26, t_offset):
        assert frames.dtype == FRAME_DTYPE
        frames = np.ascontiguousarray(frames)
        self._chk(self._L.flimo_deskew_resident_offset(self._h, frames.ctypes.data, frames.shape[0],
                                                       np.ascontiguousarray(L2B, dtype=np.float32).reshape(-1),
                                                       np.ascontiguousarray(last_x26, dtype=np.float64), float(t_offset)))

    def scan_adopt(self, src: "HipCtx"):
        """The resident raw sweep of ``src`` becomes this context's (flimo_scan_adopt)."""
        self._chk(self._L.flimo_scan_adopt(self._h, src._h))

    def raw_scan_set(self, xyz, t):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        t = np.ascontiguousarray(t, dtype=np.float64)
        n = xyz.shape[0]
        stride = xyz.strides[0] if xyz.ndim == 2 else 12
        self._chk(self._L.flimo_raw_scan_set(self._h, xyz.reshape(-1), n, stride, t))

    def deskew_resident(self, frames: np.ndarray, L2B, last_x26):
        assert frames.dtype == FRAME_DTYPE
        frames = np.ascontiguousarray(frames)
        self._chk(self._L.flimo_deskew_resident(self._h, frames.ctypes.data, frames.shape[0],
                                                np.ascontiguousarray(L2B, dtype=np.float32).reshape(-1),
                                                np.ascontiguousarray(last_x26, dtype=np.float64)))

    # ---- measurement pass ----
    def match_reduce(self, x26, cfg: MatchCfg):
        HTH = np.zeros(144, np.float64)
        HTh = np.zeros(12, np.float64)
        M = C.c_int(0)
        self._chk(self._L.flimo_match_reduce(self._h, np.ascontiguousarray(x26, dtype=np.float64), C.byref(cfg), HTH,
                                             HTh, C.byref(M)))
        return HTH.reshape(12, 12), HTh, M.value

    def match_fetch(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._chk(self._L.flimo_match_fetch(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=MATCH_REC_DTYPE)
        self._chk(self._L.flimo_match_fetch(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def match_fetch_H(self):
        n = C.c_size_t(0)
        self._chk(self._L.flimo_match_fetch_H(self._h, None, None, 0, C.byref(n)))
        H = np.zeros((max(n.value, 1), 12), np.float64)
        h = np.zeros(max(n.value, 1), np.float64)
        self._chk(self._L.flimo_match_fetch_H(self._h, H.ctypes.data, h.ctypes.data, n.value, C.byref(n)))
        return H[:n.value], h[:n.value]

    def scan_to_world(self, x26) -> np.ndarray:
        n = self.scan_size()
        out = np.empty((max(n, 1), 3), dtype=np.float32)
        self._chk(self._L.flimo_scan_to_world(self._h, np.ascontiguousarray(x26, dtype=np.float64), out.ctypes.data, n))
        return out[:n]

    def scan_clouds(self, x26):
        """(body, world) xyz of the resident scan in one round trip (flimo_scan_clouds); copies of the context's pinned records."""
        b, w, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self._chk(self._L.flimo_scan_clouds(self._h, np.ascontiguousarray(x26, dtype=np.float64), C.byref(b), C.byref(w), C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
        rec = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value, 4))[:, :3].copy()
        return rec(b), rec(w)

    def scan_debug_clouds(self, x26):
        """(deskewed_scan, final_raw_scan) x y z w records of the last deskew (flimo_scan_debug_clouds): (n, 4) float32 copies."""
        d, f, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self._chk(self._L.flimo_scan_debug_clouds(self._h, np.ascontiguousarray(x26, dtype=np.float64), C.byref(d), C.byref(f), C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)
        rec = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value, 4)).copy()
        return rec(d), rec(f)

    def map_add_scan(self, x26, stamp=0.0):
        self._chk(self._L.flimo_map_add_scan(self._h, np.ascontiguousarray(x26, dtype=np.float64), float(stamp)))

    # ---- instrumentation ----
    def set_timing(self, level=2):
        """0 off, 1 k-NN kernel only, 2 every stage (True == 2)."""
        self._chk(self._L.flimo_set_timing(self._h, 2 if level is True else int(level)))

    def set_timing_stride(self, every=1):
        """Level 1 only: time every ``every``-th pass (sampling)."""
        self._chk(self._L.flimo_set_timing_stride(self._h, int(every)))

    def set_timing_deferred(self, on=True):
        """Read the timed passes' events when the totals are asked for, not right behind each pass (include/flimo_dev.h)."""
        self._chk(self._L.flimo_set_timing_deferred(self._h, 1 if on else 0))

    def pass_count(self) -> int:
        return int(self._L.flimo_pass_count(self._h))

    def fine_stats(self):
        o = (C.c_ulonglong * 4)()
        self._chk(self._L.flimo_fine_stats(self._h, o))
        return dict(active=bool(o[0]), points=int(o[1]), builds=int(o[2]), passes=int(o[3]))

    def tie_stats(self):
        o = (C.c_ulonglong * 2)()
        self._chk(self._L.flimo_tie_stats(self._h, o))
        return dict(passes_redone=int(o[0]), queries_settled=int(o[1]))

    def map_index_bytes(self):
        o = (C.c_uint64 * 6)()
        self._chk(self._L.flimo_map_index_bytes(self._h, o))
        return dict(points=int(o[0]), index=int(o[1]), second_level=int(o[2]), tiles=int(o[3]), tile_pool_relayouts=int(o[4]),
                    sorted_array_allocated=int(o[5]))

    def map_index_layout(self, level=0):
        """flimo_map_index_layout (include/flimo_dev.h): the layout of the main grid's index (``level`` 0) or of the second level's
        (1) as it was made.  ``valid`` False: that level has no index now (nothing else is in the dict then).  Drains the stream."""
        o = (C.c_double * 28)()
        self._chk(self._L.flimo_map_index_layout(self._h, int(level), o))
        if not o[19]:
            return dict(valid=False)
        ints = ("xs", "six", "siy", "siz", "nx", "ny", "nz", "ts", "ty", "tz", "ntx", "nty", "ntz", "escape_slots", "escape_slots_taken")
        d = dict(valid=True, ox=np.float32(o[0]), oy=np.float32(o[1]), oz=np.float32(o[2]), cell=np.float32(o[3]), points=int(o[20]))
        d.update((name, int(o[4 + i])) for i, name in enumerate(ints))
        if level == 1:
            d.update(qlo=tuple(int(o[21 + a]) for a in range(3)), qhi=tuple(int(o[24 + a]) for a in range(3)))
        return d

    def fused_pass_count(self) -> int:
        return int(self._L.flimo_fused_pass_count(self._h))

    def grid_selfcheck(self):
        """(mismatching words of the incrementally maintained index vs a from-scratch sort, merges, full builds)."""
        mm = C.c_uint64(0)
        st = (C.c_uint64 * 2)()
        self._chk(self._L.flimo_map_grid_selfcheck(self._h, C.byref(mm), st))
        return int(mm.value), int(st[0]), int(st[1])

    def set_debug_records(self, on=True):
        self._chk(self._L.flimo_set_debug_records(self._h, int(on)))

    def last_kernel_ms(self):
        a = C.c_float(0)
        b = C.c_float(0)
        d = C.c_float(0)
        self._chk(self._L.flimo_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(d)))
        return a.value, b.value, d.value

    def timing_totals(self, reset=False):
        a = C.c_double(0); b = C.c_double(0); d = C.c_double(0); n = C.c_longlong(0); q = C.c_longlong(0)
        self._chk(self._L.flimo_timing_totals(self._h, C.byref(a), C.byref(b), C.byref(d), C.byref(n), C.byref(q), int(reset)))
        return dict(knn_ms=a.value, widen_ms=b.value, fit_ms=d.value, passes=n.value, queries=q.value)

    def set_path_switches(self, tail=-1, fuse=-1):
        self._chk(self._L.flimo_set_path_switches(self._h, int(tail), int(fuse)))

    def timing_split(self, reset=False):
        o = np.zeros(6)
        self._chk(self._L.flimo_timing_split(self._h, o, int(reset)))
        return dict(fused_ms=o[0], fused_n=int(o[1]), knn_ms=o[2], widen_ms=o[3], fit_ms=o[4], separate_n=int(o[5]))

    def update_chain(self, cfg: "MatchCfg", x26, P, limits, R=0.001, D=5.0, max_iter=3, want_log=True):
        """The iterations of the update of the resident scan enqueued at once (flimo_update_chain).  Returns a dict: status (0 declined,
        2 handed back), reason (1 M < 23, 2 ties, 3 degenerate, 5 the iteration that ends the loop), passes, it_next, t, x (26), the
        handed-back iteration's sums (meas: M, HTH, HTh or None) and the per-pass log."""
        io = ChainIO()
        io.x26[:] = list(np.asarray(x26, dtype=np.float64))
        io.P[:] = list(np.asarray(P, dtype=np.float64).reshape(-1))
        io.limits[:] = list(np.asarray(limits, dtype=np.float64))
        io.R, io.D, io.max_iter, io.want_log = float(R), float(D), int(max_iter), int(bool(want_log))
        self._chk(self._L.flimo_update_chain(self._h, C.byref(cfg), C.byref(io)))
        n_log = min(CHAIN_MAX_PASSES, io.passes + (1 if io.status == 2 else 0))   # + the handed-back iteration's counts
        log = [dict(M=io.log[i].M, stragglers=io.log[i].stragglers, ties=io.log[i].ties,
                    HTH=np.array(io.log[i].HTH).reshape(12, 12), HTh=np.array(io.log[i].HTh), dx=np.array(io.log[i].dx),
                    x_after=np.array(io.log[i].x_after)) for i in range(n_log)]
        meas = dict(M=io.meas_M, HTH=np.array(io.meas_HTH).reshape(12, 12), HTh=np.array(io.meas_HTh)) if io.meas_valid else None
        return dict(status=io.status, reason=io.reason, passes=io.passes, it_next=io.it_next, t=io.t, x=np.array(io.x26_out),
                    meas=meas, log=log)

    def set_update_mode(self, mode: int):
        """0: chain or host loop by this host's launch -> result round trip; 1: host loop; 2: chain."""
        self._chk(self._L.flimo_set_update_mode(self._h, int(mode)))

    def update_mode(self):
        ch = C.c_int(0); rtt = C.c_double(0)
        self._chk(self._L.flimo_update_mode(self._h, C.byref(ch), C.byref(rtt)))
        return dict(chained=bool(ch.value), launch_rtt_us=rtt.value)

    def set_pass_pipeline(self, on: bool):
        self._chk(self._L.flimo_set_pass_pipeline(self._h, int(on)))

    def pass_pipeline_end(self):
        self._chk(self._L.flimo_pass_pipeline_end(self._h))

    def pass_pipeline_last(self):
        """The next match_reduce is the last pass its update can run: nothing is queued behind it."""
        self._chk(self._L.flimo_pass_pipeline_last(self._h))

    def pass_pipeline_stats(self):
        o = (C.c_ulonglong * 4)()
        self._chk(self._L.flimo_pass_pipeline_stats(self._h, o))
        return dict(published=int(o[0]), cancelled=int(o[1]), aged=int(o[2]), left=int(o[3]))

    def chain_stats(self, reset=False):
        o = np.zeros(5)
        self._chk(self._L.flimo_chain_stats(self._h, o, int(reset)))
        return dict(algebra_ms=o[0], algebra_n=int(o[1]), chains=int(o[2]), handed_back=int(o[3]), declined=int(o[4]))

    def ieskf_eval(self, op, items):
        """The device filter's helper ``op`` (IK_* below; include/flimo_dev.h: flimo_ieskf_eval) on a batch: items [n, n_in] ->
        [n, n_out], on the GPU."""
        a, no = ik_items(op, items)
        out = np.zeros((a.shape[0], no))
        if a.shape[0]:
            self._chk(self._L.flimo_ieskf_eval(self._h, int(op), a.reshape(-1), a.shape[0], out.reshape(-1)))
        return out

    def ieskf_run_fixed(self, x26, P, limits, partials, extras=None, tag_ok=None, R=0.001, D=5.0, max_iter=3):
        """The whole device algebra on caller-given sums (flimo_ieskf_run_fixed): ``partials`` [n_sets, 8, 91], ``extras``
        [n_sets, 2] (stragglers, ties; zeros when None), ``tag_ok`` [n_sets] or None.  Returns (iterations, final): per iteration
        run a dict pre_dxn, pre_AG, HTH, HTh, dx, x_after (None when it handed back), pose (66 float32), prev_RT, status, it, t,
        passes, went_on; final: status, reason, passes, it, t, x, passinfo [12, 3], sums [91]."""
        x, Pm, lim, part = ik_fixed_args(x26, P, limits, partials)
        ns = part.shape[0]
        ex = np.zeros((ns, 2)) if extras is None else np.ascontiguousarray(extras, dtype=np.float64).reshape(ns, 2)
        tg = None if tag_ok is None else np.ascontiguousarray(tag_ok, dtype=np.int32).reshape(ns)
        it_out = np.zeros((int(max_iter) + 1, IK_ITER_N))
        fin = np.zeros(IK_FINAL_N)
        n = C.c_int(0)
        self._chk(self._L.flimo_ieskf_run_fixed(self._h, x, Pm, lim, float(R), float(D), int(max_iter), ns, part.reshape(-1), ex.reshape(-1),
                                                None if tg is None else tg.ctypes.data, it_out.reshape(-1), fin, C.byref(n)))
        its = []
        for r in it_out[:n.value]:
            on = bool(r[590])
            its.append(dict(pre_dxn=r[0:23].copy(), pre_AG=r[23:299].copy(), HTH=r[299:443].reshape(12, 12).copy() if on else None,
                            HTh=r[443:455].copy() if on else None, dx=r[455:478].copy() if on else None,
                            x_after=r[478:504].copy() if on else None, pose=r[504:570].astype(np.float32), prev_RT=r[570:586].astype(np.float32),
                            status=int(r[586]), it=int(r[587]), t=int(r[588]), passes=int(r[589]), went_on=on))
        final = dict(status=int(fin[0]), reason=int(fin[1]), passes=int(fin[2]), it=int(fin[3]), t=int(fin[4]), x=fin[5:31].copy(),
                     passinfo=fin[31:67].reshape(12, 3).copy(), sums=fin[67:158].copy())
        return its, final

    def last_widen_count(self) -> int:
        return int(self._L.flimo_last_widen_count(self._h))

    def set_wait_timeout_ms(self, ms: int):
        self._chk(self._L.flimo_set_wait_timeout_ms(self._h, int(ms)))

    def last_stragglers(self) -> int:
        return int(self._L.flimo_last_stragglers(self._h))

    def stragglers_by_pass(self):
        o = (C.c_int * 4)()
        self._chk(self._L.flimo_stragglers_by_pass(self._h, o))
        return [int(v) for v in o]

    def last_candidates_per_query(self) -> float:
        return float(self._L.flimo_last_candidates_per_query(self._h))


# flimo_ieskf_eval's ops (include/flimo_dev.h: FLIMO_IK_*) and the record sizes of flimo_ieskf_run_fixed
(IK_SO3_LOG, IK_A_T, IK_EXP_QUAT, IK_COS_SINC_SQRT, IK_S2_BX, IK_S2_BOXMINUS, IK_S2_J, IK_GJ12_INVERSE, IK_GJ12_SOLVE, IK_PRE) = range(10)
IK_ITER_N, IK_FINAL_N, IK_HLOG_N = 591, 158, 207


def ik_op_shape(op):
    ni, no = C.c_int(0), C.c_int(0)
    if load_hip().flimo_ieskf_op_shape(int(op), C.byref(ni), C.byref(no)) != 0:
        raise FlimoError(f"flimo_ieskf_op_shape({op}): unknown op")
    return ni.value, no.value


def ik_items(op, items):
    ni, no = ik_op_shape(op)
    return np.ascontiguousarray(items, dtype=np.float64).reshape(-1, ni), no


def ik_fixed_args(x26, P, limits, partials):
    return (np.ascontiguousarray(x26, dtype=np.float64).reshape(26), np.ascontiguousarray(P, dtype=np.float64).reshape(529),
            np.ascontiguousarray(limits, dtype=np.float64).reshape(23), np.ascontiguousarray(partials, dtype=np.float64).reshape(-1, 8, 91))


def ieskf_eval_host(op, items):
    """The host twin of ``HipCtx.ieskf_eval`` (flimo_ieskf_eval_host; no GPU): returns (out [n, n_out], branch [n] int32)."""
    a, no = ik_items(op, items)
    out = np.zeros((a.shape[0], no))
    br = np.zeros(max(a.shape[0], 1), np.int32)
    if a.shape[0]:
        rc = load_hip().flimo_ieskf_eval_host(int(op), a.reshape(-1), a.shape[0], out.reshape(-1), br.ctypes.data)
        if rc != 0:
            raise FlimoError(f"flimo_ieskf_eval_host({op}) failed ({rc})")
    return out, br[:a.shape[0]]


def device_large_bar(device: int = 0) -> bool:
    """The hardware's side of the pipelined host loop (flimo_device_large_bar): the device maps its memory for the host."""
    v = C.c_int(0)
    rc = load_hip().flimo_device_large_bar(int(device), C.byref(v))
    if rc != 0:
        raise FlimoError(f"flimo_device_large_bar({device}) failed: {_ERRS.get(rc, rc)}")
    return bool(v.value)


def default_match_cfg(**kw) -> MatchCfg:
    c = MatchCfg(5, 2000, 10000, 2.0, 5.0e-2, 1)
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def insert_rule_replay(batches, min_extent=0.2, downsample=True):
    """Host-only replay of the reference's octree insert rule; returns (keep flags per batch, stored count)."""
    L = load_hip()
    sizes = np.array([b.shape[0] for b in batches], dtype=np.uint64)
    xyz = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 3) for b in batches]))
    keep = np.zeros(xyz.shape[0], dtype=np.uint8)
    stored = C.c_size_t(0)
    rc = L.flimo_insert_rule_replay(float(min_extent), int(downsample), xyz.reshape(-1), sizes.ctypes.data, len(batches),
                                    keep.ctypes.data, C.byref(stored))
    if rc != 0:
        raise FlimoError(f"flimo_insert_rule_replay failed ({rc})")
    out, off = [], 0
    for b in batches:
        out.append(keep[off:off + b.shape[0]].astype(bool))
        off += b.shape[0]
    return out, int(stored.value)
