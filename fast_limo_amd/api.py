"""Python view of the host C++ library (``libfast_limo.so``): ``Localizer`` with the reference's
call pattern (``init`` -> ``updateIMU`` / ``updatePointCloud`` -> getters, reference
``src/main.cpp:14-95``).  Everything here forwards to C++ through ``include/flimo_localizer_c.h``;
there is no Python compute path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import numpy as np

from . import _abi, _lib
from ._abi import LocCfg
from ._lib import FlimoError, f32p, f64p

_host = None

HOST_SYMBOLS = _abi.HOST_SYMBOLS      # every symbol include/flimo_localizer_c.h declares (tests check the .so exports each one)


# the reference's PointType (Common.hpp:100-113): xyz1, intensity, 4 bytes of padding, 8-byte time union
POINT_DTYPE = np.dtype({"names": ["x", "y", "z", "w", "intensity", "tu"],
                        "formats": [np.float32, np.float32, np.float32, np.float32, np.float32, np.uint64],
                        "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})


def make_points_velodyne(pts5) -> np.ndarray:
    """(n, 5) float32 x y z intensity time -> the reference's 32-byte PointType records (VELODYNE view of the time union),
    what a ROS driver hands to Localizer::updatePointCloud."""
    p5 = np.ascontiguousarray(pts5, dtype=np.float32).reshape(-1, 5)
    p = np.zeros(p5.shape[0], POINT_DTYPE)
    p["x"], p["y"], p["z"], p["w"], p["intensity"] = p5[:, 0], p5[:, 1], p5[:, 2], 1.0, p5[:, 3]
    p.view(np.uint8).reshape(-1, 32)[:, 24:28] = p5[:, 4:5].copy().view(np.uint8)
    return p


def default_cfg(**kw) -> LocCfg:
    """Defaults of reference ``src/main.cpp:101-168`` with the synthetic-benchmark deltas of
    SURVEY.md section 8 d: identity extrinsics / sm, calibration and filters off, Velodyne time."""
    c = LocCfg()
    c.NUM_MATCH_POINTS, c.MAX_NUM_MATCHES, c.MAX_NUM_PC2MATCH = 5, 2000, 10000
    c.bucket_size = 2
    c.MAX_DIST_PLANE, c.PLANE_THRESHOLD = 2.0, 5.0e-2
    c.min_extent, c.downsampling = 0.2, 1
    c.MAX_NUM_ITERS, c.estimate_extrinsics = 3, 1
    for i in range(23):
        c.LIMITS[i] = 1e-3
    c.cov_gyro, c.cov_acc, c.cov_bias_gyro, c.cov_bias_acc = 6e-4, 1e-2, 1e-5, 3e-4
    c.time_offset, c.end_of_sweep, c.num_threads = 1, 0, 10
    eye = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for i in range(9):
        c.imu2baselink_R[i] = eye[i]
        c.lidar2baselink_R[i] = eye[i]
        c.imu_sm[i] = eye[i]
    c.voxel_active, c.leaf_size = 0, 0.25
    c.crop_active = 0
    for i in range(3):
        c.cropBoxMin[i], c.cropBoxMax[i] = -1.0, 1.0
    c.dist_active, c.min_dist = 0, 4.0
    c.rate_active, c.rate_value = 0, 4
    c.fov_active, c.fov_angle = 0, float(np.pi)
    c.sensor_type = 1
    c.gravity_align = c.calibrate_accel = c.calibrate_gyro = 0
    c.imu_calib_time = 3.0
    c.gpu_device, c.gpu_cell_size = 0, 0.0
    c.debug = 0
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def host_lib_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfast_limo.so")


def load_host():
    global _host
    if _host is not None:
        return _host
    _lib.load_hip()                     # resolve libflimo_hip.so first (same directory, rpath $ORIGIN)
    path = host_lib_path()
    if not os.path.exists(path):
        raise FlimoError(f"{path} not found: build first")
    L = C.CDLL(path)
    _abi.declare(L, 1)
    _host = L
    return L


class _MapperCtxView(_lib.HipCtx):
    """The Mapper's GPU context as seen from Python.  The handle is fetched through flimo_loc_ctx on every use, which
    waits for a map insert still running on the Mapper's worker thread."""

    @property
    def _h(self):
        return C.c_void_p(self._loc._L.flimo_loc_ctx(self._loc._h))


class Localizer(_lib._SharedEntries):
    """fast_limo::Localizer (one instance per GPU)."""

    def __init__(self, cfg: LocCfg):
        L = load_host()
        h = C.c_void_p()
        rc = L.flimo_loc_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise FlimoError(f"flimo_loc_create failed ({rc}): no gfx950 device or HIP error -- there is no CPU fallback")
        self._h, self._L, self.cfg = h, L, cfg
        self.hip = _MapperCtxView.__new__(_MapperCtxView)      # non-owning view of the Mapper's context
        self.hip._loc = self
        self.hip._L = _lib.load_hip()
        self.hip.close = lambda: None

    def close(self):
        if getattr(self, "_h", None):
            self._L.flimo_loc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update_imu(self, stamp, ang_vel, lin_accel):
        self._L.flimo_loc_update_imu(self._h, float(stamp), np.ascontiguousarray(ang_vel, dtype=np.float32),
                                     np.ascontiguousarray(lin_accel, dtype=np.float32))

    def update_imu_n(self, stamps, ang_vel, lin_accel):
        """Several samples in arrival order with one call across the binding (one updateIMU each)."""
        t = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(ang_vel, dtype=np.float32).reshape(-1)
        a = np.ascontiguousarray(lin_accel, dtype=np.float32).reshape(-1)
        assert w.size == 3 * t.size and a.size == 3 * t.size
        rc = self._L.flimo_loc_update_imu_n(self._h, t.size, t, w, a)
        if rc != 0:
            raise RuntimeError("flimo_loc_update_imu_n failed (%d)" % rc)

    def replay(self, sweeps, sweep_stamps, imu_until, imu_stamps, ang_vel, lin_accel):
        """A recorded drive at full speed from native code (flimo_loc_replay): ``sweeps`` is a list of POINT_DTYPE arrays.
        Returns (status per sweep, seconds since the start at which each call returned)."""
        sweeps = [np.ascontiguousarray(p) for p in sweeps]
        n = len(sweeps)
        ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in sweeps])
        npts = np.array([p.shape[0] for p in sweeps], np.uintp)
        t = np.ascontiguousarray(imu_stamps, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(ang_vel, dtype=np.float32).reshape(-1)
        a = np.ascontiguousarray(lin_accel, dtype=np.float32).reshape(-1)
        status = np.zeros(n, np.int32)
        secs = np.zeros(n, np.float64)
        rc = self._L.flimo_loc_replay(self._h, n, ptrs, npts, np.ascontiguousarray(sweep_stamps, dtype=np.float64),
                                      np.ascontiguousarray(imu_until, dtype=np.float64), t.size, t, w, a, status, secs)
        if rc != 0:
            raise RuntimeError("flimo_loc_replay failed (%d)" % rc)
        return status, secs

    def update_pointcloud(self, pts5, stamp) -> int:
        p = np.ascontiguousarray(pts5, dtype=np.float32).reshape(-1, 5)
        return int(self._L.flimo_loc_update_pointcloud(self._h, p.reshape(-1), p.shape[0], float(stamp)))

    def update_pointcloud_points(self, pts32, stamp) -> int:
        """pts32: structured array in the reference's 32-byte PointType layout (itemsize 32)."""
        p = np.ascontiguousarray(pts32)
        assert p.dtype.itemsize == 32
        return int(self._L.flimo_loc_update_pointcloud_points(self._h, p.ctypes.data, p.shape[0], float(stamp)))

    def map_add(self, xyz, stamp=0.0):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        rc = self._L.flimo_loc_map_add(self._h, xyz.reshape(-1), xyz.shape[0], float(stamp))
        if rc != 0:
            raise FlimoError(f"map_add failed ({rc})")

    def map_size(self) -> int:
        return int(self._L.flimo_loc_map_size(self._h))

    def get_x(self):
        x = np.empty(26, np.float64)
        self._L.flimo_loc_get_x(self._h, x)
        return x

    def set_x(self, x):
        self._L.flimo_loc_set_x(self._h, np.ascontiguousarray(x, dtype=np.float64))

    def get_P(self):
        P = np.empty(529, np.float64)
        self._L.flimo_loc_get_P(self._h, P)
        return P.reshape(23, 23)

    def set_P(self, P):
        self._L.flimo_loc_set_P(self._h, np.ascontiguousarray(P, dtype=np.float64).reshape(-1))

    def set_flags(self, add_to_map=True, download_clouds=True, keep_log=False):
        self._L.flimo_loc_set_flags(self._h, int(add_to_map), int(download_clouds), int(keep_log))

    def sync(self):
        """Wait for the map insert of the last scan (it runs on the Mapper's worker thread)."""
        self._L.flimo_loc_sync(self._h)

    def set_async_insert(self, on=True):
        self._L.flimo_loc_set_async_insert(self._h, int(on))

    def set_lazy_time_order(self, on=True):
        """off: the sweep is always put into the reference's time order before the GPU sees it (A/B of the arrival-order path)."""
        self._L.flimo_loc_set_lazy_time_order(self._h, int(on))

    def set_gpu_filters(self, on=True):
        self._L.flimo_loc_set_gpu_filters(self._h, int(on))

    def set_exact_tied_order(self, on=True):
        """Equal stamps in a sweep whose time order is observable: the reference's library order (host front end) instead of the
        device's stable order (flimo_localizer_c.h)."""
        self._L.flimo_loc_set_exact_tied_order(self._h, int(on))

    def set_local_map(self, half_extent, recentre_dist):
        """A local map (default off): after a sweep's insert, once the position has moved more than ``recentre_dist`` (per-axis
        maximum) from the box centre, the map is cropped to position +- ``half_extent``.  A non-positive or non-finite extent
        switches it off."""
        self._L.flimo_loc_set_local_map(self._h, np.ascontiguousarray(half_extent, dtype=np.float32).reshape(3), float(recentre_dist))

    def set_map_carving(self, every_n_sweeps, **cfg):
        """Map carving (default off): on every ``every_n_sweeps``-th registered sweep that is inserted, the stored points that sweep
        looks through are forgotten, behind the insert (flimo_loc_set_map_carving); ``cfg``: the fields of ``_lib.carve_cfg``.
        ``every_n_sweeps <= 0`` or an invalid cfg switches it off."""
        k = _lib.carve_cfg(**cfg)
        self._L.flimo_loc_set_map_carving(self._h, int(every_n_sweeps), C.byref(k))

    # ---- the entries shared with HipCtx (_lib._SharedEntries), on the flimo_loc_* symbols ----
    map_knn, map_radius_search = _lib._SharedEntries._knn_k, _lib._SharedEntries._radius_search
    map_normals, map_normals_range = _lib._SharedEntries._normals, _lib._SharedEntries._normals_range

    def _symbol(self, entry):
        return _abi.LOC_OF[entry]

    def _fail(self, entry, rc):
        raise FlimoError(f"{self._symbol(entry)} failed ({rc})")

    def _scan_size(self):
        return self.hip.scan_size()      # (the scan resident in the map's context; 0 when there is no map yet)

    def last_carve_removed(self) -> int:
        return int(self._L.flimo_loc_last_carve_removed(self._h))

    def voxel_cloud(self, res):
        """The decimated map one publishes or saves: the centroids of the voxels of edge ``res`` as float32 [nv, 3], in ascending
        (cz, cy, cx) -- ``map_voxels`` with only the centroid asked for."""
        return self.map_voxels(want=("centroid",), leaf=res)["centroid"].astype(np.float32)

    def desc_ref_size(self) -> int:
        return self.hip.desc_ref_size()

    def last_sweep_tied(self) -> bool:
        return bool(self._L.flimo_loc_last_sweep_tied(self._h))

    def set_propagation_wait(self, seconds: float):
        """< 0: wait for the IMU stream without bound (the reference's behaviour; needs a second thread feeding update_imu)."""
        self._L.flimo_loc_set_propagation_wait(self._h, float(seconds))

    def last_insert_seconds(self):
        return float(self._L.flimo_loc_last_insert_seconds(self._h))

    def passes(self):
        out = []
        for i in range(self._L.flimo_loc_num_passes(self._h)):
            M = C.c_int(0)
            HTH = np.empty(144); HTh = np.empty(12); dx = np.empty(23); xa = np.empty(26)
            self._L.flimo_loc_get_pass(self._h, i, C.byref(M), HTH, HTh, dx, xa)
            out.append(dict(M=M.value, HTH=HTH.reshape(12, 12), HTh=HTh, dx=dx, x_after=xa))
        return out

    def pc2match(self, out=None):
        """xyz of get_pc2match_pointcloud(); `out`: a C-contiguous float32 (>= n, 3) array to fill instead of a fresh one."""
        return self._cloud(self._L.flimo_loc_get_pc2match, out)

    def final_scan(self, out=None):
        """xyz of get_pointcloud() (world frame); `out` as for pc2match."""
        return self._cloud(self._L.flimo_loc_get_final_scan, out)

    def orig_scan(self):
        """get_orig_pointcloud(): the filtered sweep (LiDAR frame) as POINT_DTYPE records; empty unless cfg.debug."""
        return self._debug_cloud(0)

    def deskewed_scan(self):
        """get_deskewed_pointcloud(): the sweep in time order, deskewed into the world frame (POINT_DTYPE); empty unless cfg.debug."""
        return self._debug_cloud(1)

    def final_raw_scan(self):
        """get_finalraw_pointcloud(): the un-voxelised deskewed sweep in the world frame of the corrected pose (POINT_DTYPE); empty
        unless cfg.debug."""
        return self._debug_cloud(2)

    def _debug_cloud(self, which):
        n = int(self._L.flimo_loc_get_debug_cloud(self._h, which, None, 0))
        out = np.zeros(n, POINT_DTYPE)
        if n:
            self._L.flimo_loc_get_debug_cloud(self._h, which, out.ctypes.data, n)
        return out

    def _cloud(self, getter, out):
        n = int(getter(self._h, None, 0))
        if out is None or out.shape[0] < n:
            out = np.empty((max(n, 1), 3), np.float32)
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.shape[1] == 3
        getter(self._h, out.ctypes.data, n)
        return out[:n]

    def stage_times(self):
        t = np.zeros(4)
        self._L.flimo_loc_get_stage_times(self._h, t)
        return dict(host_prep=t[0], deskew=t[1], update=t[2], map_insert=t[3])

    def pose_cov(self):
        c = np.zeros(36)
        self._L.flimo_loc_get_pose_cov(self._h, c)
        return c.reshape(6, 6).T       # returned column-major like the reference

    def host_profile(self, reset=False):
        t = np.zeros(4)
        self._L.flimo_loc_host_profile(self._h, t, int(reset))
        return dict(deskew_s=t[0], update_s=t[1], match_reduce_s=t[2], passes=t[3])

    def register_resident(self, x26_prior, P_prior) -> int:
        return int(self._L.flimo_loc_register_resident(self._h, np.ascontiguousarray(x26_prior, dtype=np.float64),
                                                       np.ascontiguousarray(P_prior, dtype=np.float64).reshape(-1)))

    def register_resident_call(self, x26_prior, P_prior):
        """A zero-argument callable doing register_resident(x26_prior, P_prior): the arrays are converted and the ctypes
        prototype is bound once, so a timing loop pays for the library call, not for the harness."""
        x = np.ascontiguousarray(x26_prior, dtype=np.float64).copy()
        P = np.ascontiguousarray(P_prior, dtype=np.float64).reshape(-1).copy()
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
        fn = proto(("flimo_loc_register_resident", self._L))
        h, xp, pp = self._h.value, x.ctypes.data, P.ctypes.data

        def call(_keep=(x, P)):
            return fn(h, xp, pp)
        return call


class LocalMapRule:
    """The local-map policy's rule (flimo_local_map_rule) with its state: ``step(p)`` returns (lo, hi) when the map is to be cropped
    now, None when not; ``off`` is True when the arguments switch the policy off."""

    def __init__(self, half_extent, recentre_dist):
        self._L = load_host()
        self.half = np.ascontiguousarray(half_extent, dtype=np.float32).reshape(3)
        self.recentre = float(recentre_dist)
        self.centre = np.zeros(3, np.float64)
        self.have = C.c_int(0)
        self.off = False

    def step(self, p):
        lo = np.zeros(3, np.float32)
        hi = np.zeros(3, np.float32)
        rc = self._L.flimo_local_map_rule(np.ascontiguousarray(p, dtype=np.float64).reshape(3), self.half, self.recentre, self.centre,
                                          C.byref(self.have), lo, hi)
        self.off = rc < 0
        return (lo, hi) if rc == 1 else None


class CarveRule:
    """The carving policy's counting rule (flimo_carve_rule) restated, with its state: ``step()`` -- once per inserted sweep -- returns
    True when the map is to be carved now; ``off`` is True when ``every_n_sweeps`` switches the policy off."""

    def __init__(self, every_n_sweeps):
        self.every = int(every_n_sweeps)
        self.count = 0
        self.off = self.every <= 0

    def step(self) -> bool:
        if self.off:
            return False
        self.count += 1
        if self.count < self.every:
            return False
        self.count = 0
        return True


def carve_sensor(x26) -> np.ndarray:
    """The sensor origin the carving policy uses for a state (flimo_carve_sensor restated): float32(t + R l), float64 arithmetic,
    R from the attitude quaternion x26[3:7] (x y z w) as Eigen forms it, l = x26[11:14] the lidar-to-baselink translation."""
    x26 = np.asarray(x26, np.float64)
    x, y, z, w = x26[3:7]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = ((1.0 - (tyy + tzz), txy - twz, txz + twy), (txy + twz, 1.0 - (txx + tzz), tyz - twx), (txz - twy, tyz + twx, 1.0 - (txx + tyy)))
    l = x26[11:14]
    return np.float32([x26[a] + ((R[a][0] * l[0] + R[a][1] * l[1]) + R[a][2] * l[2]) for a in range(3)])


def cluster_lists(label, min_size=1, max_size=0):
    """The labels of ``map_clusters`` as pcl::EuclideanClusterExtraction reports clusters: a list of int64 index arrays (positions in
    ``label``, each ascending), one per label whose count c in ``label`` has min_size <= c and (max_size == 0 or c <= max_size),
    ordered by count descending, then by label.  Pure numpy."""
    label = np.asarray(label).reshape(-1)
    if int(min_size) < 0 or int(max_size) < 0 or 0 < int(max_size) < int(min_size):
        raise ValueError("cluster_lists: min_size, max_size must be >= 0 and max_size 0 or >= min_size")
    if label.size == 0:
        return []
    order = np.argsort(label, kind="stable")      # (stable: positions ascending within a label)
    labs, start, cnt = np.unique(label[order], return_index=True, return_counts=True)
    keep = cnt >= int(min_size)
    if int(max_size) > 0:
        keep &= cnt <= int(max_size)
    pick = np.flatnonzero(keep)
    pick = pick[np.lexsort((labs[pick], -cnt[pick]))]
    return [order[start[j]:start[j] + cnt[j]].astype(np.int64) for j in pick]


def fitness_cost(inliers, sum_sqd, n, max_dist):
    """The truncated least-squares cost of pose hypotheses from ``scan_fitness``' two numbers: every scan point pays its squared
    distance to the map, one without a neighbour inside the gate pays the gate's: sum_sqd + (n - inliers) * max_dist^2 (float64).
    It is the one number that ranks hypotheses with different inlier counts; the lowest wins."""
    return np.asarray(sum_sqd, np.float64) + (float(n) - np.asarray(inliers, np.float64)) * (float(max_dist) * float(max_dist))


def corr_triplets(m, nh, seed=0):
    """[nh, 3] int32: ``nh`` samples of three DISTINCT indices below ``m`` (m >= 3) from ``numpy.random.default_rng(seed)`` -- the
    minimal samples of ``corr_poses``.  Three draws a, b', c' from m, m - 1, m - 2 values, then b' and c' stepped over the indices
    already taken: every ordered triple of distinct indices is equally likely."""
    m, nh = int(m), int(nh)
    if m < 3:
        raise ValueError("corr_triplets: three distinct indices need m >= 3")
    rng = np.random.default_rng(seed)
    a = rng.integers(0, m, nh)
    b = rng.integers(0, m - 1, nh)
    c = rng.integers(0, m - 2, nh)
    b = b + (b >= a)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    c = c + (c >= lo)
    c = c + (c >= hi)
    return np.stack([a, b, c], axis=1).astype(np.int32)


def corr_pose_host(src3, dst3, **cfg):
    """The pose of ONE triplet of correspondences on the host (flimo_corr_pose_host: the function the solve kernel calls):
    ``src3`` / ``dst3`` [3, 3] = the points a, b, c of either cloud; ``cfg``: the fields of ``_lib.corr_cfg``.  Returns (status,
    pose7 [7] float64: t, x y z w, rt [3, 4] float32: the matrix ``scan_fitness`` would form from it); NaN unless CORR_OK."""
    L = _lib.load_hip()
    s = np.ascontiguousarray(src3, dtype=np.float32).reshape(9)
    d = np.ascontiguousarray(dst3, dtype=np.float32).reshape(9)
    k = _lib.corr_cfg(**cfg)
    pose = np.zeros(7)
    rt = np.zeros(12, np.float32)
    rc = L.flimo_corr_pose_host(s.ctypes.data, d.ctypes.data, C.byref(k), pose.ctypes.data, rt.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_corr_pose_host failed ({rc})")
    return int(rc), pose, rt.reshape(3, 4)


def corr_consensus(obj, src, dst, nh, seed=0, top=8, x26_like=None, **cfg):
    """Pose guesses from putative correspondences (``src[i]`` in the body frame is ``dst[i]`` in the map's): ``nh`` samples of
    ``corr_triplets(m, nh, seed)`` through ``obj.corr_poses`` (a ``HipCtx`` or a ``Localizer``; ``cfg``: the fields of
    ``_lib.corr_cfg``), the OK hypotheses ranked by ``inliers`` descending, then by ``fitness_cost(inliers, sum_sqd, m, max_dist)``
    ascending (then by index).  Returns a dict of the best ``top``: x26 [k, 26] -- pos and rot filled in, everything else copied from
    ``x26_like`` [26] or zero with identity extrinsics: rows for ``scan_fitness`` / ``scan_align`` --, inliers, sum_sqd, cost [k],
    index [k] (the row of the hypothesis in tri), tri [k, 3]; and survivors: the number of OK hypotheses."""
    s = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    m = s.shape[0]
    tri = corr_triplets(m, nh, seed)
    out = obj.corr_poses(s, dst, tri, want=("pose",), **cfg)
    ok = np.nonzero(out["status"] == _lib.CORR_OK)[0]
    max_dist = float(_lib.corr_cfg(**cfg).max_dist)
    gate = max_dist if np.isfinite(max_dist) else 0.0      # (no gate: every pair is an inlier and pays its distance)
    cost = fitness_cost(out["inliers"][ok], out["sum_sqd"][ok], m, gate)
    order = np.lexsort((ok, cost, -out["inliers"][ok].astype(np.int64)))[:max(int(top), 0)]
    best = ok[order]
    base = np.zeros(26)
    base[10] = 1.0
    if x26_like is not None:
        base = np.array(np.asarray(x26_like, np.float64).reshape(26))
    x = np.tile(base, (best.size, 1))
    x[:, 0:7] = out["pose"][best]
    return dict(x26=x, inliers=out["inliers"][best], sum_sqd=out["sum_sqd"][best], cost=cost[order], index=best.astype(np.int64),
                tri=tri[best], survivors=int(ok.size))


def plane_solve_host(p3, **cfg):
    """The plane of ONE triplet of points on the host (flimo_plane_solve_host: the function the solve kernel of ``map_planes``
    calls): ``p3`` [3, 3] = the points a, b, c; ``cfg``: the fields of ``_lib.plane_cfg``.  Returns (status, plane4 [4] float64:
    nx ny nz d, nf [3] float32: the normal the inlier test uses); NaN unless PLANE_OK.  It sees points, not indices."""
    L = _lib.load_hip()
    p = np.ascontiguousarray(p3, dtype=np.float32).reshape(9)
    k = _lib.plane_cfg(**cfg)
    plane = np.zeros(4)
    nf = np.zeros(3, np.float32)
    rc = L.flimo_plane_solve_host(p.ctypes.data, C.byref(k), plane.ctypes.data, nf.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_plane_solve_host failed ({rc})")
    return int(rc), plane, nf


def voxel_key_host(p, leaf):
    """The voxel of ONE point on the host (flimo_voxel_key_host: the function the key kernel of ``map_voxels`` calls): (inside,
    ijk [3] int32 = (cx, cy, cz), key); an outside point has ijk 0 and the all-ones key.  Needs no device."""
    L = _lib.load_hip()
    q = np.ascontiguousarray(p, dtype=np.float32).reshape(3)
    ijk = np.zeros(3, np.int32)
    key = C.c_uint64(0)
    rc = L.flimo_voxel_key_host(q.ctypes.data, float(leaf), ijk.ctypes.data, C.byref(key))
    if rc < 0:
        raise FlimoError(f"flimo_voxel_key_host failed ({rc})")
    return rc == 0, ijk, int(key.value)


def region_joined_host(pi, ni, pj, nj, **cfg):
    """The predicates of ``map_regions`` for ONE pair on the host (flimo_region_joined_host: the functions the link kernel calls):
    (smooth_i, smooth_j, joined) as bools; ``ni`` / ``nj`` are rows nx ny nz curvature, ``cfg`` the fields of ``_lib.region_cfg``.
    The pair is an edge iff all three hold.  Needs no device."""
    L = _lib.load_hip()
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(m) for v, m in ((pi, 3), (ni, 4), (pj, 3), (nj, 4))]
    k = _lib.region_cfg(**cfg)
    out = [C.c_int(0), C.c_int(0), C.c_int(0)]
    rc = L.flimo_region_joined_host(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, C.byref(k), *(C.byref(o) for o in out))
    if rc != 0:
        raise FlimoError(f"flimo_region_joined_host failed ({rc})")
    return tuple(bool(o.value) for o in out)


def region_planes(listing):
    """One plane per listed region, from ``map_region_list``'s ``centroid`` and ``cov`` (both must be in ``listing``), on the host by
    ``np.linalg.eigh``: a dict of ``normal`` [nr, 3] float64 -- the eigenvector of the smallest eigenvalue, with
    ``flimo_map_normals``' sign rule without a viewpoint: its component of largest magnitude is positive, the lowest axis deciding
    between equal magnitudes --, ``d`` [nr] with n . x + d = 0 on the plane through the centroid (d = -n . centroid),
    ``eigenvalues`` [nr, 3] ascending, and ``rms`` [nr], the root mean square
    distance of the region's members to the plane (the square root of the smallest eigenvalue, clamped at 0).  Regions are few: no
    device eigen-solver is needed and the C ABI's floats stay exact."""
    cen = np.asarray(listing["centroid"], np.float64).reshape(-1, 3)
    cov = np.asarray(listing["cov"], np.float64).reshape(-1, 6)
    m = np.empty((len(cov), 3, 3))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 1], m[:, 1, 2], m[:, 2, 2] = cov.T
    m[:, 1, 0], m[:, 2, 0], m[:, 2, 1] = m[:, 0, 1], m[:, 0, 2], m[:, 1, 2]
    if len(m):
        w, v = np.linalg.eigh(m)
    else:
        w, v = np.zeros((0, 3)), np.zeros((0, 3, 3))
    n = v[:, :, 0].copy()
    lead = np.argmax(np.abs(n), axis=1)      # (the first of equal magnitudes: the lowest axis)
    n[n[np.arange(len(n)), lead] < 0.0] *= -1.0
    d = -(n[:, 0] * cen[:, 0] + (n[:, 1] * cen[:, 1] + n[:, 2] * cen[:, 2]))
    return dict(normal=n, d=d, eigenvalues=w, rms=np.sqrt(np.maximum(w[:, 0], 0.0)))


def plane_consensus(obj, nh, seed=0, top=4, **cfg):
    """The dominant planes of the stored points of ``obj`` (a ``HipCtx`` or a ``Localizer``): ``nh`` samples of
    ``corr_triplets(map_size, nh, seed)`` through ``obj.map_planes`` (``cfg``: the fields of ``_lib.plane_cfg``), the OK hypotheses
    ranked by ``inliers`` descending, then ``sum_sq`` ascending, then index.  Returns a dict of the best ``top``: plane [k, 4], sel
    (a list of ``PlaneSel`` ready for ``map_plane_mask`` / ``map_remove_plane``: the float32 normal, the sample's first point, the
    same dist, side 0), inliers, sum_sq, index [k] (the row of the hypothesis in tri), tri [k, 3]; and survivors: the number of OK
    hypotheses.  The ranking is RANSAC's; a least-squares refit of the winner is the caller's."""
    n_map = int(obj.map_size())
    tri = corr_triplets(n_map, nh, seed)
    out = obj.map_planes(tri, want=("plane",), **cfg)
    ok = np.nonzero(out["status"] == _lib.PLANE_OK)[0]
    order = np.lexsort((ok, out["sum_sq"][ok], -out["inliers"][ok].astype(np.int64)))[:max(int(top), 0)]
    best = ok[order]
    dist = float(_lib.plane_cfg(**cfg).dist)
    sel = []
    if best.size:
        pts = np.asarray(getattr(obj, "hip", obj).map_points(), np.float32).reshape(-1, 3)      # (the anchors: the samples' first points)
        sel = [_lib.plane_sel(out["plane"][j, 0:3].astype(np.float32), pts[tri[j, 0]], dist, 0) for j in best]
    return dict(plane=out["plane"][best], sel=sel, inliers=out["inliers"][best], sum_sq=out["sum_sq"][best], index=best.astype(np.int64),
                tri=tri[best], survivors=int(ok.size))


def corr_compatible_host(si, sj, di, dj, **cfg):
    """Whether the correspondences (si, di) and (sj, dj) can both be true, on the host (flimo_corr_compatible_host: the function
    the adjacency kernel of ``corr_graph`` calls); ``cfg``: the fields of ``_lib.corr_graph_cfg``.  It sees points, not indices."""
    L = _lib.load_hip()
    p = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (si, sj, di, dj)]
    k = _lib.corr_graph_cfg(**cfg)
    rc = L.flimo_corr_compatible_host(p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, p[3].ctypes.data, C.byref(k))
    if rc < 0:
        raise FlimoError(f"flimo_corr_compatible_host failed ({rc})")
    return bool(rc)


def corr_prune(obj, src, dst, min_core=None, **cfg):
    """The putative pairs worth sampling from: those in the innermost core of their consistency graph (``obj.corr_graph``: a
    ``HipCtx`` or a ``Localizer``; ``cfg``: the fields of ``_lib.corr_graph_cfg``).  True pairs are compatible with each other,
    false ones with few.  Returns a dict: keep -- the ascending int64 indices with core >= ``min_core`` (None: max_core) --, core,
    degree [m] and max_core.  No pairs: nothing is called, the arrays are empty and max_core is 0."""
    s = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    if s.shape[0] == 0:
        return dict(keep=np.zeros(0, np.int64), core=np.zeros(0, np.int32), degree=np.zeros(0, np.int32), max_core=0)
    out = obj.corr_graph(s, dst, want=(), **cfg)
    level = out["max_core"] if min_core is None else int(min_core)
    return dict(keep=np.nonzero(out["core"] >= level)[0].astype(np.int64), core=out["core"], degree=out["degree"], max_core=int(out["max_core"]))


def desc_pairs(ref_obj, qry_obj, q_desc, r_desc, ratio=0.9, mutual=True):
    """Putative pairs (qi, rj) -- two int64 arrays, ascending in qi -- between the rows of ``q_desc`` and ``r_desc`` by nearest
    descriptor, Lowe's ratio test and a mutual check.  ``ref_obj`` holds ``r_desc`` as its resident reference set, ``qry_obj`` holds
    ``q_desc`` (``desc_ref_set`` on a ``HipCtx`` or a ``Localizer``: the context whose map is the scan exists anyway, its FPFH came
    from it).  Forward: ``ref_obj.desc_match(q_desc, k=2)``; query i proposes (i, idx[i, 0]) when it has a neighbour, neither row of
    the pair is all-zero (points FPFH found no feature for), and -- float64 on the squared distances -- cnt < 2 or
    d0 <= ratio^2 * d1.  Mutual: the DISTINCT proposed reference rows go through ``qry_obj.desc_match(.., k=1)``; a pair stays when
    the answer is i.  That second call is nq-by-at-most-nq: no reverse pass over the map."""
    q = _lib.desc_rows(q_desc)
    r = _lib.desc_rows(r_desc)
    fwd = ref_obj.desc_match(q, k=2)
    idx, dist, cnt = fwd["idx"], fwd["dist"].astype(np.float64), fwd["cnt"]
    j0 = np.where(cnt >= 1, idx[:, 0], 0).astype(np.int64)
    keep = (cnt >= 1) & np.any(q != 0, axis=1)
    if r.shape[0]:
        keep &= np.any(r[j0] != 0, axis=1)
    keep &= (cnt < 2) | (dist[:, 0] <= (float(ratio) * float(ratio)) * dist[:, 1])
    qi = np.nonzero(keep)[0].astype(np.int64)
    rj = j0[qi]
    if mutual and qi.size:
        sel, inv = np.unique(rj, return_inverse=True)
        back = qry_obj.desc_match(r[sel], k=1)
        answer = np.where(back["cnt"] >= 1, back["idx"][:, 0], -1).astype(np.int64)
        stay = answer[inv] == qi
        qi, rj = qi[stay], rj[stay]
    return qi, rj


def relocalize(map_obj, scan_obj, fpfh=None, scan_fpfh=None, ratio=0.9, mutual=True, nh=4096, seed=0, top=8, corr=None, fitness_max_dist=1.0, align=None,
               x26_like=None, prune=None, keypoints=None, scan_keypoints=None, refine="plane", ndt=None, gicp=None):
    """A pose of a scan in a map from nothing but the two clouds -- plumbing over six calls, every parameter the caller's.
    ``map_obj`` (a ``HipCtx`` or a ``Localizer``) holds the map, and the scan (body frame) as its resident scan; ``scan_obj`` is a
    context whose MAP is that scan.  FPFH of both sides (``fpfh``: the fields of ``_lib.fpfh_cfg``; ``scan_fpfh``: the scan side's
    where they differ -- a viewpoint is in the frame of its cloud), ``desc_ref_set`` on both,
    ``desc_pairs(ratio, mutual)``, ``corr_consensus`` on the paired points (``nh``, ``seed``, ``top``, ``corr``: the fields of
    ``_lib.corr_cfg``), ``scan_fitness`` of the returned rows on ``map_obj`` ranked by ``fitness_cost`` at ``fitness_max_dist``,
    ``scan_align`` (``align``: its keyword arguments) of the best row.  Returns the dict of each stage: pairs (qi, rj), fpfh (the
    scan's rows, the map's), src, dst,
    consensus, fitness (inliers, sum_sqd, cost, x26: the rows in ranked order), align, and x26: the refined best row.
    ``prune``: None, or a dict of ``corr_prune``'s keyword arguments -- the pairs then go through ``corr_prune`` on ``map_obj``, and
    ``corr_consensus`` samples from ``src[keep]``, ``dst[keep]`` alone.  The returned pairs, src and dst stay the unpruned ones;
    ``prune`` is added to the result, the dict ``corr_prune`` returned, and ``consensus["tri"]`` then indexes the KEPT pairs:
    pair ``prune["keep"][t]`` of the unpruned ones.
    ``keypoints``: None, or a dict of the fields of ``_lib.keypoint_cfg`` (``scan_keypoints``: the scan side's where they differ) --
    both sides then run ``map_keypoints``, and ``desc_ref_set`` and ``desc_pairs`` see the keypoints' FPFH rows alone; FPFH itself is
    still formed for every point.  The returned pairs, src and dst are in the ORIGINAL indices; ``keypoints`` is added to the result:
    (the scan's ascending indices, the map's).
    ``refine``: "plane" (the default: ``scan_align``) or "ndt" -- the best row is then refined by ``ndt_align`` (``ndt``: its keyword
    arguments; ``slots`` is required and names models already built on ``map_obj`` with ``ndt_build``, coarse to fine) -- or "gicp":
    by ``gicp_align`` (``gicp``: its keyword arguments; ``map_obj`` already holds the model of ``gicp_build`` and the scan's
    covariances of ``scan_cov_set``)."""
    if refine not in ("plane", "ndt", "gicp"):
        raise ValueError(f"relocalize: refine must be 'plane', 'ndt' or 'gicp', not {refine!r}")
    fpfh, corr, align = dict(fpfh or {}), dict(corr or {}), dict(align or {})
    m_hip, s_hip = getattr(map_obj, "hip", map_obj), getattr(scan_obj, "hip", scan_obj)
    f_map = map_obj.map_fpfh(want=(), **fpfh)["fpfh"]
    f_scan = scan_obj.map_fpfh(want=(), **(fpfh if scan_fpfh is None else dict(scan_fpfh)))["fpfh"]
    if keypoints is None:
        kp = None
        map_obj.desc_ref_set(f_map)
        scan_obj.desc_ref_set(f_scan)
        qi, rj = desc_pairs(map_obj, scan_obj, f_scan, f_map, ratio=ratio, mutual=mutual)
    else:
        kp_map = map_obj.map_keypoints(want=(), **dict(keypoints))["index"]
        kp_scan = scan_obj.map_keypoints(want=(), **dict(keypoints if scan_keypoints is None else scan_keypoints))["index"]
        kp = (kp_scan, kp_map)
        k_scan, k_map = np.ascontiguousarray(f_scan[kp_scan]), np.ascontiguousarray(f_map[kp_map])
        map_obj.desc_ref_set(k_map)
        scan_obj.desc_ref_set(k_scan)
        qi, rj = desc_pairs(map_obj, scan_obj, k_scan, k_map, ratio=ratio, mutual=mutual)
        qi, rj = kp_scan[qi], kp_map[rj]
    src, dst = s_hip.map_points()[qi], m_hip.map_points()[rj]
    pruned = None if prune is None else corr_prune(map_obj, src, dst, **dict(prune))
    s_in, d_in = (src, dst) if pruned is None else (src[pruned["keep"]], dst[pruned["keep"]])
    cons = corr_consensus(map_obj, s_in, d_in, nh, seed=seed, top=top, x26_like=x26_like, **corr)
    inliers, sum_sqd = map_obj.scan_fitness(cons["x26"], max_dist=fitness_max_dist)
    cost = fitness_cost(inliers, sum_sqd, m_hip.scan_size(), fitness_max_dist)
    order = np.lexsort((np.arange(cost.size), cost))
    ranked = cons["x26"][order]
    if refine == "plane":
        aligned = scan_align(map_obj, ranked[:1], **align)
    elif refine == "ndt":
        aligned = ndt_align(map_obj, ranked[:1], **dict(ndt or {}))
    else:
        aligned = gicp_align(map_obj, ranked[:1], **dict(gicp or {}))
    out = dict(pairs=(qi, rj), fpfh=(f_scan, f_map), src=src, dst=dst, consensus=cons,
               fitness=dict(inliers=inliers[order], sum_sqd=sum_sqd[order], cost=cost[order], x26=ranked), align=aligned,
               x26=aligned["x26"][0] if ranked.shape[0] else None)
    if pruned is not None:
        out["prune"] = pruned
    if kp is not None:
        out["keypoints"] = kp
    return out


def sc_bin_host(p, cfg=None, frame12=None, **kw):
    """The Scan Context bin of ONE point on the host (flimo_sc_bin_host: the function the descriptor kernel calls): ``cfg`` a
    ``_lib.ScCfg`` or None with the fields of ``_lib.sc_cfg`` as keywords.  Returns (has, ring, sector, h); ring = sector = -1 and
    h = 0 for a point without a bin.  Needs no device."""
    L = _lib.load_hip()
    k, f = _lib._as_sc_cfg(cfg, kw), _lib._frame12(frame12)
    q = np.ascontiguousarray(p, dtype=np.float32).reshape(3)
    ring, sector, h = C.c_int(-1), C.c_int(-1), C.c_float(0.0)
    rc = L.flimo_sc_bin_host(q.ctypes.data, C.byref(k), None if f is None else f.ctypes.data, C.byref(ring), C.byref(sector), C.byref(h))
    if rc < 0:
        raise FlimoError(f"flimo_sc_bin_host failed ({rc})")
    return rc == 1, int(ring.value), int(sector.value), np.float32(h.value)


def sc_dist_host(a, b, min_cols=1, want_profile=False):
    """The Scan Context distance of ONE pair of descriptors [rings, sectors] on the host (flimo_sc_dist_host: the functions the
    kernels call).  Returns (have, dist float32, shift[, profile [sectors] float32: NaN for an excluded shift]); have is False, dist
    0 and shift -1 when every shift is excluded.  Needs no device."""
    L = _lib.load_hip()
    x, y = (np.ascontiguousarray(v, dtype=np.float32) for v in (a, b))
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError("sc_dist_host: two descriptors [rings, sectors] of one shape")
    dist, shift = C.c_float(0.0), C.c_int(-1)
    prof = np.full(x.shape[1], np.nan, np.float32) if want_profile else None
    rc = L.flimo_sc_dist_host(x.ctypes.data, y.ctypes.data, x.shape[0], x.shape[1], int(min_cols), C.byref(dist), C.byref(shift),
                              None if prof is None else prof.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_sc_dist_host failed ({rc})")
    out = (rc == 1, np.float32(dist.value), int(shift.value))
    return out + (prof,) if want_profile else out


def sc_guesses(x26_keyframes, idx, shift, sectors):
    """Pose guesses from ``sc_match``'s answer: one x26 row per (idx, shift) pair -- the keyframe's row ``x26_keyframes[idx]`` with
    its position, roll and pitch, and the yaw of the match: yaw_query = yaw_keyframe - shift * 2 pi / sectors, i.e. the keyframe's
    rotation with Rz(-shift * 2 pi / sectors) in front of it (float64; q = x26[3:7] as x y z w).  The descriptor carries no
    translation: the position is the keyframe's.  ``idx`` and ``shift`` of any one shape, every idx >= 0; returns [idx.size, 26]."""
    kf = np.asarray(x26_keyframes, np.float64).reshape(-1, 26)
    idx, shift = np.asarray(idx, np.int64).reshape(-1), np.asarray(shift, np.int64).reshape(-1)
    if idx.shape != shift.shape or np.any(idx < 0) or np.any(idx >= kf.shape[0]):
        raise ValueError("sc_guesses: idx and shift must pair up and name keyframes")
    x = np.array(kf[idx])
    half = -0.5 * shift.astype(np.float64) * (2.0 * math.pi / float(sectors))
    sz, cw = np.sin(half), np.cos(half)
    bx, by, bz, bw = x[:, 3], x[:, 4], x[:, 5], x[:, 6]
    q = np.stack([cw * bx - sz * by, cw * by + sz * bx, cw * bz + sz * bw, cw * bw - sz * bz], axis=1)
    x[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return x


def place_relocalize(obj, x26_keyframes, cfg, frame12=None, k=4, first=0, n=None, match=None, fitness_max_dist=1.0, align=None):
    """A pose of the resident scan in the map by place recognition -- plumbing over five calls.  ``obj`` (a ``HipCtx`` or a
    ``Localizer``) holds the map, the scan (body frame) as its resident scan, and a Scan Context database whose entry i was taken at
    ``x26_keyframes[i]``.  ``scan_context(cfg, frame12)`` of the scan, ``sc_match`` of it against the entries [first, first + n) for
    the best ``k`` (``match``: further keyword arguments of ``sc_match``), ``sc_guesses``, ``scan_fitness`` of the guesses ranked by
    ``fitness_cost`` at ``fitness_max_dist``, ``scan_align`` (``align``: its keyword arguments) of the best.  Returns the dict of
    each stage: desc, used, match, guesses (x26 rows in the match's order), fitness (inliers, sum_sqd, cost, x26, order: ranked),
    align, and x26: the refined best row, None when nothing matched."""
    hip = getattr(obj, "hip", obj)
    desc, used = obj.scan_context(cfg, frame12)
    m = obj.sc_match(desc, k=k, first=first, n=n, **dict(match or {}))
    cnt = int(m["cnt"][0])
    guesses = sc_guesses(x26_keyframes, m["idx"][0, :cnt], m["shift"][0, :cnt], desc.shape[1])
    out = dict(desc=desc, used=used, match=m, guesses=guesses, fitness=None, align=None, x26=None)
    if cnt == 0:
        return out
    inliers, sum_sqd = obj.scan_fitness(guesses, max_dist=fitness_max_dist)
    cost = fitness_cost(inliers, sum_sqd, hip.scan_size(), fitness_max_dist)
    order = np.lexsort((np.arange(cost.size), cost))
    ranked = guesses[order]
    aligned = scan_align(obj, ranked[:1], **dict(align or {}))
    out.update(fitness=dict(inliers=inliers[order], sum_sqd=sum_sqd[order], cost=cost[order], x26=ranked, order=order), align=aligned,
               x26=aligned["x26"][0])
    return out


def seg_move_host(T, p):
    """ONE stored point moved by ONE matrix on the host (flimo_seg_move_host: the function the move's kernel calls).  ``T``: 12
    float64, row-major 3 x 4; ``p``: 3 float32.  Returns float32 [3].  Needs no device."""
    L = _lib.load_hip()
    m = np.ascontiguousarray(T, dtype=np.float64).reshape(12)
    q, out = np.ascontiguousarray(p, dtype=np.float32).reshape(3), np.zeros(3, np.float32)
    rc = L.flimo_seg_move_host(m.ctypes.data, q.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise FlimoError(f"flimo_seg_move_host failed ({rc})")
    return out


def _pose_mats(x26):
    """[n, 26] state rows -> [n, 4, 4] float64: R of the normalised quaternion x26[3:7] (x y z w), t = x26[0:3]."""
    x = np.asarray(x26, np.float64).reshape(-1, 26)
    q = x[:, 3:7] / np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    M = np.zeros((x.shape[0], 4, 4))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = 2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)
    M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = 2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)
    M[:, :3, 3] = x[:, 0:3]
    M[:, 3, 3] = 1.0
    return M


def segment_corrections(x26_old, x26_new):
    """The matrices of ``map_correct`` from keyframe poses before and after an optimisation: row s = T_new[s] . T_old[s]^-1 as
    [n, 12] float64 (row-major 3 x 4, new world <- old world), from ``pos`` and the normalised ``rot`` of each row, all in float64:
    R = R_new R_old^T, t = t_new - R t_old."""
    A, B = _pose_mats(x26_old), _pose_mats(x26_new)
    if A.shape != B.shape:
        raise ValueError("segment_corrections: as many new poses as old ones")
    R = B[:, :3, :3] @ np.transpose(A[:, :3, :3], (0, 2, 1))
    t = B[:, :3, 3] - np.einsum("nij,nj->ni", R, A[:, :3, 3])
    return np.ascontiguousarray(np.concatenate([R, t[:, :, None]], axis=2).reshape(-1, 12))


def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _so3_log(R):
    """The rotation vector of R (float64), angle in [0, pi]."""
    c = min(1.0, max(-1.0, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * float(np.linalg.norm(w))      # sin(angle)
    th = math.atan2(s, c)
    if s > 1e-9:
        return w * (0.5 * th / s)
    if c > 0.0:
        return 0.5 * w                       # angle -> 0
    ax = np.sqrt(np.maximum(0.5 * (np.diag(R) + 1.0), 0.0))      # angle -> pi: the axis from the diagonal, signs from the largest entry's row
    k = int(np.argmax(ax))
    for j in range(3):
        if j != k and R[k, j] + R[j, k] < 0.0:
            ax[j] = -ax[j]
    return ax / np.linalg.norm(ax) * th


def _so3_jr_inv(phi):
    """Inverse of SO(3)'s right Jacobian at rotation vector phi: Log(Exp(phi) Exp(d)) = phi + Jr^-1 d + o(d)."""
    th = float(np.linalg.norm(phi))
    K = _hat(phi)
    a = 1.0 / 12.0 if th < 1e-4 else 1.0 / (th * th) - (1.0 + math.cos(th)) / (2.0 * th * math.sin(th))
    return np.eye(3) + 0.5 * K + a * (K @ K)


def _pg_edges(edges, n):
    out = []
    for e in edges:
        a, b, Z = int(e[0]), int(e[1]), np.asarray(e[2], np.float64).reshape(4, 4)
        w = np.ones(6) if len(e) < 4 or e[3] is None else np.asarray(e[3], np.float64).reshape(6)
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise ValueError("pose_graph_solve: an edge joins two different nodes of the graph")
        out.append((a, b, Z, w))
    return out


def pose_graph_residuals(M, edges):
    """Per edge (i, j, Z, w) of ``_pg_edges`` the residual of E = Z^-1 T_i^-1 T_j as (translation of E, rotation vector of E), with
    the pieces the Jacobians need: (r [6], R_E, R_a, t_a) where (R_a, t_a) = T_i^-1 T_j."""
    out = []
    for a, b, Z, _ in edges:
        Ri, Rj = M[a, :3, :3], M[b, :3, :3]
        Ra, ta = Ri.T @ Rj, Ri.T @ (M[b, :3, 3] - M[a, :3, 3])
        Rz = Z[:3, :3]
        Re, te = Rz.T @ Ra, Rz.T @ (ta - Z[:3, 3])
        out.append((np.concatenate([te, _so3_log(Re)]), Re, Ra, ta))
    return out


def pose_graph_solve(x26, edges, fixed=0, iters=50, tol=1e-10):
    """Pose-graph optimisation on the host, in float64 -- a helper like ``scan_align``'s Cholesky, nothing on the GPU.  ``x26``
    [n, 26]: the nodes (pos and rot are read and written, the rest is copied through); ``edges``: (i, j, Z) or (i, j, Z, w) with Z
    the measured T_i^-1 T_j as a 4 x 4 matrix and w six weights (translation then rotation; default 1).  Gauss-Newton on SE(3) with
    the body-frame perturbation of ``pose_retract`` (t += R drho, R <- R Exp(dphi)), dense normal equations, node ``fixed`` held.
    The cost is sum_e sum_k w_k r_k^2 with r = (translation, rotation vector) of Z^-1 T_i^-1 T_j; a step that would raise it is
    halved (at most 30 times), so the cost never rises.  Ends after ``iters`` steps, when a step's norm falls below ``tol``, or when
    no shorter step lowers the cost.  Returns a dict: x26 [n, 26], cost and grad (the cost and the gradient's norm at the start and
    after every step), iters (steps taken)."""
    x = np.array(np.asarray(x26, np.float64).reshape(-1, 26))
    n = x.shape[0]
    E = _pg_edges(edges, n)
    fixed = int(fixed)
    if not 0 <= fixed < n:
        raise ValueError("pose_graph_solve: `fixed` names no node")
    free = [k for k in range(n) if k != fixed]
    col = {k: 6 * c for c, k in enumerate(free)}

    def linearise(x):
        M = _pose_mats(x)
        H, g, cost = np.zeros((6 * len(free), 6 * len(free))), np.zeros(6 * len(free)), 0.0
        for (a, b, Z, w), (r, Re, Ra, ta) in zip(E, pose_graph_residuals(M, E)):
            cost += float(np.dot(w, r * r))
            Ji, Jj, Jri = np.zeros((6, 6)), np.zeros((6, 6)), _so3_jr_inv(r[3:6])
            RzT = Re @ Ra.T
            Ji[0:3, 0:3], Ji[0:3, 3:6], Ji[3:6, 3:6] = -RzT, RzT @ _hat(ta), -Jri @ Ra.T
            Jj[0:3, 0:3], Jj[3:6, 3:6] = Re, Jri
            for (p, Jp) in ((a, Ji), (b, Jj)):
                if p == fixed:
                    continue
                g[col[p]:col[p] + 6] += Jp.T @ (w * r)
                for (q, Jq) in ((a, Ji), (b, Jj)):
                    if q != fixed:
                        H[col[p]:col[p] + 6, col[q]:col[q] + 6] += Jp.T @ (w[:, None] * Jq)
        return H, g, cost

    def cost_of(x):
        return sum(float(np.dot(w, r * r)) for (_, _, _, w), (r, _, _, _) in zip(E, pose_graph_residuals(_pose_mats(x), E)))

    H, g, cost = linearise(x)
    costs, grads, steps = [cost], [float(np.linalg.norm(g))], 0
    for _ in range(int(iters)):
        if not free or not E:
            break
        try:
            dx = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            dx = -np.linalg.lstsq(H, g, rcond=None)[0]
        if not np.all(np.isfinite(dx)):
            break
        scale, trial = 1.0, None
        for _ in range(31):
            trial = np.array(x)
            for k in free:
                trial[k] = pose_retract(x[k], scale * dx[col[k]:col[k] + 6])
            if cost_of(trial) <= cost:
                break
            scale, trial = 0.5 * scale, None
        if trial is None:
            break
        x = trial
        H, g, cost = linearise(x)
        steps += 1
        costs.append(cost)
        grads.append(float(np.linalg.norm(g)))
        if scale * float(np.linalg.norm(dx)) < tol:
            break
    return dict(x26=x, cost=np.array(costs), grad=np.array(grads), iters=steps)


def loop_close(obj, x26_keyframes, edges, **solve):
    """Close a loop: ``pose_graph_solve(x26_keyframes, edges, **solve)``, then ``obj.map_correct(segment_corrections(old, new))``
    -- every stored point of segment s moves with keyframe s.  Convention: segment 0 is open from the start and holds keyframe 0's
    points; the caller calls ``map_segment_mark`` right before the first insert of each later keyframe, so segment ids, rows of
    ``x26_keyframes`` and ``sc_db_add_scan`` ids coincide.  ``obj``: a ``HipCtx`` or a ``Localizer`` (whose filter pose is then the
    caller's to set, ``set_x``).  Returns a dict: x26 (the new keyframe poses), changed (stored points whose bits changed), T (the
    matrices), solve (``pose_graph_solve``'s dict)."""
    old = np.asarray(x26_keyframes, np.float64).reshape(-1, 26)
    begin, stale = obj.map_segments()
    if not stale and begin.size - 1 != old.shape[0]:
        raise ValueError(f"loop_close: {old.shape[0]} keyframes for {begin.size - 1} segments")
    sol = pose_graph_solve(old, edges, **solve)
    T = segment_corrections(old, sol["x26"])
    return dict(x26=sol["x26"], changed=obj.map_correct(T), T=T, solve=sol)


ALIGN_RUNNING, ALIGN_FEW, ALIGN_SINGULAR = 0, 1, 2    # scan_align's status per pose: ran every iteration / too few valid pairs / H not positive definite


def sym6(H21):
    """[.., 21] upper triangles (row-major 00, 01 .. 05, 11 .. 55) -> the symmetric [.., 6, 6] matrices."""
    H21 = np.asarray(H21, np.float64)
    iu = np.triu_indices(6)
    M = np.zeros(H21.shape[:-1] + (6, 6))
    M[..., iu[0], iu[1]] = H21
    M[..., iu[1], iu[0]] = H21
    return M


def pose_retract(x26, xi):
    """The body-frame update of scan_linearize's perturbation on one state vector, in float64: t += R(q) drho, q <- q (x) Exp(dphi),
    renormalised (q = x26[3:7] as x y z w).  Everything else is copied through."""
    x = np.array(x26, np.float64)
    qx, qy, qz, qw = x[3:7] / np.linalg.norm(x[3:7])
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    x[0:3] += R @ np.asarray(xi[0:3], np.float64)
    phi = np.asarray(xi[3:6], np.float64)
    th = float(np.linalg.norm(phi))
    half = 0.5 * th
    s = 0.5 - th * th / 48.0 if th < 1e-6 else math.sin(half) / th      # sin(th / 2) / th
    dx, dy, dz, dw = s * phi[0], s * phi[1], s * phi[2], math.cos(half)
    q = np.array([qw * dx + qx * dw + qy * dz - qz * dy, qw * dy - qx * dz + qy * dw + qz * dx, qw * dz + qx * dy - qy * dx + qz * dw,
                  qw * dw - qx * dx - qy * dy - qz * dz])
    x[3:7] = q / np.linalg.norm(q)
    return x


def scan_align(obj, x26s, k=5, max_dist=1.0, min_pts=3, max_curv=0.05, iters=10, min_valid=30, linearize=None):
    """Refine pose hypotheses of the resident scan against the map by point-to-plane Gauss-Newton: the GPU linearises
    (``scan_linearize`` of ``obj``, a ``HipCtx`` or a ``Localizer``; or ``linearize(x26s)`` when given: any callable that returns
    that dict), the host solves.  Per iteration ONE call for all poses still running, a Cholesky factorisation of every 6 x 6
    system, H xi = -g, and ``pose_retract``.  A pose with fewer than ``min_valid`` valid pairs, or whose H is not positive definite,
    stops where it is.  The loop ends by the iteration count alone: neighbour sets may flip from one pass to the next, so a step
    norm need not fall below a tolerance.  Returns a dict: x26 [np, 26] (refined; all other entries copied through), valid and cost
    [np] of each pose's LAST linearisation (at the pose before its last step), iters [np] (steps taken), status [np]
    (ALIGN_RUNNING / ALIGN_FEW / ALIGN_SINGULAR)."""
    if linearize is None:
        linearize = lambda x: obj.scan_linearize(x, k, max_dist, min_pts, max_curv)
    x = np.array(np.asarray(x26s, np.float64).reshape(-1, 26))
    m = x.shape[0]
    valid, cost = np.zeros(m, np.int32), np.zeros(m)
    steps, status = np.zeros(m, np.int32), np.full(m, ALIGN_RUNNING, np.int32)
    for _ in range(int(iters)):
        run = np.nonzero(status == ALIGN_RUNNING)[0]
        if run.size == 0:
            break
        lin = linearize(x[run])
        valid[run], cost[run] = lin["valid"], lin["cost"]
        H, g = sym6(lin["H"]), np.asarray(lin["g"], np.float64)
        for a, j in enumerate(run):
            if valid[j] < min_valid:
                status[j] = ALIGN_FEW
                continue
            try:
                Lc = np.linalg.cholesky(H[a])
            except np.linalg.LinAlgError:
                status[j] = ALIGN_SINGULAR
                continue
            xi = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g[a]))
            if not np.all(np.isfinite(xi)):
                status[j] = ALIGN_SINGULAR
                continue
            x[j] = pose_retract(x[j], xi)
            steps[j] += 1
    return dict(x26=x, valid=valid, cost=cost, iters=steps, status=status)


def ndt_params(outlier_ratio, leaf):
    """PCL's Gaussian fit of the NDT likelihood (pcl::NormalDistributionsTransform::init / computeTransformation) for an outlier
    ratio and a leaf size: returns (d1, d2) -- a term scores -d1 * exp(-d2 / 2 * m).  c1 = 10 (1 - o), c2 = o / leaf^3,
    d3 = -log c2, d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 e^(-1/2) + c2) - d3) / d1)."""
    o, leaf = float(outlier_ratio), float(leaf)
    c1, c2 = 10.0 * (1.0 - o), o / (leaf * leaf * leaf)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def ndt_term_host(w, p, R, mean, evec, wgt, d2):
    """One NDT term on the host (flimo_ndt_term_host: the function the kernels of ``scan_ndt`` call, with libm's exp): ``w`` the
    float32 world point, ``p`` the float32 scan point, ``R`` [3, 3] the float32 rotation, (``mean``, ``evec`` [3, 3], ``wgt``) a
    cell of ``ndt_cells``.  Returns (live, m, e, sums [28]: H's 21, g's 6, the score).  Needs no device."""
    L = _lib.load_hip()
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(n) for v, n in ((w, 3), (p, 3), (R, 9))]
    b = [np.ascontiguousarray(v, dtype=np.float64).reshape(n) for v, n in ((mean, 3), (evec, 9), (wgt, 3))]
    out = np.zeros(30)
    rc = L.flimo_ndt_term_host(*(v.ctypes.data for v in a + b), float(d2), out.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_ndt_term_host failed ({rc})")
    return rc == 1, float(out[0]), float(out[1]), out[2:].copy()


def ndt_align(obj, x26s, slots, hood=7, outlier_ratio=0.55, iters=30, min_valid=30):
    """Refine pose hypotheses of the resident scan by NDT, coarse to fine: for each slot of ``slots`` in the given order (models
    built with ``ndt_build``, largest leaf first) ``scan_align`` runs ``iters`` Gauss-Newton steps on ``scan_ndt``'s normal
    equations at that model's ``d2`` (``ndt_params(outlier_ratio, leaf)``), starting where the previous slot ended.  Returns
    ``scan_align``'s dict of the LAST slot -- cost is -score, the sum of e negated --, and ``stages``: the dict of every slot."""
    x = np.array(np.asarray(x26s, np.float64).reshape(-1, 26))
    stages = []
    for slot in slots:
        d2 = ndt_params(outlier_ratio, obj.ndt_info(slot)["leaf"])[1]

        def linearize(xs, _slot=slot, _d2=d2):
            lin = obj.scan_ndt(_slot, xs, _d2, hood=hood)
            lin["cost"] = -lin["score"]
            return lin
        stages.append(scan_align(obj, x, iters=iters, min_valid=min_valid, linearize=linearize))
        x = stages[-1]["x26"]
    if not stages:
        raise ValueError("ndt_align: no slots")
    return dict(stages[-1], stages=stages)


def gicp_eigen_host(cov6):
    """The eigen-pairs ``gicp_regularize_host`` works from (flimo_gicp_eigen_host: the Jacobi of the kernels, on the host): returns
    (l [3] ascending, v [3, 3]: row k the unit vector of l[k]).  Needs no device."""
    L = _lib.load_hip()
    c = np.ascontiguousarray(cov6, dtype=np.float64).reshape(6)
    out = np.zeros(12)
    rc = L.flimo_gicp_eigen_host(c.ctypes.data, out.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_gicp_eigen_host failed ({rc})")
    return out[:3].copy(), out[3:].reshape(3, 3).copy()


def gicp_regularize_host(cov6, rule=_lib.GICP_PLANE, eps=1e-3):
    """One regularised covariance on the host (flimo_gicp_regularize_host: the function ``gicp_build``'s kernel calls): ``cov6`` =
    xx xy xz yy yz zz of a neighbourhood.  Returns (has, out [6]); six NaN and False where there is no covariance (a non-finite
    number, or no positive eigenvalue).  Needs no device."""
    L = _lib.load_hip()
    c = np.ascontiguousarray(cov6, dtype=np.float64).reshape(6)
    out = np.zeros(6)
    rc = L.flimo_gicp_regularize_host(c.ctypes.data, int(rule), float(eps), out.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_gicp_regularize_host failed ({rc})")
    return rc == 1, out


def gicp_term_host(w, b, p, R, CA, CB):
    """One GICP term on the host (flimo_gicp_term_host: the function the kernel of ``scan_gicp`` calls): ``w`` the float32 world
    point, ``b`` the float32 stored point, ``p`` the float32 scan point, ``R`` [3, 3] the float32 rotation, ``CA`` / ``CB`` [6] the
    scan point's and the stored point's covariance.  Returns (live, m, det, sums [28]: H's 21, g's 6, the cost).  Needs no device."""
    L = _lib.load_hip()
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(n) for v, n in ((w, 3), (b, 3), (p, 3), (R, 9))]
    c = [np.ascontiguousarray(v, dtype=np.float64).reshape(6) for v in (CA, CB)]
    out = np.zeros(30)
    rc = L.flimo_gicp_term_host(*(v.ctypes.data for v in a + c), out.ctypes.data)
    if rc < 0:
        raise FlimoError(f"flimo_gicp_term_host failed ({rc})")
    return rc == 1, float(out[0]), float(out[1]), out[2:].copy()


def gicp_covs(scan_obj, xyz=None, k=20, max_dist=float("inf"), min_pts=3, rule=_lib.GICP_PLANE, eps=1e-3):
    """The covariances ``scan_cov_set`` takes, for the points ``xyz`` [n, 3] of a scan (body frame): ``scan_obj`` is a context whose
    MAP is that scan (``map_config(downsample=False)``, as for the scan's FPFH rows); per point the covariance of its ``k`` nearest
    there (``normals``; ``xyz`` None: the stored points themselves, ``normals_range``), then ``gicp_regularize_host`` of every row.
    Returns float64 [n, 6]; a point with fewer than max(3, min_pts) neighbours keeps its NaN row."""
    if xyz is None:
        cov = getattr(scan_obj, "normals_range", None) or scan_obj.map_normals_range
        cov = cov(0, scan_obj.map_size(), k, max_dist, min_pts, want=("cov",))["cov"]
    else:
        cov = (getattr(scan_obj, "normals", None) or scan_obj.map_normals)(xyz, k, max_dist, min_pts, want=("cov",))["cov"]
    out = np.full(cov.shape, np.nan)
    for i in np.nonzero(np.all(np.isfinite(cov), axis=1))[0]:
        out[i] = gicp_regularize_host(cov[i], rule, eps)[1]
    return out


def gicp_align(obj, x26s, max_dist=1.0, iters=10, min_valid=30):
    """Refine pose hypotheses of the resident scan by GICP: ``scan_align`` on ``scan_gicp``'s normal equations -- ``iters``
    Gauss-Newton steps, each with the nearest stored points and the weights (CB + R CA R^T)^-1 of its own pose.  ``obj`` holds the
    model (``gicp_build``) and the scan's covariances (``scan_cov_set``).  Returns ``scan_align``'s dict; cost is the sum of m."""
    return scan_align(obj, x26s, iters=iters, min_valid=min_valid, linearize=lambda xs: obj.scan_gicp(xs, max_dist))


def eskf_update_fixed(x26, P, H, h, max_iters=3, limits=None, R=0.001, D=5.0):
    L = load_host()
    x = np.ascontiguousarray(x26, dtype=np.float64).copy()
    Pm = np.ascontiguousarray(P, dtype=np.float64).reshape(-1).copy()
    H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 12)
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
    lim = np.full(23, 1e-3) if limits is None else np.ascontiguousarray(limits, dtype=np.float64)
    n = C.c_int(0)
    L.flimo_eskf_update_fixed(x, Pm, H.reshape(-1) if H.size else np.zeros(1), h if h.size else np.zeros(1), H.shape[0],
                              max_iters, lim, R, D, C.byref(n))
    return x, Pm.reshape(23, 23), n.value


def ieskf_gj12_host(op, items):
    """The host filter's own elimination (flimo_host::inverse_gj / solve_gj, n = 12) on a batch: ``op`` _lib.IK_GJ12_INVERSE
    (items [n, 144] -> [n, 145]) or _lib.IK_GJ12_SOLVE ([n, 156] -> [n, 13]); the last column is ``ok``."""
    L = load_host()
    a, no = _lib.ik_items(op, items)
    out = np.zeros((a.shape[0], no))
    if a.shape[0]:
        rc = L.flimo_ieskf_gj12_host(int(op), a.reshape(-1), a.shape[0], out.reshape(-1))
        if rc != 0:
            raise FlimoError(f"flimo_ieskf_gj12_host({op}) failed ({rc})")
    return out


def ieskf_run_fixed_host(x26, P, limits, partials, R=0.001, D=5.0, max_iter=3):
    """The host twin of ``HipCtx.ieskf_run_fixed`` (flimo_ieskf_run_fixed_host): the host filter on the same per-iteration sums.
    Returns a dict: log (per completed pass a dict M, HTH, HTh, dx, x_after, t: the filter's own count so far), x, P, it (the iteration the loop ended in), t,
    passes."""
    L = load_host()
    x, Pm, lim, part = _lib.ik_fixed_args(x26, P, limits, partials)
    lg = np.zeros((int(max_iter) + 1, _lib.IK_HLOG_N))
    n = C.c_int(0)
    xo, Po = np.zeros(26), np.zeros(529)
    loop = (C.c_int * 3)()
    rc = L.flimo_ieskf_run_fixed_host(x, Pm, lim, float(R), float(D), int(max_iter), part.shape[0], part.reshape(-1), lg.reshape(-1),
                                      C.byref(n), xo, Po, loop)
    if rc != 0:
        raise FlimoError(f"flimo_ieskf_run_fixed_host failed ({rc})")
    log = [dict(M=int(r[0]), HTH=r[1:145].reshape(12, 12).copy(), HTh=r[145:157].copy(), dx=r[157:180].copy(), x_after=r[180:206].copy(), t=int(r[206]))
           for r in lg[:n.value]]
    return dict(log=log, x=xo, P=Po.reshape(23, 23), it=int(loop[0]), t=int(loop[1]), passes=int(loop[2]))


def eigen_solver6(A):
    """The host filter's restatement of Eigen::EigenSolver<Matrix6d>: (eigenvalues real, imag, eigenvector real parts as columns)."""
    L = load_host()
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(36)
    wr = np.zeros(6); wi = np.zeros(6); V = np.zeros(36)
    L.flimo_host_eigen_solver6(A, wr, wi, V)
    return wr, wi, V.reshape(6, 6)


def eskf_predict(x26, P, dt, Qdiag, acc, gyro):
    L = load_host()
    x = np.ascontiguousarray(x26, dtype=np.float64).copy()
    Pm = np.ascontiguousarray(P, dtype=np.float64).reshape(-1).copy()
    L.flimo_eskf_predict(x, Pm, float(dt), np.ascontiguousarray(Qdiag, dtype=np.float64),
                         np.ascontiguousarray(acc, dtype=np.float64), np.ascontiguousarray(gyro, dtype=np.float64))
    return x, Pm.reshape(23, 23)
