"""Shared helpers of the radius-search tests: numpy brute force with the call's float32 arithmetic, the reference's traversal
(tests/radius_ref/radius_ref.cpp, compiled on the fly against the oracle's octree) behind ctypes, and the scenes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from fast_limo_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (0.0, 0.05, 0.3, 1.0, 3.0, 10.0)


def sqdist_f32(q, pts):
    """[nq, n] squared distances as the call computes them: float32, dx*dx + (dy*dy + dz*dz), nothing contracted."""
    q = np.asarray(q, np.float32)
    pts = np.asarray(pts, np.float32)
    dx = q[:, None, 0] - pts[None, :, 0]
    dy = q[:, None, 1] - pts[None, :, 1]
    dz = q[:, None, 2] - pts[None, :, 2]
    return dx * dx + (dy * dy + dz * dz)


def brute_force_multi(q, pts, radii, chunk=64):
    """Per radius the CSR (offsets, idx ascending per query, sqd) of the points with float32 squared distance <
    float32(radius)^2 (strict); the distances are evaluated once for all radii."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore"):
        r2 = [np.float32(np.float32(r) * np.float32(r)) for r in radii]
    counts = [np.zeros(q.shape[0], np.int64) for _ in radii]
    idx, sqd = [[] for _ in radii], [[] for _ in radii]
    for a in range(0, q.shape[0], chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            d = sqdist_f32(q[a:a + chunk], pts)
            for k, t in enumerate(r2):
                m = d < t
                qi, pi = np.nonzero(m)               # row-major: per query, ascending index
                counts[k][a:a + chunk] = m.sum(1)
                idx[k].append(pi.astype(np.int32))
                sqd[k].append(d[qi, pi])
    out = []
    for k in range(len(radii)):
        off = np.zeros(q.shape[0] + 1, np.uint64)
        off[1:] = np.cumsum(counts[k])
        out.append((off, np.concatenate(idx[k]) if idx[k] else np.zeros(0, np.int32),
                    np.concatenate(sqd[k]) if sqd[k] else np.zeros(0, np.float32)))
    return out


def brute_force(q, pts, radius, chunk=64):
    return brute_force_multi(q, pts, [radius], chunk)[0]


def sorted_order(off, idx, sqd):
    """Brute-force results (idx ascending per query) in the order of FLIMO_RADIUS_SORTED: per query by (distance bits, index)."""
    qid = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    o = np.lexsort((idx, bits(sqd), qid))
    return idx[o], sqd[o]


def by_index(off, idx, *more):
    """The results of every query re-ordered ascending by index (the unsorted form has no promised order)."""
    n = len(off) - 1
    qid = np.repeat(np.arange(n), np.diff(off).astype(np.int64))
    o = np.lexsort((idx, qid))
    return (idx[o],) + tuple(m[o] for m in more)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_batches(n_batches, per_batch, L=25.0, seed=100, sigma=0.01):
    """A box-world map in batches: fed one by one, the insert rule drops points of later batches."""
    return [synth.box_world_map(per_batch, L, seed + i, sigma=sigma) for i in range(n_batches)]


def query_mix(mp, rs, n_near=3000, n_air=500, n_far=50, n_on=50, L=25.0):
    """The mix of test_knn_bit_exact: near the surfaces, in the air, 500 m outside, exactly on map points."""
    return np.concatenate([
        mp[rs.choice(mp.shape[0], n_near)] + rs.normal(0, 0.2, (n_near, 3)).astype(np.float32),
        rs.uniform(-L, L, (n_air, 3)).astype(np.float32),
        rs.uniform(-L, L, (n_far, 3)).astype(np.float32) + np.float32(500.0),
        mp[:n_on],
    ]).astype(np.float32)


class RadiusRef:
    """The reference's radiusSearch restated over the oracle's octree (tests/radius_ref/radius_ref.cpp)."""
    _lib = None
    _dir = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            cls._dir = tempfile.TemporaryDirectory()
            so = os.path.join(cls._dir.name, "libradius_ref.so")
            r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"),
                                os.path.join(ROOT, "tests", "radius_ref", "radius_ref.cpp"), "-o", so],
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-4000:]
            L = C.CDLL(so)
            L.rr_create.restype = C.c_void_p
            L.rr_create.argtypes = [C.c_float, C.c_int]
            L.rr_destroy.argtypes = [C.c_void_p]
            L.rr_update.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
            L.rr_size.restype = C.c_uint64
            L.rr_size.argtypes = [C.c_void_p]
            L.rr_points.argtypes = [C.c_void_p, C.c_void_p]
            L.rr_radius_search.restype = C.c_uint64
            L.rr_radius_search.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p, C.POINTER(C.c_uint64)]
            L.rr_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            cls._lib = L
        return cls._lib

    def __init__(self, min_extent=0.2, downsample=True):
        self._L = self.lib()
        self._h = self._L.rr_create(float(min_extent), int(downsample))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rr_destroy(self._h)
            self._h = None

    def update(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._L.rr_update(self._h, xyz.ctypes.data, xyz.shape[0])

    def size(self):
        return int(self._L.rr_size(self._h))

    def points(self):
        out = np.empty((max(self.size(), 1), 3), np.float32)
        self._L.rr_points(self._h, out.ctypes.data)
        return out[:self.size()]

    def radius_search(self, q, radius):
        """(offsets, xyz, sqd, results that came through the whole-octant shortcut)."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        off = np.zeros(q.shape[0] + 1, np.uint64)
        sc = C.c_uint64(0)
        n = int(self._L.rr_radius_search(self._h, q.ctypes.data, q.shape[0], float(radius), off.ctypes.data, C.byref(sc)))
        xyz = np.empty((max(n, 1), 3), np.float32)
        sqd = np.empty(max(n, 1), np.float32)
        self._L.rr_results(self._h, xyz.ctypes.data, sqd.ctypes.data)
        return off, xyz[:n], sqd[:n], int(sc.value)


class PointIds:
    """Maps xyz rows to the number of their distinct value among a point set (checked, not assumed: a row that is not in the set,
    or two distinct rows with one hash, fail)."""

    def __init__(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        h = self._hash(pts)
        o = np.argsort(h, kind="stable")
        self._h = h[o]
        self._p = pts[o]
        first = np.ones(len(h), bool)
        first[1:] = self._h[1:] != self._h[:-1]
        same_row = np.all(bits(self._p[1:]) == bits(self._p[:-1]), axis=1)
        assert np.all(first[1:] | same_row), "two distinct points share a hash"
        self._uid = np.cumsum(first) - 1
        self.n = int(self._uid[-1]) + 1 if len(h) else 0

    @staticmethod
    def _hash(p):
        b = bits(p).astype(np.uint64)
        with np.errstate(over="ignore"):
            return (b[:, 0] * np.uint64(0x9E3779B97F4A7C15)) ^ (b[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F)) ^ (b[:, 2] * np.uint64(0x165667B19E3779F9))

    def ids(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        if xyz.shape[0] == 0:
            return np.zeros(0, np.int64)
        at = np.searchsorted(self._h, self._hash(xyz))
        assert np.all(at < len(self._h)), "a result is not a stored point"
        assert np.array_equal(bits(self._p[at]), bits(xyz)), "a result is not a stored point"
        return self._uid[at].astype(np.int64)


def disagreeing_queries(ids, off_a, xyz_a, sqd_a, off_b, xyz_b, sqd_b):
    """Number of queries whose results differ as multisets of (x, y, z) or in a distance's bits.  ids: PointIds of the stored points."""
    nq = len(off_a) - 1
    ca, cb = np.diff(off_a).astype(np.int64), np.diff(off_b).astype(np.int64)
    bad = ca != cb
    if not bad.any():
        qa = np.repeat(np.arange(nq), ca)
        ka, kb = qa * ids.n + ids.ids(xyz_a), qa * ids.n + ids.ids(xyz_b)
        oa, ob = np.argsort(ka, kind="stable"), np.argsort(kb, kind="stable")
        row_bad = (ka[oa] != kb[ob]) | (bits(sqd_a)[oa] != bits(sqd_b)[ob])
        bad = np.zeros(nq, bool)
        bad[qa[oa][row_bad]] = True
    return int(bad.sum())
