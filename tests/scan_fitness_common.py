"""Shared helpers of the scan-fitness tests (flimo_scan_fitness): the poses, the standard scene and the yardstick.

The yardstick of a pose is what the call replaces, restated: the world points of the scan (on the GPU: the existing
``ctx.scan_to_world``; without one: ``world_points`` below, the same float32 arithmetic in numpy), their nearest stored point by
``knn_k_common.brute_knn(w, map, 1, max_dist)``, the count of the non-empty queries and ``math.fsum`` of their float32 distances."""
import math
from multiprocessing.pool import ThreadPool

import numpy as np

from fast_limo_amd import synth
from knn_k_common import brute_knn

INF = float("inf")
N_MAP, N_SCAN, L_BOX, N_BATCHES = 20000, 1024, 10.0, 4
SHIFTS = (-1.0, -0.5, 0.0, 0.5, 1.0)          # dx, dy [m]
YAWS = (-10.0, -5.0, 0.0, 5.0, 10.0)          # [deg]
TRUE_POSE = (len(SHIFTS) * len(YAWS) + len(YAWS) + 1) * 2      # index of the undisplaced pose among standard_poses(): 62


def quat_xyzw(R):
    """Unit quaternion (x, y, z, w) of a rotation matrix whose angle is well below 180 degrees."""
    w = 0.5 * math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
    return np.float64([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def x26_of(t=synth.T_STAR_T, rpy_deg=synth.T_STAR_RPY_DEG):
    """The filter's state vector for a pose: pos, rot (x y z w); identity extrinsics; everything else 0."""
    x = np.zeros(26)
    x[0:3] = t
    x[3:7] = quat_xyzw(synth.rpy_to_R(*[math.radians(a) for a in rpy_deg]))
    x[10] = 1.0
    return x


def displaced(dx=0.0, dy=0.0, dz=0.0, dyaw_deg=0.0):
    t, r = synth.T_STAR_T, synth.T_STAR_RPY_DEG
    return x26_of((t[0] + dx, t[1] + dy, t[2] + dz), (r[0], r[1], r[2] + dyaw_deg))


def standard_poses():
    """[125, 26]: the true pose T* displaced by dx, dy in SHIFTS and yaw in YAWS; row TRUE_POSE is T* itself."""
    return np.stack([displaced(dx, dy, 0.0, yaw) for dx in SHIFTS for dy in SHIFTS for yaw in YAWS])


def standard_batches():
    """synth.box_world_map(20000, 10.0, 1), fed in four batches (the insert rule drops points of the later ones)."""
    return np.array_split(synth.box_world_map(N_MAP, L_BOX, 1), N_BATCHES)


def standard_scan(n=N_SCAN):
    return np.ascontiguousarray(synth.box_world_scan_random(n, L_BOX, 2)[:, :3])


def pose_rt(x26):
    """The 3 x 4 float32 matrix of State::get_RT as pose_from_x26 forms it (Eigen's toRotationMatrix on the float32 casts)."""
    f = np.float32
    p = [f(v) for v in x26[0:3]]
    q = [f(v) for v in x26[3:7]]
    two = f(2.0)
    tx, ty, tz = two * q[0], two * q[1], two * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    one = f(1.0)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy, p[0]],
                     [txy + twz, one - (txx + tzz), tyz - twx, p[1]],
                     [txz - twy, tyz + twx, one - (txx + tyy), p[2]]], np.float32)


def world_points(x26, scan):
    """transform_kernel in numpy: c0*x + (c1*y + (c2*z + c3)), float32, nothing contracted."""
    M = pose_rt(x26)
    s = np.asarray(scan, np.float32)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([M[r, 0] * x + (M[r, 1] * y + (M[r, 2] * z + M[r, 3])) for r in range(3)], axis=1).astype(np.float32)


def _full(w, mp, max_dist):
    """brute_knn(w, mp, 1, max_dist) over the whole map, the rows cut into slices for a pool of threads (numpy releases the lock)."""
    cuts = list(range(0, w.shape[0], 256))
    with ThreadPool(min(16, max(len(cuts), 1))) as pool:
        parts = pool.map(lambda a: brute_knn(w[a:a + 256], mp, 1, max_dist, chunk=64), cuts)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def nearest(w, mp, max_dist, cell=2.5, margin=1.5):
    """knn_k_common.brute_knn(w, mp, 1, max_dist) as (nn_sqd [m] with -1 for an empty query, nn_idx [m] with -1), without its
    m x |map| cost.  The queries are grouped by the cube of edge `cell` they lie in, and brute_knn runs per group over the stored
    points inside that cube grown by `margin` (in ascending index, so ties fall as over the whole map).  A stored point outside the
    grown cube is farther than `margin` from every query of the group, and its float32 squared distance -- a few 2^-24 off -- is above
    safe = (margin * (1 - 1e-3))^2.  So a group's result stands where the distance found is <= safe, and an empty result stands
    where the gate's square is <= safe; every other query is put to brute_knn over the whole map."""
    m = w.shape[0]
    nn_sqd, nn_idx = np.full(m, -1, np.float32), np.full(m, -1, np.int32)
    if mp.shape[0] == 0 or m == 0:
        return nn_sqd, nn_idx
    safe = np.float32((margin * (1.0 - 1e-3)) ** 2)
    with np.errstate(over="ignore"):
        gate_inside = np.float32(max_dist) * np.float32(max_dist) <= safe
    w64, mp64 = w.astype(np.float64), mp.astype(np.float64)
    near = np.isfinite(w64).all(1) & (np.abs(w64).max(1) < 1.0e6)
    cells = np.floor(w64[near] / cell).astype(np.int64)
    uniq, inv = np.unique(cells, axis=0, return_inverse=True)
    rows_near = np.nonzero(near)[0]
    order = np.argsort(inv.reshape(-1), kind="stable")
    bounds = np.searchsorted(inv.reshape(-1)[order], np.arange(len(uniq) + 1))
    settled = np.zeros(m, bool)

    def group(g):
        rows = rows_near[order[bounds[g]:bounds[g + 1]]]
        lo, hi = uniq[g] * cell - margin, (uniq[g] + 1) * cell + margin
        cand = np.nonzero(((mp64 >= lo) & (mp64 <= hi)).all(1))[0]
        if cand.size == 0:
            settled[rows] = gate_inside
            return
        idx, sqd, cnt = brute_knn(w[rows], mp[cand], 1, max_dist, chunk=64)
        has = cnt == 1
        ok = has & (sqd[:, 0] <= safe)
        nn_sqd[rows[ok]] = sqd[ok, 0]
        nn_idx[rows[ok]] = cand[idx[ok, 0]]
        settled[rows] = ok | (~has & gate_inside)

    with ThreadPool(16) as pool:
        pool.map(group, range(len(uniq)))
    rest = np.nonzero(~settled)[0]
    if rest.size:
        idx, sqd, cnt = _full(w[rest], mp, max_dist)
        has = cnt == 1
        nn_sqd[rest[has]] = sqd[has, 0]
        nn_idx[rest[has]] = idx[has, 0]
    return nn_sqd, nn_idx


def yardstick(worlds, mp, max_dist):
    """For a list of poses' world points [n, 3]: (inliers [np], math.fsum of the float32 distances [np], nn_sqd [np, n], nn_idx [np, n])."""
    k = len(worlds)
    n = worlds[0].shape[0] if k else 0
    nn_sqd, nn_idx = nearest(np.concatenate(worlds) if k else np.zeros((0, 3), np.float32), mp, max_dist)
    nn_sqd, nn_idx = nn_sqd.reshape(k, n), nn_idx.reshape(k, n)
    has = nn_idx >= 0
    return (has.sum(1).astype(np.int32), np.array([math.fsum(float(v) for v in nn_sqd[j][has[j]]) for j in range(k)], np.float64),
            nn_sqd, nn_idx)


def sum_bound(n, fsum):
    """|S - fsum| of any summation order of n non-negative float64 terms: each of the n - 1 additions rounds a partial sum that is at
    most the total, by at most 2^-53 of it -- n * 2^-52 * fsum covers it twice over (and fsum's own rounding)."""
    return n * 2.0 ** -52 * fsum


def check(got, ref, n, tag="", want_nn=True):
    """Inliers, nn_idx and the bits of nn_sqd with no tolerance; sum_sqd within sum_bound of fsum."""
    np.testing.assert_array_equal(got[0], ref[0], err_msg=f"{tag}: inliers")
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    for j in range(len(ref[1])):
        assert abs(got[1][j] - ref[1][j]) <= sum_bound(n, ref[1][j]), f"{tag}: sum_sqd of pose {j}: {got[1][j]!r} against fsum {ref[1][j]!r}"
    if want_nn:
        assert got[2].dtype == np.float32 and got[3].dtype == np.int32
        np.testing.assert_array_equal(got[2].view(np.uint32), ref[2].view(np.uint32), err_msg=f"{tag}: nn_sqd bits")
        np.testing.assert_array_equal(got[3], ref[3], err_msg=f"{tag}: nn_idx")

