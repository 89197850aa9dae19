"""Shared helpers of the correspondence tests (flimo_corr_poses): the definition of include/flimo_c.h restated in numpy.

Steps 1 - 4 (edges, the two tests, TRIAD, Shepperd) are float64 array arithmetic on the float32 inputs widened, written term by term
in the header's association -- no ``@``, no ``einsum``, no ``sum`` --, for all hypotheses at once; numpy's elementwise + - * / sqrt
are IEEE operations and never contracted.  Step 5 reuses scan_fitness_common.pose_rt / world_points (the float32 matrix and world
points flimo_scan_fitness sees) and ends in the 256-partial tree of the header."""
import math

import numpy as np

import scan_fitness_common as sf

OK, DEGENERATE, REJECTED = 0, 1, 2
RED = 256


def sq(v):
    """v.x*v.x + (v.y*v.y + v.z*v.z) over the last axis."""
    return v[..., 0] * v[..., 0] + (v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def cross(a, b):
    """(y z' - z y', z x' - x z', x y' - y x')."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def frame(p):
    """p [.., 3 points, 3] float64 -> u1, u2, u3 [.., 3]."""
    e1, e2 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :]
    u1 = e1 / np.sqrt(sq(e1))[..., None]
    cr = cross(u1, e2)
    u3 = cr / np.sqrt(sq(cr))[..., None]
    return u1, cross(u3, u1), u3


def solve_points(S, D, edge_sim, min_edge):
    """Steps 1 - 4 and the matrix of step 5 for triangles given by their points: S, D [nh, 3 points, 3] float32.  Returns (status
    [nh], pose7 [nh, 7] float64, rt [nh, 3, 4] float32, branch [nh]: Shepperd's branch 0..3); pose7 and rt NaN unless OK."""
    S = np.asarray(S, np.float32).reshape(-1, 3, 3).astype(np.float64)
    D = np.asarray(D, np.float32).reshape(-1, 3, 3).astype(np.float64)
    nh = S.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        edges = lambda p: np.stack([sq(p[:, 1] - p[:, 0]), sq(p[:, 2] - p[:, 1]), sq(p[:, 0] - p[:, 2])], axis=1)
        es, ed = edges(S), edges(D)
        min2 = float(np.float32(min_edge)) * float(np.float32(min_edge))
        s2 = float(np.float32(edge_sim)) * float(np.float32(edge_sim))
        degenerate = ~((es >= min2).all(1) & (ed >= min2).all(1))
        rejected = ~(np.fmin(es, ed) >= s2 * np.fmax(es, ed)).all(1)
        u1s, u2s, u3s = frame(S)
        u1d, u2d, u3d = frame(D)
        R = np.empty((nh, 3, 3))
        for r in range(3):
            for c in range(3):
                R[:, r, c] = u1d[:, r] * u1s[:, c] + (u2d[:, r] * u2s[:, c] + u3d[:, r] * u3s[:, c])
        cs = ((S[:, 0] + S[:, 1]) + S[:, 2]) / 3.0
        cd = ((D[:, 0] + D[:, 1]) + D[:, 2]) / 3.0
        t = np.stack([cd[:, r] - (R[:, r, 0] * cs[:, 0] + (R[:, r, 1] * cs[:, 1] + R[:, r, 2] * cs[:, 2])) for r in range(3)], axis=1)
        singular = ~(np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1))
        tr = R[:, 0, 0] + (R[:, 1, 1] + R[:, 2, 2])
        branch = np.argmax(np.nan_to_num(np.stack([tr, R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], axis=1), nan=-np.inf), axis=1)      # the first on a tie
        a21, a02, a10 = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]      # antisymmetric parts
        s01, s02, s12 = R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]      # symmetric parts
        w0 = 0.5 * np.sqrt(1.0 + tr)
        f0 = 0.25 / w0
        x1 = 0.5 * np.sqrt(1.0 + ((R[:, 0, 0] - R[:, 1, 1]) - R[:, 2, 2]))
        f1 = 0.25 / x1
        y2 = 0.5 * np.sqrt(1.0 + ((R[:, 1, 1] - R[:, 0, 0]) - R[:, 2, 2]))
        f2 = 0.25 / y2
        z3 = 0.5 * np.sqrt(1.0 + ((R[:, 2, 2] - R[:, 0, 0]) - R[:, 1, 1]))
        f3 = 0.25 / z3
        quats = np.stack([np.stack([a21 * f0, a02 * f0, a10 * f0, w0], axis=1),      # x y z w per branch
                          np.stack([x1, s01 * f1, s02 * f1, a21 * f1], axis=1),
                          np.stack([s01 * f2, y2, s12 * f2, a02 * f2], axis=1),
                          np.stack([s02 * f3, s12 * f3, z3, a10 * f3], axis=1)], axis=1)
        q = quats[np.arange(nh), branch]
    status = np.full(nh, OK, np.int32)
    status[singular] = DEGENERATE
    status[rejected] = REJECTED
    status[degenerate] = DEGENERATE
    pose = np.concatenate([t, q], axis=1)
    pose[status != OK] = np.nan
    rt = np.full((nh, 3, 4), np.nan, np.float32)
    for j in np.nonzero(status == OK)[0]:
        rt[j] = sf.pose_rt(pose[j])
    return status, pose, rt, branch


def solve(src, dst, tri, edge_sim, min_edge):
    """... for the triplets tri [nh, 3] of the clouds src / dst [m, 3]; two equal indices are DEGENERATE."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    status, pose, rt, branch = solve_points(src[tri], dst[tri], edge_sim, min_edge)
    same = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    status[same] = DEGENERATE
    pose[same] = np.nan
    rt[same] = np.nan
    return status, pose, rt, branch


def pair_sqd(rt, src, dst, max_dist):
    """Step 5 for one float32 matrix rt [3, 4]: the slots [m] -- sqd of an inlier pair, -1 otherwise."""
    s, d = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    M = np.asarray(rt, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = s[:, 0], s[:, 1], s[:, 2]
        w = [M[r, 0] * x + (M[r, 1] * y + (M[r, 2] * z + M[r, 3])) for r in range(3)]      # (world_points' arithmetic)
        dx, dy, dz = w[0] - d[:, 0], w[1] - d[:, 1], w[2] - d[:, 2]
        v = (dx * dx + (dy * dy + dz * dz)).astype(np.float32)
        gate2 = np.float32(max_dist) * np.float32(max_dist)
        inl = v < gate2
    return np.where(inl, v, np.float32(-1.0)).astype(np.float32)


def tree_sum(slots):
    """The float64 sum of the slots that hold a distance (>= 0) in the header's shape: partial t of 256 adds slots t, t + 256, .. in
    ascending order, then partial[t] += partial[t + o] for o = 128 .. 1."""
    v = np.asarray(slots, np.float32)
    vals = np.zeros(-(-max(v.size, 1) // RED) * RED, np.float64)
    vals[:v.size] = np.where(v >= 0, v.astype(np.float64), 0.0)      # (a partial starts at +0.0: adding +0.0 leaves its bits)
    partial = np.zeros(RED, np.float64)
    for row in vals.reshape(-1, RED):
        partial = partial + row
    o = RED // 2
    while o >= 1:
        partial[:o] = partial[:o] + partial[o:2 * o]
        o //= 2
    return float(partial[0])


def reference(src, dst, tri, edge_sim=0.9, min_edge=0.0, max_dist=float("inf")):
    """What ``HipCtx.corr_poses(src, dst, tri, want=("pose", "pair_sqd"), ..)`` must return, plus rt [nh, 3, 4] and fsum [nh]: math.fsum
    of the inliers' distances."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    status, pose, rt, _ = solve(src, dst, tri, edge_sim, min_edge)
    nh, m = status.size, src.shape[0]
    pairs = np.full((nh, m), -1, np.float32)
    inliers, sums, fsums = np.zeros(nh, np.int32), np.zeros(nh), np.zeros(nh)
    for j in np.nonzero(status == OK)[0]:
        pairs[j] = pair_sqd(rt[j], src, dst, max_dist)
        inl = pairs[j] >= 0
        inliers[j] = int(inl.sum())
        sums[j] = tree_sum(pairs[j])
        fsums[j] = math.fsum(float(v) for v in pairs[j][inl])
    return dict(status=status, inliers=inliers, sum_sqd=sums, pose=pose, pair_sqd=pairs, rt=rt, fsum=fsums)


def check(got, ref, tag=""):
    """status, inliers and the bits of pose, pair_sqd and sum_sqd with no tolerance (whichever of them ``got`` holds); sum_sqd also
    within scan_fitness_common.sum_bound of math.fsum."""
    m = ref["pair_sqd"].shape[1]
    assert got["status"].dtype == np.int32 and got["inliers"].dtype == np.int32 and got["sum_sqd"].dtype == np.float64
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=f"{tag}: status")
    np.testing.assert_array_equal(got["inliers"], ref["inliers"], err_msg=f"{tag}: inliers")
    np.testing.assert_array_equal(got["sum_sqd"].view(np.uint64), ref["sum_sqd"].view(np.uint64), err_msg=f"{tag}: sum_sqd bits")
    for j in range(ref["status"].size):
        assert abs(got["sum_sqd"][j] - ref["fsum"][j]) <= sf.sum_bound(m, ref["fsum"][j]), f"{tag}: sum_sqd of {j} against fsum"
    if "pose" in got:
        assert got["pose"].dtype == np.float64
        np.testing.assert_array_equal(np.isnan(got["pose"]), np.isnan(ref["pose"]), err_msg=f"{tag}: pose NaNs")
        okr = ref["status"] == OK
        np.testing.assert_array_equal(got["pose"][okr].view(np.uint64), ref["pose"][okr].view(np.uint64), err_msg=f"{tag}: pose bits")
    if "pair_sqd" in got:
        assert got["pair_sqd"].dtype == np.float32
        np.testing.assert_array_equal(got["pair_sqd"].view(np.uint32), ref["pair_sqd"].view(np.uint32), err_msg=f"{tag}: pair_sqd bits")


def same_bytes(a, b, tag="", names=None):
    for name in (names or sorted(a)):
        assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), f"{tag}: {name} differs"


def scene(seed, stored, m=512, keep=0.3, noise=0.01):
    """Putative correspondences of the standard scan against a map: src = scan_fitness_common.standard_scan(m); pair i keeps its
    true mate with probability ``keep`` (rs.rand(m) < keep, rs = np.random.RandomState(seed)) -- its dst is the scan point's float32
    world point at the true pose x26_of() plus N(0, noise) per coordinate --, every other pair's dst is a random point of ``stored``
    [.., 3].  Returns (src, dst, true [m] bool)."""
    rs = np.random.RandomState(seed)
    src = sf.standard_scan(m)
    true = rs.rand(m) < keep
    world = sf.world_points(sf.x26_of(), src).astype(np.float64) + rs.randn(m, 3) * noise
    stored = np.asarray(stored, np.float32).reshape(-1, 3)
    wrong = stored[rs.randint(0, stored.shape[0], m)]
    dst = np.where(true[:, None], world.astype(np.float32), wrong).astype(np.float32)
    return src, np.ascontiguousarray(dst), true


def pose_error(x26, x26_true):
    """(translation error [m], rotation angle between the two attitudes [deg]) of a state row against another."""
    a, b = np.asarray(x26, np.float64), np.asarray(x26_true, np.float64)
    qa, qb = a[3:7] / np.linalg.norm(a[3:7]), b[3:7] / np.linalg.norm(b[3:7])
    dot = min(1.0, abs(float(qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3])))
    return float(np.linalg.norm(a[0:3] - b[0:3])), math.degrees(2.0 * math.acos(dot))
