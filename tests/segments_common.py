"""Map segments restated in numpy (plain, deterministic, no GPU), shared by test_segments_host.py and test_gpu_segments.py.

The contract (include/flimo_c.h, "Map segments"; fast_limo_amd/csrc/hip/flimo_segment.h):
  * segment of stored point i = the largest s with begin[s] <= i;
  * the move: with X = float64(x) and so on, r_k = T[4k] X + (T[4k+1] Y + (T[4k+2] Z + T[4k+3])), one rounding per written
    operation, nothing contracted; the moved component is float32(r_k).
numpy's elementwise float64 multiply and add round once each and never fuse, so the two functions below ARE that definition and
every comparison with the library is bit for bit."""
import math

import numpy as np

from fast_limo_amd import synth

F = np.float32


def seg_find(begin, i):
    """begin: the starts begin[0 .. S - 1] (ascending from 0); i: insertion indices.  The largest s with begin[s] <= i."""
    return np.searchsorted(np.asarray(begin, np.uint64), np.asarray(i, np.uint64), side="right").astype(np.int64) - 1


def seg_move(T, p):
    """T: [n, 12] (or one [12]) float64, row-major 3 x 4; p: [n, 3] float32.  The moved points, float32 [n, 3]."""
    T = np.asarray(T, np.float64).reshape(-1, 12)
    p = np.asarray(p, F).reshape(-1, 3)
    X, Y, Z = (p[:, a].astype(np.float64) for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        r = [T[:, 4 * k] * X + (T[:, 4 * k + 1] * Y + (T[:, 4 * k + 2] * Z + T[:, 4 * k + 3])) for k in range(3)]
        return np.stack(r, axis=1).astype(F)


def corrected(begin, T, pts, first=0):
    """What flimo_map_corrected reports for the stored points pts = map[first : first + len(pts)]: (moved points, changed).
    begin: the table begin[0 .. S] as flimo_map_segments reports it (the last entry, the size, is not read)."""
    begin = np.asarray(begin, np.uint64)
    pts = np.asarray(pts, F).reshape(-1, 3)
    s = seg_find(begin[:-1], first + np.arange(len(pts)))
    out = seg_move(np.asarray(T, np.float64).reshape(-1, 12)[s], pts)
    changed = int(np.any(out.view(np.uint32) != pts.view(np.uint32), axis=1).sum())
    return out, changed


def range_removed_table(begin, first, n):
    """begin'[s] = begin[s] - |[first, first + n) with [0, begin[s])| for the whole table begin[0 .. S] (the range cut to the size)."""
    b = np.asarray(begin, np.int64)
    n = max(0, min(int(n), int(b[-1]) - int(first)))
    return (b - np.clip(b - int(first), 0, n)).astype(np.uint64)


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def rigid(rpy_deg, t):
    """A rigid 3 x 4 matrix as 12 float64: Rz Ry Rx of the angles (degrees), then t."""
    R = synth.rpy_to_R(*[math.radians(a) for a in rpy_deg])
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12)


def mat4(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def quat_of(R):
    """Unit quaternion x y z w of a rotation matrix (Shepperd's branches), w >= 0."""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def x26_of(M):
    """A state row with pos and rot of the 4 x 4 pose M, the rest zero."""
    x = np.zeros(26)
    x[0:3], x[3:7] = M[:3, 3], quat_of(M[:3, :3])
    return x


def mat_of_x26(x):
    """The 4 x 4 pose of a state row, from the normalised quaternion -- written out on its own (Rodrigues through the angle and
    the axis), not the library's polynomial in the quaternion's entries."""
    q = np.asarray(x[3:7], np.float64)
    q = q / np.linalg.norm(q)
    v, w = q[:3], q[3]
    nv = np.linalg.norm(v)
    if nv < 1e-300:
        return mat4(np.eye(3), x[0:3])
    th, ax = 2.0 * math.atan2(nv, w), v / nv
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return mat4(np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K), x[0:3])


# ---- the ring: keyframes on a circle, odometry that drifts, one loop edge ------------------------------------------------------
def ring_truth(n=24, radius=10.0):
    """n poses on a circle of `radius` metres in the plane z = 0, heading along the tangent: [n, 4, 4]."""
    out = []
    for k in range(n):
        a = 2.0 * math.pi * k / n
        out.append(mat4(synth.rpy_to_R(0.0, 0.0, a + 0.5 * math.pi), [radius * math.cos(a), radius * math.sin(a), 0.0]))
    return np.array(out)


def ring_case(n=24, radius=10.0, err_t=0.02, err_deg=0.1):
    """The ring with every relative pose corrupted by the same body-frame error (err_t metres along x, err_deg degrees of yaw).
    Returns (truth [n, 4, 4], drifted [n, 4, 4], edges): the n - 1 odometry edges carry the corrupted measurements, which the drifted
    poses satisfy exactly; the loop edge last -> first is exact."""
    truth = ring_truth(n, radius)
    E = mat4(synth.rpy_to_R(0.0, 0.0, math.radians(err_deg)), [err_t, 0.0, 0.0])
    drift, edges = [truth[0]], []
    for k in range(n - 1):
        Z = np.linalg.inv(truth[k]) @ truth[k + 1] @ E
        drift.append(drift[k] @ Z)
        edges.append((k, k + 1, Z))
    edges.append((n - 1, 0, np.linalg.inv(truth[n - 1]) @ truth[0]))
    return truth, np.array(drift), edges


def ring_sweep(k, pose, n_pts=1500, L=25.0):
    """Sweep k of the box world (its own sample of the surfaces) as seen from `pose` (4 x 4): body-frame points, float64 [n, 3]."""
    pw = synth.box_world_map(n_pts, L, 100 + k).astype(np.float64)
    return (pw - pose[:3, 3]) @ pose[:3, :3]


def place(pose, pb):
    """Body-frame points at a 4 x 4 pose, float64."""
    return pb @ pose[:3, :3].T + pose[:3, 3]
