"""Shared helpers of the GICP tests (flimo_gicp_build / flimo_scan_gicp): the two functions of fast_limo_amd/csrc/hip/flimo_gicp.h
restated in numpy -- float64, vectorised over the pairs, every product and sum in the association include/flimo_c.h writes out --,
the pass (the nearest stored point by scan_fitness_common.nearest: float32 distances in the order (bits, insertion index), the gate),
and the 28 sums in the shape of sums_common, a slot being a scan point with one term.

A covariance is its six numbers xx xy xz yy yz zz (normals_common.PAIRS); v[k] is the unit vector of eigenvalue l[k], ascending."""
import math

import numpy as np

import scan_fitness_common as sf
import sums_common
from normals_common import PAIRS
from scan_linearize_common import PAIRS21
from sums_common import RED, SEG

D = np.float64
PLANE, CLAMP = 0, 1      # FLIMO_GICP_PLANE, FLIMO_GICP_CLAMP


def sym3(c6):
    c6 = np.asarray(c6, D)
    return np.stack([np.stack([c6[..., 0], c6[..., 1], c6[..., 2]], -1), np.stack([c6[..., 1], c6[..., 3], c6[..., 4]], -1),
                     np.stack([c6[..., 2], c6[..., 4], c6[..., 5]], -1)], -2)


def regularize(l, v, rule, eps):
    """gicp_regularize given the eigen-pairs: l [.., 3] ascending, v [.., 3, 3] (row k the vector of l[k]) -> C' [.., 6]; six NaN
    where a pair is not finite or l2 is not > 0.0."""
    l, v = np.asarray(l, D), np.asarray(v, D)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.all(np.isfinite(l), -1) & np.all(np.isfinite(v), (-2, -1)) & (l[..., 2] > 0.0)
        if rule == PLANE:
            lp = np.stack([np.full(l.shape[:-1], D(eps)), np.ones(l.shape[:-1]), np.ones(l.shape[:-1])], -1)
        else:
            floor = D(eps) * l[..., 2]
            lp = np.where(l < floor[..., None], floor[..., None], l)
        out = np.empty(l.shape[:-1] + (6,))
        for t, (a, b) in enumerate(PAIRS):
            s = np.zeros(l.shape[:-1])
            for k in range(3):
                s = s + (lp[..., k] * v[..., k, a]) * v[..., k, b]
            out[..., t] = s
    out[~ok] = np.nan
    return out


def eigh_pairs(cov6):
    """numpy's eigen-pairs of covariances [.., 6]: (l [.., 3] ascending, v [.., 3, 3] rows); NaN for a non-finite covariance."""
    c = np.asarray(cov6, D)
    ok = np.all(np.isfinite(c), -1)
    w, V = np.linalg.eigh(sym3(np.where(ok[..., None], c, 0.0)))
    l, v = np.where(ok[..., None], w, np.nan), np.where(ok[..., None, None], np.swapaxes(V, -1, -2), np.nan)
    return l, v


def regularize_numpy(cov6, rule, eps):
    """gicp_regularize with numpy.linalg.eigh in the place of the Jacobi."""
    return regularize(*eigh_pairs(cov6), rule, eps)


def knn_covs(q, pts, k, chunk=512):
    """The covariance [nq, 6] of the k nearest of pts around every q (float64, about the neighbours' mean): the numpy stand-in for
    flimo_map_normals' cov where only its use matters, not its bits."""
    q, pts = np.asarray(q, np.float32).astype(D), np.asarray(pts, np.float32).astype(D)
    out = np.empty((q.shape[0], 6))
    p2 = (pts * pts).sum(1)
    for a in range(0, q.shape[0], chunk):
        qq = q[a:a + chunk]
        d2 = (qq * qq).sum(1)[:, None] - 2.0 * (qq @ pts.T) + p2[None, :]
        nb = pts[np.argpartition(d2, k - 1, axis=1)[:, :k]]
        dv = nb - nb.mean(1, keepdims=True)
        for t, (i, j) in enumerate(PAIRS):
            out[a:a + chunk, t] = (dv[:, :, i] * dv[:, :, j]).mean(1)
    return out


def dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def term(w, b, p, R, CA, CB, wide_w=False):
    """gicp_term over n pairs: w, b, p [n, 3] float32; R [3, 3] float32; CA, CB [n, 6] float64.  Returns dict(live [n], m [n],
    det [n], C [n, 28]: H's 21, g's 6, the cost; everything 0 where the term is not live).  wide_w: w is taken as float64 as it
    is (the derivative's test, which moves w in float64)."""
    b, p = (np.asarray(a, np.float32).astype(D) for a in (b, p))
    w = np.asarray(w, D) if wide_w else np.asarray(w, np.float32).astype(D)
    R = np.asarray(R, np.float32).astype(D).reshape(3, 3)
    CA, CB = np.asarray(CA, D).reshape(-1, 6), np.asarray(CB, D).reshape(-1, 6)
    n = w.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        r = [w[:, i] - b[:, i] for i in range(3)]
        A = [[CA[:, 0], CA[:, 1], CA[:, 2]], [CA[:, 1], CA[:, 3], CA[:, 4]], [CA[:, 2], CA[:, 4], CA[:, 5]]]
        T = [[R[i, 0] * A[0][j] + (R[i, 1] * A[1][j] + R[i, 2] * A[2][j]) for j in range(3)] for i in range(3)]
        S = {(i, j): CB[:, t] + dot3(T[i], R[j]) for t, (i, j) in enumerate(PAIRS)}
        S00, S01, S02, S11, S12, S22 = (S[ij] for ij in PAIRS)
        c00, c01, c02 = S11 * S22 - S12 * S12, S02 * S12 - S01 * S22, S01 * S12 - S02 * S11
        c11, c12, c22 = S00 * S22 - S02 * S02, S01 * S02 - S00 * S12, S00 * S11 - S01 * S01
        det = S00 * c00 + (S01 * c01 + S02 * c02)
        live = np.all(np.isfinite(CA), 1) & np.all(np.isfinite(CB), 1) & (det > 0.0) & np.isfinite(1.0 / det)
        M = [[c00 / det, c01 / det, c02 / det], [c01 / det, c11 / det, c12 / det], [c02 / det, c12 / det, c22 / det]]
        y = [dot3(M[i], r) for i in range(3)]
        m = dot3(r, y)
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        J = [[np.full(n, R[i, c]) for i in range(3)] for c in range(3)]
        J.append([py * R[i, 2] - pz * R[i, 1] for i in range(3)])
        J.append([pz * R[i, 0] - px * R[i, 2] for i in range(3)])
        J.append([px * R[i, 1] - py * R[i, 0] for i in range(3)])
        U = [[dot3(M[a], J[c]) for a in range(3)] for c in range(6)]
        C = np.zeros((n, 28))
        for t, (a, c) in enumerate(PAIRS21):
            C[:, t] = dot3(J[a], U[c])
        for a in range(6):
            C[:, 21 + a] = dot3(J[a], y)
        C[:, 27] = m
    C[~live] = 0.0
    return dict(live=live, m=np.where(live, m, 0.0), det=np.where(live, det, 0.0), C=C)


def restate(x26, scan, scan_cov, mp, model, max_dist, nn_idx=None):
    """One pose of flimo_scan_gicp: dict(w, idx [n] (the neighbour or -1), valid [n], m [n] (NaN for an invalid pair), C [n, 28]
    (+0.0 rows for invalid pairs)).  nn_idx: the neighbours when the caller has them already."""
    scan = np.asarray(scan, np.float32).reshape(-1, 3)
    mp = np.asarray(mp, np.float32).reshape(-1, 3)
    w = sf.world_points(x26, scan)
    n = scan.shape[0]
    if nn_idx is None:
        nn_idx = sf.nearest(w, mp, max_dist)[1] if (n and mp.shape[0] and max_dist != 0.0) else np.full(n, -1, np.int32)
    has = nn_idx >= 0
    at = np.where(has, nn_idx, 0)
    if mp.shape[0] == 0:
        return dict(w=w, idx=nn_idx, valid=np.zeros(n, bool), m=np.full(n, np.nan), C=np.zeros((n, 28)))
    t = term(w, mp[at], scan, sf.pose_rt(x26)[:, :3], scan_cov, np.asarray(model, D).reshape(-1, 6)[at])
    valid = has & t["live"]
    C = t["C"].copy()
    C[~valid] = 0.0
    return dict(w=w, idx=nn_idx, valid=valid, m=np.where(valid, t["m"], np.nan), C=C)


def shape_sums(C):
    """The 28 sums of one pose in the shape of the call: C [n, 28] -> [28]."""
    C = np.asarray(C, D)
    return sums_common.shape_sums(C.reshape(C.shape[0], 1, 28)) if C.shape[0] else np.zeros(28)


def shape_sums_plain(C):
    """shape_sums in plain Python floats."""
    C = np.asarray(C)
    n = C.shape[0]
    total = [0.0] * 28
    for s0 in range(0, n, SEG):
        acc = [[0.0] * 28 for _ in range(RED)]
        for t in range(RED):
            for i in range(s0 + t, min(n, s0 + SEG), RED):
                row, a = C[i].tolist(), acc[t]
                for q in range(28):
                    a[q] = a[q] + row[q]
        part = []
        for wave in range(4):
            lanes = [acc[64 * wave + l][:] for l in range(64)]
            o = 1
            while o < 64:
                lanes = [[lanes[l][q] + lanes[l ^ o][q] for q in range(28)] for l in range(64)]
                o <<= 1
            part.append(lanes[0])
        for q in range(28):
            total[q] = total[q] + ((part[0][q] + part[1][q]) + (part[2][q] + part[3][q]))
    return np.array(total)


def fsum_sums(C):
    """(sums [28] by math.fsum, sums of absolute values [28], the number of added terms)."""
    flat = np.asarray(C).reshape(-1, 28)
    flat = flat[np.any(flat != 0.0, axis=1)]
    return (np.array([math.fsum(flat[:, q]) for q in range(28)]), np.array([math.fsum(np.abs(flat[:, q])) for q in range(28)]),
            max(flat.shape[0], 1))


def as_call(per_pose):
    """The dict of scan_gicp(want_pairs=True) from the restatement of every pose, the sums in the call's shape."""
    S = [shape_sums(r["C"]) for r in per_pose]
    return dict(valid=np.array([int(r["valid"].sum()) for r in per_pose], np.int32), H=np.array([s[:21] for s in S]).reshape(-1, 21),
                g=np.array([s[21:27] for s in S]).reshape(-1, 6), cost=np.array([s[27] for s in S]).reshape(-1),
                pair_idx=np.array([r["idx"] for r in per_pose], np.int32), pair_m=np.array([r["m"] for r in per_pose]))


def linearizer(scan, scan_cov, mp, model, max_dist, neighbours=None):
    """``linearize`` for api.scan_align: the restatement in the place of the device, all poses of a call in one neighbour search.
    neighbours(xs) -> nn_idx [np, n]: another source of the neighbours (the device's scan_fitness)."""
    scan = np.asarray(scan, np.float32).reshape(-1, 3)

    def linearize(xs):
        xs = np.asarray(xs, D).reshape(-1, 26)
        n = scan.shape[0]
        if neighbours is not None:
            idx = np.asarray(neighbours(xs)).reshape(len(xs), n)
        else:
            idx = sf.nearest(np.concatenate([sf.world_points(x, scan) for x in xs]), np.asarray(mp, np.float32), max_dist)[1].reshape(len(xs), n)
        out = as_call([restate(x, scan, scan_cov, mp, model, max_dist, nn_idx=idx[j]) for j, x in enumerate(xs)])
        return {k: out[k] for k in ("valid", "H", "g", "cost")}
    return linearize
