"""Shared helpers of the tests of flimo_scan_linearize (point-to-plane normal equations of the resident scan per pose hypothesis):
the yardstick, the sum bound, the starts of the convergence tests and the pose error.

The yardstick of a pose is what the call replaces, restated.  The planes of the pose's world points come from the route that
exists without the call -- on the GPU the public ``ctx.scan_to_world`` + ``ctx.normals(w, k, gate, min_pts)`` (``composed``), without
one ``normals_common.reference`` over the map (``planes_ref``: brute-force neighbourhoods, math.fsum moments, numpy eigh) -- and the
terms of flimo_c.h are formed from them in numpy float64, in the stated association (``terms``; numpy's elementwise products and
sums are not contracted), and summed with math.fsum (``sums``).

The sum bound.  A sum S of n float64 terms taken in any order differs from the exact sum by at most (n - 1) * 2^-53 * sum|term| to
first order: each of the n - 1 additions rounds a partial sum whose magnitude is at most sum|term|.  n * 2^-52 * sum|term| covers
it twice over, and fsum's own rounding (derived as scan_fitness_common.sum_bound, with absolute values because the terms carry
signs).  The products J_a * J_b themselves are single float64 roundings of the same operands on both sides: no tolerance there."""
import math
from multiprocessing.pool import ThreadPool

import numpy as np

import normals_common as nc
import scan_fitness_common as sf
import sums_common
from fast_limo_amd import synth

INF = float("inf")
PAIRS21 = [(a, b) for a in range(6) for b in range(a, 6)]      # H's packing: 00, 01 .. 05, 11 .. 55
# (dx, dy, yaw deg) of the nine starts of the convergence test; the host test runs HOST_STARTS
STARTS = ((0, 0, 0), (0.5, 0, 0), (-0.5, 0.5, 5), (0.5, -0.5, -5), (1, 0, 0), (1, 1, 10), (-1, 1, -10), (0, 0, 10), (0.5, 0.5, 10))
HOST_STARTS = ((0.5, 0, 0), (-0.5, 0.5, 5), (1, 1, 10), (-1, 1, -10))
POS_BAR, ROT_BAR_DEG = 0.01, 0.1


def start_poses(starts):
    return np.stack([sf.displaced(dx=dx, dy=dy, dyaw_deg=yaw) for dx, dy, yaw in starts])


def quat_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_error(x26):
    """(position error [m], rotation error [deg]) of a state vector against the scene's true pose synth.T_STAR_*."""
    R_true = synth.rpy_to_R(*[math.radians(a) for a in synth.T_STAR_RPY_DEG])
    dR = R_true.T @ quat_R(x26[3:7])
    ang = math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(dR) - 1.0)))))
    return float(np.linalg.norm(np.asarray(x26[0:3]) - np.asarray(synth.T_STAR_T))), ang


def terms(x26, scan, w, cnt, centroid, evals, normal, min_pts, max_curv):
    """The rows [n, 7] (J0..J5, d; NaN for an invalid pair) and the validity [n] of one pose, from its planes: w [n, 3] float32,
    cnt [n], centroid / evals / normal [n, 3] float64 (NaN where there are too few neighbours)."""
    n = w.shape[0]
    R = sf.pose_rt(x26)[:, :3].astype(np.float64)
    p = np.asarray(scan, np.float32).astype(np.float64)
    wd = np.asarray(w, np.float32).astype(np.float64)
    c, l, nr = np.asarray(centroid, np.float64), np.asarray(evals, np.float64), np.asarray(normal, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tr = l[:, 0] + l[:, 1] + l[:, 2]
        curv = np.where(tr == 0.0, 0.0, l[:, 0] / np.where(tr == 0.0, 1.0, tr))
        valid = (np.asarray(cnt) >= max(3, int(min_pts))) & (curv <= np.float64(np.float32(max_curv)))
        d = nr[:, 0] * (wd[:, 0] - c[:, 0]) + (nr[:, 1] * (wd[:, 1] - c[:, 1]) + nr[:, 2] * (wd[:, 2] - c[:, 2]))
        a = [R[0, t] * nr[:, 0] + (R[1, t] * nr[:, 1] + R[2, t] * nr[:, 2]) for t in range(3)]
        b = [p[:, 1] * a[2] - p[:, 2] * a[1], p[:, 2] * a[0] - p[:, 0] * a[2], p[:, 0] * a[1] - p[:, 1] * a[0]]
    rows = np.stack(a + b + [d], axis=1)
    rows[~valid] = np.nan
    assert rows.shape == (n, 7)
    return rows, valid


def sums(rows):
    """math.fsum of a pose's 28 sums over its valid rows, and the sums of the terms' absolute values (for the bound):
    (valid count, H [21], g [6], cost, absH [21], absg [6])."""
    r = rows[~np.isnan(rows[:, 6])]
    H = np.array([math.fsum(r[:, a] * r[:, b]) for a, b in PAIRS21])
    aH = np.array([math.fsum(np.abs(r[:, a] * r[:, b])) for a, b in PAIRS21])
    g = np.array([math.fsum(r[:, a] * r[:, 6]) for a in range(6)])
    ag = np.array([math.fsum(np.abs(r[:, a] * r[:, 6])) for a in range(6)])
    return r.shape[0], H, g, math.fsum(r[:, 6] * r[:, 6]), aH, ag


def sum_bound(n, abs_sum):
    return n * 2.0 ** -52 * abs_sum


def as_call(per_pose, n):
    """The dict of HipCtx.scan_linearize(want_rows=True) from a list of (rows, pair_cnt) per pose, the sums being fsum's."""
    m = len(per_pose)
    out = dict(valid=np.zeros(m, np.int32), H=np.zeros((m, 21)), g=np.zeros((m, 6)), cost=np.zeros(m), rows=np.full((m, n, 7), np.nan),
               pair_cnt=np.zeros((m, n), np.int32), absH=np.zeros((m, 21)), absg=np.zeros((m, 6)))
    for j, (rows, cnt) in enumerate(per_pose):
        out["valid"][j], out["H"][j], out["g"][j], out["cost"][j], out["absH"][j], out["absg"][j] = sums(rows)
        out["rows"][j], out["pair_cnt"][j] = rows, cnt
    return out


def composed(ctx, poses, k, gate, min_pts=3, max_curv=INF):
    """The yardstick on the GPU, by the public calls that exist without flimo_scan_linearize."""
    scan = ctx.scan_get()
    per = []
    for x in np.asarray(poses, np.float64).reshape(-1, 26):
        w = ctx.scan_to_world(x)
        nm = ctx.normals(w, k, gate, min_pts, None, want=("centroid", "eig"))
        rows, _ = terms(x, scan, w, nm["cnt"], nm["centroid"], nm["eig"][:, :3], nm["eig"][:, 3:], min_pts, max_curv)
        per.append((rows, nm["cnt"]))
    return as_call(per, scan.shape[0])


def planes_ref(w, mp, k, gate, min_pts=3, cell=2.5):
    """normals_common.reference(w, mp, k, gate, min_pts) -- cnt, centroid, evals, normal -- without its |w| x |map| cost when there is
    a gate: the queries are grouped by the cube of edge `cell` they lie in and the reference runs per group over the stored points
    inside that cube grown by the gate (widened by 1e-3 of it and 1 mm: a point whose float32 squared distance passes the gate lies
    inside), kept in ascending index, so every tie falls as over the whole map."""
    m = w.shape[0]
    out = dict(cnt=np.zeros(m, np.int32), centroid=np.full((m, 3), np.nan), evals=np.full((m, 3), np.nan), normal=np.full((m, 3), np.nan))

    def put(rows, ref):
        for name in out:
            out[name][rows] = ref[name]
    ok = np.isfinite(w.astype(np.float64)).all(1)
    if np.isinf(gate) or mp.shape[0] == 0:
        put(np.arange(m), nc.reference(w, mp, k, gate, min_pts))
        return out
    grow = gate * (1.0 + 1e-3) + 1e-3
    w64, mp64 = w.astype(np.float64), mp.astype(np.float64)
    rows_ok = np.nonzero(ok)[0]
    cells = np.floor(w64[ok] / cell).astype(np.int64)
    uniq, inv = np.unique(cells, axis=0, return_inverse=True)
    inv = inv.reshape(-1)

    def group(gi):
        rows = rows_ok[inv == gi]
        lo, hi = uniq[gi] * cell - grow, (uniq[gi] + 1) * cell + grow
        cand = np.nonzero(((mp64 >= lo) & (mp64 <= hi)).all(1))[0]
        if cand.size:
            put(rows, nc.reference(w[rows], mp[cand], k, gate, min_pts))
    with ThreadPool(8) as pool:
        pool.map(group, range(len(uniq)))
    return out


def linearize_ref(poses, scan, mp, k, gate, min_pts=3, max_curv=INF):
    """The yardstick without a GPU: the dict of the call for `poses` over the stored points `mp`."""
    per = []
    for x in np.asarray(poses, np.float64).reshape(-1, 26):
        w = sf.world_points(x, scan)
        pl = planes_ref(w, mp, k, gate, min_pts)
        rows, _ = terms(x, scan, w, pl["cnt"], pl["centroid"], pl["evals"], pl["normal"], min_pts, max_curv)
        per.append((rows, pl["cnt"]))
    return as_call(per, np.asarray(scan).shape[0])


def check(got, ref, n, tag="", want_rows=True):
    """valid, pair_cnt and every bit of rows (the NaN pattern included) with no tolerance; H, g, cost within sum_bound of fsum."""
    np.testing.assert_array_equal(got["valid"], ref["valid"], err_msg=f"{tag}: valid")
    assert got["valid"].dtype == np.int32 and got["H"].dtype == np.float64 and got["H"].shape == ref["H"].shape
    if want_rows:
        np.testing.assert_array_equal(got["pair_cnt"], ref["pair_cnt"], err_msg=f"{tag}: pair_cnt")
        assert got["rows"].dtype == np.float64 and got["rows"].shape == ref["rows"].shape
        # every NaN of either side is the one quiet NaN: the bits compare
        np.testing.assert_array_equal(np.isnan(got["rows"]), np.isnan(ref["rows"]), err_msg=f"{tag}: NaN pattern of rows")
        fin = ~np.isnan(ref["rows"])
        np.testing.assert_array_equal(got["rows"][fin].view(np.uint64), ref["rows"][fin].view(np.uint64), err_msg=f"{tag}: bits of rows")
    worst = 0.0
    for j in range(ref["valid"].shape[0]):
        for name, e, b in (("H", np.abs(got["H"][j] - ref["H"][j]), sum_bound(n, ref["absH"][j])),
                           ("g", np.abs(got["g"][j] - ref["g"][j]), sum_bound(n, ref["absg"][j])),
                           ("cost", np.abs(got["cost"][j] - ref["cost"][j]), sum_bound(n, ref["cost"][j]))):
            assert np.all(e <= b), f"{tag}: {name} of pose {j}: off by {np.max(e)!r}, bound {np.max(b)!r}"
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(np.asarray(b) > 0, e / b, 0.0))))
    return worst


def pinned(got, tag=""):
    """H, g and cost of every pose are, byte for byte, sums_common.shape_sums of the 28 products formed in numpy float64 from the
    returned rows (21 of H: J[a] * J[b], a <= b, row-major; 6 of g: J[a] * J[6]; the cost: J[6] * J[6]; a NaN row adds +0.0), and
    valid is the number of rows that are not NaN."""
    for j, rows in enumerate(got["rows"]):
        dead = np.isnan(rows[:, 6])
        np.testing.assert_array_equal(np.isnan(rows), np.broadcast_to(dead[:, None], rows.shape), err_msg=f"{tag}: a row is NaN as a whole")
        with np.errstate(invalid="ignore"):
            T = np.stack([rows[:, a] * rows[:, b] for a, b in PAIRS21] + [rows[:, a] * rows[:, 6] for a in range(6)] + [rows[:, 6] * rows[:, 6]], axis=1)
        T[dead] = 0.0
        want = sums_common.shape_sums(T[:, None, :])
        mine = np.concatenate([got["H"][j], got["g"][j], got["cost"][j:j + 1]])
        assert mine.tobytes() == want.tobytes(), f"{tag}: the sums of pose {j} are not the shape's: {np.nonzero(mine != want)[0]}"
        assert got["valid"][j] == int((~dead).sum()), f"{tag}: valid of pose {j}"


def same_bytes(a, b, tag="", names=("valid", "H", "g", "cost", "rows", "pair_cnt")):
    for name in names:
        if name in a or name in b:
            x, y = a[name], b[name]
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{tag}: {name} differs"
