"""Shared helper of the FPFH tests: flimo_map_fpfh's definition (include/flimo_c.h) restated in numpy, and the scenes.

The restatement takes the normals and the neighbour lists as inputs -- on the GPU those of normals_range / knn_k of the same context,
on the CPU brute force -- and forms every term in float64 in the written association.  np.sqrt and '/' on float64 are correctly
rounded, as the device's; the one operation numpy cannot pin bit for bit is atan2.  So every pair carries an `ambiguous` flag:
11 * ((f1 + pi) / (2 pi)) lies within EDGE = 1e-9 of an integer (an atan2 that differs in its last bits may land in the other bin),
or w.m == 0 with u.m < 0 (the sign of a zero decides between bin 0 and bin 10).  A point is `tainted` if a pair of its own SPFH, or
of the SPFH of any point in its list, is ambiguous; the GPU tests hold every other point to the restatement bit for bit."""
import functools
import itertools

import numpy as np

from knn_k_common import brute_knn
from normals_common import orient

F = np.float32
INF = float("inf")
SLOTS = 64
BINS = 11
DIM = 3 * BINS
EDGE = 1.0e-9
MAX_TAINTED = 0.005
BLOCK = 16384


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(seed=7, lattice=False):
    """Two jittered planes meeting at an edge and a jittered cylinder standing on one of them, spacing 0.1 m, 5 060 points.  The
    jitter (sigma 1 cm, every coordinate) leaves no three points exactly collinear with a normal.  lattice: the coordinates
    rounded to multiples of 2^-10 m (all inside +-32 m)."""
    rs = np.random.RandomState(seed)
    g = np.arange(40) * 0.1
    a, b = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([a.ravel(), b.ravel(), np.zeros(a.size)], 1)                      # z = 0
    wall = np.stack([np.zeros(a.size), b.ravel(), a.ravel() + 0.1], 1)                 # x = 0, above the edge
    th = np.arange(62) * (2.0 * np.pi / 62)
    h = 0.1 + np.arange(30) * 0.1
    t, z = np.meshgrid(th, h, indexing="ij")
    cyl = np.stack([2.5 + np.cos(t.ravel()), 2.0 + np.sin(t.ravel()), z.ravel()], 1)   # radius 1 m
    pts = np.concatenate([floor, wall, cyl])
    pts = pts + rs.normal(0.0, 0.01, pts.shape)
    pts = pts[rs.permutation(len(pts))]
    if lattice:
        pts = np.round(pts * 1024.0) / 1024.0
    pts = pts.astype(F)
    assert pts.shape == (5060, 3) and len(np.unique(pts, axis=0)) == len(pts)
    pts.setflags(write=False)
    return pts


SHIFT = F([64.0, -64.0, 32.0])


def shifted(pts):
    """The lattice cloud moved by SHIFT: every sum is exact in float32."""
    out = (np.asarray(pts, F) + SHIFT).astype(F)
    assert np.array_equal(out.astype(np.float64), np.asarray(pts, np.float64) + SHIFT.astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def two_clusters(seed=3):
    """Two clusters of 40 points 300 m apart: with k = 64 and no gate every list crosses over."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(0.0, 1.0, (40, 3))
    b = rs.uniform(0.0, 1.0, (40, 3)) + [300.0, 0.0, 0.0]
    pts = np.concatenate([a, b]).astype(F)
    pts.setflags(write=False)
    return pts


def sparse_scene():
    """The scene plus one point 0.2 m beyond the floor's far corner: under a normal gate of 0.15 m it has no plane (nothing but itself
    inside the gate), every point of the scene keeps one, and the corner's points still list it among their 10 nearest."""
    pts = np.concatenate([scene(), F([[4.04, 4.04, 0.0]])]).astype(F)
    pts.setflags(write=False)
    return pts


def duplicate_scene():
    """The scene plus one point, away from everything, stored four times."""
    pts = np.concatenate([scene(), np.tile(F([[7.0, 7.0, 2.0]]), (4, 1))]).astype(F)
    pts.setflags(write=False)
    return pts


VIEWPOINT = (2.0, 2.0, 10.0)

# the clouds and configurations the GPU tests compare with the restatement: name -> (cloud, cfg of HipCtx.map_fpfh)
CASES = {
    "scene-k10": (scene, dict(k=10, normal_k=10)),
    "scene-k33": (scene, dict(k=33, normal_k=10)),
    "lattice-k10": (lambda: scene(lattice=True), dict(k=10, normal_k=10)),
    "lattice-shifted-k10": (lambda: shifted(scene(lattice=True)), dict(k=10, normal_k=10)),
    "clusters-k64": (two_clusters, dict(k=64, normal_k=10)),
    "clusters-k64-gate": (two_clusters, dict(k=64, normal_k=10, max_dist=5.0)),
    "sparse-normal": (sparse_scene, dict(k=10, normal_k=10, normal_max_dist=0.15)),
    "duplicates": (duplicate_scene, dict(k=3, normal_k=10)),
    "viewpoint": (scene, dict(k=10, normal_k=10, viewpoint=VIEWPOINT)),
}


# ---- brute force on the CPU (the GPU tests take these from the context instead) -------------------------------------------------------
def cpu_lists(pts, k, max_dist=INF):
    """(idx [N, k] -1 padded, sqd [N, k] float32, cnt [N]) of flimo_knn_k(p_j, k, max_dist) for every stored point."""
    return brute_knn(pts, pts, k, max_dist, chunk=256)


def cpu_normals(pts, k, max_dist=INF, min_pts=3, viewpoint=None):
    """float32 normals [N, 3] after flimo_map_normals_range's rule (numpy's eigenvectors, not the device's bits): NaN below
    max(3, min_pts) neighbours."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    idx, _, cnt = brute_knn(pts, pts, k, max_dist, chunk=256)
    out = np.full((len(pts), 3), np.nan)
    ok = cnt >= max(3, int(min_pts))
    for c in np.unique(cnt[ok]):
        rows = np.nonzero(ok & (cnt == c))[0]
        r = pts[idx[rows, :c]].astype(np.float64) - pts[rows].astype(np.float64)[:, None, :]
        d = r - r.mean(1, keepdims=True)
        cov = np.einsum("nka,nkb->nab", d, d) / c
        _, v = np.linalg.eigh(cov)
        out[rows] = orient(v[:, :, 0], pts[rows], viewpoint)
    return out.astype(F)


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _bin(x):
    with np.errstate(invalid="ignore"):
        return np.clip(np.floor(x), 0.0, BINS - 1.0).astype(np.int64)


def pair_features(ps, pt, ns, nt):
    """The pair features of source (ps, ns) and target (pt, nt), float32 [.., 3] each: dict of ok (a pair at all, given a non-zero
    distance), f1, f2, f3, h1, h2, h3, ambiguous."""
    ps, pt, ns, nt = (np.asarray(a, F).astype(np.float64) for a in (ps, pt, ns, nt))
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = ~(np.isnan(ns).any(-1) | np.isnan(nt).any(-1))
        d = pt - ps
        f4 = np.sqrt(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))
        a1 = _dot(ns, d) / f4
        a2 = _dot(nt, d) / f4
        swap = np.abs(a1) < np.abs(a2)
        u = np.where(swap[..., None], nt, ns)
        m = np.where(swap[..., None], ns, nt)
        d = np.where(swap[..., None], -d, d)
        f3 = np.where(swap, -a2, a1)
        v = _cross(d, u)
        vn = np.sqrt(v[..., 0] * v[..., 0] + (v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]))
        ok = ok & (vn != 0.0) & ~np.isnan(vn)
        v = v / vn[..., None]
        w = _cross(u, v)
        f2 = _dot(v, m)
        wm, um = _dot(w, m), _dot(u, m)
        f1 = np.arctan2(wm, um)
        x1 = 11.0 * ((f1 + np.pi) * (1.0 / (2.0 * np.pi)))
        h1, h2, h3 = _bin(x1), _bin(11.0 * ((f2 + 1.0) * 0.5)), _bin(11.0 * ((f3 + 1.0) * 0.5))
        x1e = 11.0 * ((f1 + np.pi) / (2.0 * np.pi))
        amb = ok & ((np.abs(x1e - np.round(x1e)) < EDGE) | ((wm == 0.0) & (um < 0.0)))
    return dict(ok=ok, f1=f1, f2=f2, f3=f3, h1=h1, h2=h2, h3=h3, ambiguous=amb)


def slot_tree(v):
    """The pairwise tree over the 64 slots (axis 1): ((v0 + v1) + (v2 + v3)) + ..."""
    v = np.asarray(v, np.float64)
    assert v.shape[1] == SLOTS
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def restate(pts, normals, idx, sqd, cnt, first=0, n=None, spfh_rows=None):
    """flimo_map_fpfh over the stored points `pts` [N, 3], from their float32 normals [N, 3+] and their lists (idx [N, k] -1 padded,
    sqd [N, k] float32, cnt [N]): dict of fpfh [n, 33] float32, spfh [N, 33] uint8 (the WHOLE map's), cnt [n], pair_h1 / pair_ok /
    pair_amb [N, k] (the theta bin of every slot's pair, whether it is one, whether it is ambiguous), tainted [N].
    spfh_rows: form the sums from these rows instead of the restated ones."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    nrm = np.asarray(normals, F)[:, :3]
    idx, sqd, cnt = np.asarray(idx), np.asarray(sqd, F), np.asarray(cnt)
    N, k = idx.shape
    n = N - first if n is None else n
    has = idx >= 0
    assert np.array_equal(has.sum(1), cnt)
    j = np.where(has, idx, 0)
    slot = has & (sqd != 0)
    ok, amb, h1 = np.zeros((N, k), bool), np.zeros((N, k), bool), np.zeros((N, k), np.int8)
    spfh = np.zeros((N, DIM), np.int64)
    for a in range(0, N, BLOCK):                                      # (blocks of points: the pairs of a million points do not fit at once)
        s = slice(a, min(a + BLOCK, N))
        pf = pair_features(pts[s, None, :], pts[j[s]], nrm[s, None, :], nrm[j[s]])
        ok[s] = slot[s] & pf["ok"]
        amb[s] = ok[s] & pf["ambiguous"]
        h1[s] = pf["h1"]
        rows = np.broadcast_to(np.arange(s.start, s.stop)[:, None], ok[s].shape)
        for g, key in enumerate(("h1", "h2", "h3")):
            np.add.at(spfh, (rows[ok[s]], g * BINS + pf[key][ok[s]]), 1)
    assert spfh.max(initial=0) <= 255
    own = amb.any(1)
    tainted = own | (own[j] & has).any(1)
    use = spfh if spfh_rows is None else np.asarray(spfh_rows, np.int64)
    with np.errstate(divide="ignore"):
        inc = np.where(cnt >= 2, 100.0 / np.maximum(cnt - 1, 1).astype(np.float64), 0.0)
        w = np.where(slot, 1.0 / np.where(slot, sqd, F(1)).astype(np.float64), 0.0)
    Fb = np.zeros((n, DIM))
    for a in range(0, n, BLOCK):
        r = slice(first + a, first + min(a + BLOCK, n))
        t = np.zeros((r.stop - r.start, SLOTS))
        for b in range(DIM):
            t[:, :k] = np.where(has[r], w[r] * (use[j[r], b].astype(np.float64) * inc[j[r]]), 0.0)
            Fb[a:a + BLOCK, b] = slot_tree(t)
    r = slice(first, first + n)
    out = np.zeros((n, DIM), F)
    for g in range(3):
        S = Fb[:, g * BINS].copy()
        for b in range(1, BINS):
            S = S + Fb[:, g * BINS + b]
        with np.errstate(divide="ignore", invalid="ignore"):
            scaled = (Fb[:, g * BINS:(g + 1) * BINS] * (100.0 / S)[:, None]).astype(F)
        out[:, g * BINS:(g + 1) * BINS] = np.where((S != 0.0)[:, None], scaled, F(0))
    return dict(fpfh=out, spfh=spfh.astype(np.uint8), cnt=cnt[r].astype(np.int32), pair_h1=h1.astype(np.int64), pair_ok=ok, pair_amb=amb, tainted=tainted,
                group_sum=np.stack([Fb[:, g * BINS:(g + 1) * BINS].sum(1) for g in range(3)], 1))


def moved_by_ambiguous_pairs(got_row, want_row, amb_bins):
    """Whether got differs from want by at most one count moved from the restated theta bin of each ambiguous pair to a neighbouring
    one (0 and 10 are neighbours), everything else equal."""
    got, want = np.asarray(got_row, np.int64), np.asarray(want_row, np.int64)
    if not np.array_equal(got[BINS:], want[BINS:]):
        return False
    for moves in itertools.product((0, -1, 1), repeat=len(amb_bins)):
        t = want[:BINS].copy()
        for h, mv in zip(amb_bins, moves):
            if mv:
                t[h] -= 1
                t[(h + mv) % BINS] += 1
        if np.array_equal(t, got[:BINS]):
            return True
    return False


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
