"""Shared helpers of the region tests (flimo_map_regions / flimo_map_region_list / flimo_map_remove_regions): the definition
restated, and the scenes.

The definition (include/flimo_c.h), restated.  The vertices are the N stored points in insertion order; the normals are an INPUT:
rows nx ny nz curvature, float32 -- on the GPU those of the same context's map_normals_range, on the CPU numpy's (``cpu_normals``).
 1. a point HAS A NORMAL iff its four floats are finite;
 2. it is SMOOTH iff it has a normal and curvature <= max_curv (float32; max_curv may be inf);
 3. {i, j}, i != j, both smooth, is an edge iff sqdist3(p_i, p_j) < tol * tol (flimo_map_clusters' predicate) and
    |n_i.x*n_j.x + (n_i.y*n_j.y + n_i.z*n_j.z)| >= min_cos, all float32 in this association;
 4. a region is a connected component of that graph over the smooth points of the whole map; its label is the smallest insertion
    index among its smooth points;
 5. border != 0: a point b that has a normal and is not smooth joins the region of the smooth j that passes both tests of 3.
    against b, the one of smallest key (bits of the float32 sqdist3(p_b, p_j), j); it carries nothing further, counts towards the
    region's size and leaves the label alone;
 6. a point with no region has label -1 and size 0 and is never selected;
 7. selection and mask as the clusters'; stats: n, smooth, regions, largest, sel_regions, unassigned, sel_points;
 8. the listing: the selected regions in ascending label, members in insertion order, centroid and cov in the voxels' SHAPE
    (voxels_common.sum_shape: runs of 64, the pairwise tree, the runs chained from +0.0), two passes, divided by count;
 9. tol == 0: no edges, no border attachment.
Every integer has one correct value given the normals and numpy's float32 / float64 arithmetic is the device's bit for bit: no
tolerance anywhere.  ``restate`` is a dense predicate in blocks of rows and a plain union-find in Python (clusters_common's);
``labels_bfs`` is a second form of the components."""
import functools

import numpy as np

import clusters_common as cc
import voxels_common as vc

F = np.float32
D = np.float64
INF = float("inf")
COS20, COS12 = 0.93969262, 0.9781476
DEFAULTS = dict(tol=0.5, normal_k=16, normal_max_dist=INF, normal_min_pts=3, min_cos=COS20, max_curv=0.05, border=1, min_size=1, max_size=0)
NORMAL_KEYS = ("normal_k", "normal_max_dist", "normal_min_pts")
STATS = ("n", "smooth", "regions", "largest", "sel_regions", "unassigned", "sel_points")
# the settings of the standard scene: the issue's three
SETTINGS = (dict(normal_k=16, tol=0.15, min_cos=COS20, max_curv=0.05, border=0),
            dict(normal_k=16, tol=0.15, min_cos=COS20, max_curv=0.05, border=1),
            dict(normal_k=10, tol=0.2, min_cos=COS12, max_curv=0.02, border=1))


def cfg_of(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def bits32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def up(x):
    return F(np.nextafter(F(x), F(np.inf)))


def down(x):
    return F(np.nextafter(F(x), F(-np.inf)))


# ---- normals on the CPU -------------------------------------------------------------------------------------------------------------------
def cpu_normals(pts, k, max_dist=INF, min_pts=3):
    """float32 rows nx ny nz curvature after flimo_map_normals_range's rule without a viewpoint (fpfh_common.cpu_normals plus the
    curvature l0 / (l0 + l1 + l2), 0 for a zero sum): numpy's eigenvectors, not the device's bits; NaN rows below max(3, min_pts)
    neighbours."""
    from knn_k_common import brute_knn
    from normals_common import orient
    pts = np.asarray(pts, F).reshape(-1, 3)
    idx, _, cnt = brute_knn(pts, pts, k, max_dist, chunk=256)
    out = np.full((len(pts), 4), np.nan)
    ok = cnt >= max(3, int(min_pts))
    for c in np.unique(cnt[ok]):
        rows = np.nonzero(ok & (cnt == c))[0]
        r = pts[idx[rows, :c]].astype(D) - pts[rows].astype(D)[:, None, :]
        d = r - r.mean(1, keepdims=True)
        cov = np.einsum("nka,nkb->nab", d, d) / c
        w, v = np.linalg.eigh(cov)
        w = np.maximum(w, 0.0)
        out[rows, :3] = orient(v[:, :, 0], pts[rows], None)
        s = w.sum(1)
        out[rows, 3] = np.where(s > 0.0, w[:, 0] / np.where(s > 0.0, s, 1.0), 0.0)
    return out.astype(F)


# ---- the predicates -----------------------------------------------------------------------------------------------------------------------
def has_normal(nrm):
    return np.isfinite(np.asarray(nrm, F).reshape(-1, 4)).all(1)


def smooth(nrm, max_curv):
    nrm = np.asarray(nrm, F).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return has_normal(nrm) & (nrm[:, 3] <= F(max_curv))


def joined_block(pts, nrm, a, b, tol, min_cos):
    """[b - a, N] bool: both tests of an edge for the points a .. b - 1 against all, for points that have normals (float32, in the
    written association); and the float32 distances."""
    p, n = np.asarray(pts, F).reshape(-1, 3), np.asarray(nrm, F).reshape(-1, 4)
    d = cc.sqdist_block(p, a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = n[a:b, None, 0] * n[None, :, 0] + (n[a:b, None, 1] * n[None, :, 1] + n[a:b, None, 2] * n[None, :, 2])
        ok = (d < F(tol) * F(tol)) & (np.abs(dot) >= F(min_cos))
    h = has_normal(n)
    return ok & h[a:b, None] & h[None, :], d


def joined_pair(pi, ni, pj, nj, tol, min_cos, max_curv):
    """(smooth_i, smooth_j, joined) of one pair: flimo_region_joined_host restated."""
    p, n = F([pi, pj]).reshape(2, 3), F([ni, nj]).reshape(2, 4)
    s = smooth(n, max_curv)
    j, _ = joined_block(p, n, 0, 1, tol, min_cos)
    return bool(s[0]), bool(s[1]), bool(j[0, 1])


def edges(pts, nrm, tol, min_cos, max_curv, block=256):
    """(i, j) int64 arrays of every edge with i < j, by the dense predicate in blocks of rows."""
    s = smooth(nrm, max_curv)
    I, J = [], []
    for a in range(0, len(s), block):
        b = min(a + block, len(s))
        hit, _ = joined_block(pts, nrm, a, b, tol, min_cos)
        hit &= s[a:b, None] & s[None, :]
        i, j = np.nonzero(hit)
        keep = i + a < j
        I.append(i[keep] + a); J.append(j[keep])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)


def attach(pts, nrm, tol, min_cos, max_curv, block=256):
    """[N] int64: for a point that has a normal and is not smooth the smooth j of smallest (distance bits, j) that passes both tests
    against it, -1 where there is none and for every other point.  By sorted keys."""
    s, h = smooth(nrm, max_curv), has_normal(nrm)
    N = len(s)
    out = np.full(N, -1, np.int64)
    rows = np.flatnonzero(h & ~s)
    ar = np.arange(N, dtype=np.uint64)
    for a in range(0, N, block):
        b = min(a + block, N)
        mine = rows[(rows >= a) & (rows < b)]
        if not len(mine):
            continue
        hit, d = joined_block(pts, nrm, a, b, tol, min_cos)
        hit &= s[None, :]
        key = (bits32(d).astype(np.uint64) << np.uint64(32)) | ar[None, :]
        key[~hit] = np.uint64(0xFFFFFFFFFFFFFFFF)
        for r in mine:
            k = np.sort(key[r - a])[0]
            if k != np.uint64(0xFFFFFFFFFFFFFFFF):
                out[r] = int(k & np.uint64(0xFFFFFFFF))
    return out


def labels(pts, nrm, tol=0.5, min_cos=COS20, max_curv=0.05, border=1, **_):
    """label [N] int64 of the whole map: -1 for a point with no region."""
    s = smooth(nrm, max_curv)
    N = len(s)
    lab = cc.components(N, *edges(pts, nrm, tol, min_cos, max_curv)) if N else np.zeros(0, np.int64)
    lab = np.where(s, lab, -1)
    if border and N:
        j = attach(pts, nrm, tol, min_cos, max_curv)
        lab = np.where(j >= 0, lab[np.maximum(j, 0)], lab)
    return lab


def labels_bfs(pts, nrm, tol, min_cos, max_curv):
    """A second form of the components (no border): breadth-first search over the dense matrix, seeds in ascending order -- a seed
    is its region's smallest smooth index."""
    s = smooth(nrm, max_curv)
    N = len(s)
    adj = joined_block(pts, nrm, 0, N, tol, min_cos)[0] & s[:, None] & s[None, :] if N else np.zeros((0, 0), bool)
    label = np.full(N, -1, np.int64)
    for seed in np.flatnonzero(s):
        if label[seed] >= 0:
            continue
        label[seed] = seed
        front = [seed]
        while front:
            nxt = np.flatnonzero(adj[front].any(0) & (label < 0))
            label[nxt] = seed
            front = nxt.tolist()
    return label


def finish(label_all, nrm, max_curv, first=0, n=None, min_size=1, max_size=0, **_):
    """The outputs of flimo_map_regions from the whole map's labels."""
    label_all = np.asarray(label_all, np.int64)
    N = len(label_all)
    n = N - first if n is None else n
    has = label_all >= 0
    cnt = np.bincount(label_all[has], minlength=max(N, 1))[:N] if N else np.zeros(0, np.int64)
    size_all = np.where(has, cnt[np.maximum(label_all, 0)], 0) if N else np.zeros(0, np.int64)
    roots = np.flatnonzero(label_all == np.arange(N))
    sel_all = has & cc.selected(size_all, min_size, max_size)
    mask = sel_all[first:first + n]
    stats = dict(n=int(n), smooth=int(smooth(nrm, max_curv).sum()), regions=int(len(roots)), largest=int(cnt.max()) if N else 0,
                 sel_regions=int(sel_all[roots].sum()) if N else 0, unassigned=int((~has).sum()), sel_points=int(mask.sum()))
    return dict(label=label_all[first:first + n].astype(np.int32), size=size_all[first:first + n].astype(np.int32), mask=mask.astype(bool),
                stats=stats, sel_all=sel_all)


def listing(pts, label_all, nrm, max_curv, min_size=1, max_size=0, **_):
    """The outputs of flimo_map_region_list: the SHAPE written out as in voxels_common."""
    p = np.asarray(pts, F).reshape(-1, 3)
    fin = finish(label_all, nrm, max_curv, 0, None, min_size, max_size)
    idx = np.flatnonzero(fin["sel_all"])
    order = idx[np.lexsort((idx, np.asarray(label_all)[idx]))]          # by label, then by insertion index
    ls = np.asarray(label_all)[order]
    head = np.ones(len(order), bool)
    head[1:] = ls[1:] != ls[:-1]
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, len(order)))
    nr = len(start)
    vid = np.cumsum(head) - 1
    pd = p[order].astype(D)
    cd = count.astype(D)
    centroid = np.stack([vc.sum_shape(pd[:, a], start, count) / cd for a in range(3)], 1) if nr else np.zeros((0, 3))
    d = pd - centroid[vid] if nr else np.zeros((0, 3))
    cov = np.stack([vc.sum_shape(d[:, a] * d[:, b], start, count) / cd for a in range(3) for b in range(a, 3)], 1) if nr else np.zeros((0, 6))
    return dict(label=ls[start].astype(np.int32), count=count.astype(np.int32), first=order[start].astype(np.int32), centroid=centroid, cov=cov,
                nr=nr, stats=fin["stats"])


def restate(pts, nrm, first=0, n=None, **cfg):
    k = cfg_of(**cfg)
    out = finish(labels(pts, nrm, **k), nrm, k["max_curv"], first, n, k["min_size"], k["max_size"])
    out.pop("sel_all")
    return out


def same(got, want, what=""):
    """label, size, mask and every field of stats, with no tolerance."""
    for key in ("label", "size", "mask"):
        if key in got:
            np.testing.assert_array_equal(got[key], want[key], err_msg="%s %s" % (what, key))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


def same_listing(got, want, what=""):
    """Integers with no tolerance, every float64 bit for bit."""
    assert got["nr"] == want["nr"], (what, got["nr"], want["nr"])
    for key in ("label", "count", "first"):
        if key in got:
            np.testing.assert_array_equal(got[key], want[key], err_msg="%s %s" % (what, key))
    for key in ("centroid", "cov"):
        if key in got:
            np.testing.assert_array_equal(vc.bits(got[key]), vc.bits(want[key]), err_msg="%s %s (bits)" % (what, key))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def scene():
    """Two planes meeting at an edge and a cylinder standing on one of them, 5 060 points: fpfh_common.scene()."""
    import fpfh_common as fc
    return fc.scene()


@functools.lru_cache(maxsize=None)
def scene_surface():
    """The surface of every point of ``scene()``, recomputed from the scene's seed: 0 floor, 1 wall, 2 cylinder."""
    rs = np.random.RandomState(7)
    rs.normal(0.0, 0.01, (5060, 3))
    order = rs.permutation(5060)
    surf = np.concatenate([np.zeros(1600, np.int64), np.ones(1600, np.int64), np.full(1860, 2, np.int64)])[order]
    pts = scene()
    # (the generator's geometry: a floor point has z near 0, a wall point x near 0, a cylinder point lies 1 m from its axis)
    rad = np.hypot(pts[:, 0] - 2.5, pts[:, 1] - 2.0)
    assert np.all(np.abs(pts[surf == 0, 2]) < 0.06) and np.all(np.abs(pts[surf == 1, 0]) < 0.06) and np.all(np.abs(rad[surf == 2] - 1.0) < 0.06)
    return surf


def recovery(label, surf, min_size=100):
    """(the labels of the regions of at least min_size points, the share of each one's members that lie on its commonest surface,
    the points in them)."""
    label = np.asarray(label)
    labs, cnt = np.unique(label[label >= 0], return_counts=True)
    big = labs[cnt >= min_size]
    purity = [float(np.bincount(surf[label == r], minlength=3).max()) / float((label == r).sum()) for r in big]
    return big, purity, int(np.isin(label, big).sum())


def tie_case(swap=False):
    """Two 8 x 8 lattice patches (spacing 0.125) at z = 0 and z = 1 and the point (0.5, 0.5, 0.5) between them, 129 points: the
    middle point's two nearest lattice points, (0.5, 0.5, 0) and (0.5, 0.5, 1), are exactly equally far.  swap: the upper patch is
    inserted first.  The middle point is the last."""
    g = np.arange(8) * 0.125
    a, b = np.meshgrid(g, g, indexing="ij")
    lo = np.stack([a.ravel(), b.ravel(), np.zeros(64)], 1)
    hi = lo + [0.0, 0.0, 1.0]
    return np.concatenate(([hi, lo] if swap else [lo, hi]) + [[[0.5, 0.5, 0.5]]]).astype(F)


TIE_CFG = dict(tol=0.6, min_cos=0.0, max_curv=0.01, border=1)


def hand_regions(counts=((7, 9), (8, 8), (5, 13), (25, 41)), seed=11):
    """Flat lattice patches (spacing 0.1) of exactly a * b points each -- 63, 64, 65 and 1 025 --, 8 m apart along x at different
    heights, all in one seeded random order.  Returns (points, the patch of each point)."""
    rs = np.random.RandomState(seed)
    pts, which = [], []
    for t, (na, nb) in enumerate(counts):
        a, b = np.meshgrid(np.arange(na) * 0.1, np.arange(nb) * 0.1, indexing="ij")
        pts.append(np.stack([8.0 * t + a.ravel(), b.ravel(), np.full(a.size, 0.5 * t)], 1))
        which.append(np.full(a.size, t))
    pts, which = np.concatenate(pts), np.concatenate(which)
    o = rs.permutation(len(pts))
    pts, which = pts[o].astype(F), which[o]
    pts.setflags(write=False)
    return pts, which


def gated_scene():
    """The scene plus five points far from everything and from each other: under a normal gate of 0.5 m each has nothing but
    itself inside the gate, so it has no normal."""
    far = F([[4.04 + 3.0 * t, 9.0, 5.0 + t] for t in range(5)])
    pts = np.concatenate([scene()[:2000], far[:2], scene()[2000:], far[2:]]).astype(F)
    pts.setflags(write=False)
    return pts


def moved(pts, by=(10000.0, -10000.0, 250.0)):
    out = (np.asarray(pts, D) + np.asarray(by, D)).astype(F)
    out.setflags(write=False)
    return out
