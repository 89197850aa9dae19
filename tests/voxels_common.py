"""Shared helpers of the voxel tests (flimo_map_voxels / flimo_map_voxel_mask / flimo_map_thin): the definition restated, and the maps.

The definition (include/flimo_c.h), restated:
 * stored point i (insertion order) is p_i, float32, finite;
 * the lattice is anchored at the world origin: inv = float32(1) / float32(leaf), c_a = floor(p_a * inv) in float32 per axis; a
   point is OUTSIDE when any |c_a| >= 2^20; otherwise key = ((cz + 2^20) << 42) | ((cy + 2^20) << 21) | (cx + 2^20);
 * the voxels are the occupied keys of the WHOLE map in ascending key = ascending (cz, cy, cx); voxel v has the members
   m_0 < m_1 < ... (insertion indices): ijk = (cx, cy, cz), count, first = m_0;
 * the SHAPE of a float64 sum over u_0 .. u_{c-1} in member order: runs of 64 slots (absent: +0.0), each run the pairwise tree
   ((u0 + u1) + (u2 + u3)) + ..., then S = ((+0.0 + R_0) + R_1) + ... over the runs in ascending order;
 * centroid = SHAPE over (double)p / (double)c; cov = (xx, xy, xz, yy, yz, zz), each the SHAPE over d_a * d_b with
   d = (double)p - centroid, / (double)c; rep = m_0 (KEEP_FIRST) or the member of smallest q = dx*dx + (dy*dy + dz*dz), ties to the
   smallest insertion index (KEEP_NEAREST);
 * mask: KEEP_FIRST with max_pts = m: a point goes iff its rank among its voxel's members is >= m; KEEP_NEAREST: iff it is not rep;
 * voxel[i]: the position of the point's voxel in the listing, -1 outside; stats: n, voxels, largest, outside, sel_points.
Every output has one correct value and numpy's float32 / float64 arithmetic is the device's bit for bit: no tolerance anywhere.
``sum_shape`` is the SHAPE as a reshape-and-add over many voxels at once, ``sum_shape_plain`` the same in plain Python floats."""
import functools

import numpy as np

F = np.float32
D = np.float64
RUN = 64
HALF = 1 << 20
KEEP_FIRST, KEEP_NEAREST = 0, 1
OUTSIDE_KEY = (1 << 64) - 1
DEFAULTS = dict(leaf=0.25, keep=KEEP_FIRST, max_pts=1)
BAD_CFGS = (dict(leaf=float("nan")), dict(leaf=0.0), dict(leaf=-0.5), dict(leaf=float("inf")), dict(leaf=1e-39), dict(keep=-1), dict(keep=2),
            dict(max_pts=0), dict(max_pts=-3), dict(keep=KEEP_NEAREST, max_pts=2))


def cfg_of(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def bits(a):
    return np.ascontiguousarray(a, D).view(np.uint64)


def up(x):
    return F(np.nextafter(F(x), F(np.inf)))


def down(x):
    return F(np.nextafter(F(x), F(-np.inf)))


# ---- the lattice ------------------------------------------------------------------------------------------------------------------------
def cells(pts, leaf):
    """(c [N, 3] float32: the floors, inside [N] bool)."""
    p = np.asarray(pts, F).reshape(-1, 3)
    inv = F(1.0) / F(leaf)                                   # one float32 division
    c = np.floor(p * inv)                                    # one float32 product, then floorf
    return c, np.all(np.abs(c) < F(HALF), axis=1)


def keys(pts, leaf):
    """(ijk [N, 3] int32 -- 0 for an outside point --, key [N] uint64 -- all ones for an outside point --, inside [N])."""
    c, inside = cells(pts, leaf)
    ijk = np.where(inside[:, None], c, F(0)).astype(np.int64)
    k = ((ijk[:, 2] + HALF).astype(np.uint64) << np.uint64(42)) | ((ijk[:, 1] + HALF).astype(np.uint64) << np.uint64(21)) | \
        (ijk[:, 0] + HALF).astype(np.uint64)
    k = np.where(inside, k, np.uint64(OUTSIDE_KEY))
    return ijk.astype(np.int32), k, inside


def group(pts, leaf):
    """The voxels of the map: dict(order [M]: the insertion indices of the inside points sorted by (cz, cy, cx, index), start [nv],
    count [nv], ijk [nv, 3], vid [M]: the voxel of each sorted position, inside [N])."""
    ijk, _, inside = keys(pts, leaf)
    idx = np.flatnonzero(inside)
    c = ijk[idx]
    order = idx[np.lexsort((idx, c[:, 0], c[:, 1], c[:, 2]))]          # (the last key is the primary one)
    cs = ijk[order]
    head = np.ones(len(order), bool)
    head[1:] = np.any(cs[1:] != cs[:-1], axis=1)
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, len(order)))
    vid = np.cumsum(head) - 1
    return dict(order=order, start=start, count=count, ijk=cs[start].astype(np.int32), vid=vid, inside=inside)


# ---- the SHAPE --------------------------------------------------------------------------------------------------------------------------
def sum_shape(vals, start=None, count=None):
    """The SHAPE of every voxel's sum: vals [M] float64 in sorted member order, the voxels at start / count (default: one voxel of
    all M values).  Runs of 64 by a reshape, the tree by adding neighbouring columns, the runs in a loop that adds whole columns."""
    vals = np.ascontiguousarray(vals, D).reshape(-1)
    one = start is None
    if one:
        start, count = np.array([0]), np.array([len(vals)])
    start, count = np.asarray(start, np.int64), np.asarray(count, np.int64)
    runs = (count + RUN - 1) // RUN
    out = np.zeros(len(start), D)                            # (+0.0)
    for r in np.unique(runs):
        if r == 0:
            continue
        sel = np.flatnonzero(runs == r)
        slot = np.arange(r * RUN)
        have = slot[None, :] < count[sel, None]
        at = np.minimum(start[sel, None] + slot[None, :], max(len(vals) - 1, 0))
        a = np.where(have, vals[at], D(0.0)).reshape(len(sel), r, RUN)
        while a.shape[2] > 1:
            a = a[:, :, 0::2] + a[:, :, 1::2]
        S = np.zeros(len(sel), D)
        for j in range(r):
            S = S + a[:, j, 0]
        out[sel] = S
    return out[0] if one else out


def sum_shape_plain(u):
    """The same for one voxel, written out in plain Python floats."""
    u = [float(x) for x in u]
    S = 0.0
    for j in range(0, len(u), RUN):
        t = u[j:j + RUN] + [0.0] * (RUN - len(u[j:j + RUN]))
        while len(t) > 1:
            t = [t[i] + t[i + 1] for i in range(0, len(t), 2)]
        S = S + t[0]
    return S


def sum_shape_butterfly(u):
    """... and as the butterfly t[s] += t[s ^ o], o = 1 .. 32, every slot ending with the run's sum."""
    u = [float(x) for x in u]
    S = 0.0
    for j in range(0, len(u), RUN):
        t = u[j:j + RUN] + [0.0] * (RUN - len(u[j:j + RUN]))
        o = 1
        while o < RUN:
            t = [t[s] + t[s ^ o] for s in range(RUN)]
            o *= 2
        assert all(np.float64(x).tobytes() == np.float64(t[0]).tobytes() for x in t)
        S = S + t[0]
    return S


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def restate(pts, first=0, n=None, leaf=0.25, keep=KEEP_FIRST, max_pts=1):
    p = np.asarray(pts, F).reshape(-1, 3)
    N = len(p)
    n = N - first if n is None else n
    g = group(p, leaf)
    order, start, count, vid = g["order"], g["start"], g["count"], g["vid"]
    nv = len(start)
    pd = p[order].astype(D)
    cd = count.astype(D)
    centroid = np.stack([sum_shape(pd[:, a], start, count) / cd for a in range(3)], 1) if nv else np.zeros((0, 3))
    d = pd - centroid[vid] if nv else np.zeros((0, 3))
    cov = np.stack([sum_shape(d[:, a] * d[:, b], start, count) / cd for a in range(3) for b in range(a, 3)], 1) if nv else np.zeros((0, 6))
    q = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    pos = np.arange(len(order))
    by_q = np.lexsort((pos, q, vid))                         # per voxel: ascending q, then ascending member rank
    nearest = order[by_q[start]] if nv else np.zeros(0, np.int64)      # (by_q keeps the voxels' segments where they are)
    firstm = order[start] if nv else np.zeros(0, np.int64)
    rep = firstm if keep == KEEP_FIRST else nearest
    rank = pos - start[vid] if nv else pos
    goes_sorted = (rank >= max_pts) if keep == KEEP_FIRST else (order != rep[vid])
    voxel_all = np.full(N, -1, np.int64)
    voxel_all[order] = vid
    mask_all = np.zeros(N, bool)
    mask_all[order] = goes_sorted
    mask = mask_all[first:first + n]
    stats = dict(n=int(n), voxels=int(nv), largest=int(count.max()) if nv else 0, outside=int(N - len(order)), sel_points=int(mask.sum()))
    return dict(ijk=g["ijk"], count=count.astype(np.int32), first=firstm.astype(np.int32), rep=rep.astype(np.int32), centroid=centroid,
                cov=cov, nearest=nearest.astype(np.int32), voxel=voxel_all[first:first + n].astype(np.int32), mask=mask, nv=nv, stats=stats,
                q=q, order=order, vid=vid)


def restate_plain(pts, leaf):
    """centroid, cov and the nearest member of every voxel in plain Python floats, voxel by voxel (small maps)."""
    p = np.asarray(pts, F).reshape(-1, 3)
    g = group(p, leaf)
    cen, cov, near = [], [], []
    for s, c in zip(g["start"], g["count"]):
        m = g["order"][s:s + c]
        x = [[float(v) for v in p[i]] for i in m]
        ce = [sum_shape_plain([r[a] for r in x]) / float(c) for a in range(3)]
        d = [[r[a] - ce[a] for a in range(3)] for r in x]
        cov.append([sum_shape_plain([r[a] * r[b] for r in d]) / float(c) for a in range(3) for b in range(a, 3)])
        qs = [r[0] * r[0] + (r[1] * r[1] + r[2] * r[2]) for r in d]
        near.append(int(m[min(range(len(m)), key=lambda t: (qs[t], t))]))
        cen.append(ce)
    return np.array(cen, D).reshape(-1, 3), np.array(cov, D).reshape(-1, 6), np.array(near, np.int32)


def same(got, want, what="", keys=("ijk", "count", "first", "rep", "voxel", "mask"), floats=("centroid", "cov")):
    """Integers with no tolerance, every float64 bit for bit."""
    for k in keys:
        if k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))
    for k in floats:
        if k in got:
            np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg="%s %s (bits)" % (what, k))
    if "nv" in got:
        assert got["nv"] == want["nv"], (what, got["nv"], want["nv"])
    if "stats" in got:
        assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


# ---- maps -------------------------------------------------------------------------------------------------------------------------------
def scene():
    """Two planes, a cylinder and forty blobs: the clusters' scene."""
    import clusters_common as cc
    return cc.scene()


SCENE_LEAVES = (0.1, 0.25, 1.0)
HAND_COUNTS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4097)


def small(n, seed=0):
    """n points of which some share a voxel at leaf 0.25."""
    return np.random.RandomState(300 + seed + n).uniform(-0.4, 0.4 + 0.02 * n ** 0.5, (n, 3)).astype(F)


@functools.lru_cache(maxsize=None)
def hand_voxels(leaf=0.5, seed=5):
    """Voxels built to hold exactly HAND_COUNTS points: voxel t is the cell (3 t - 15, 2, -1) of a lattice of edge ``leaf``, its
    points drawn well inside it, all in one seeded random order.  Returns (points, the cell's x index of each point)."""
    rs = np.random.RandomState(seed)
    pts, which = [], []
    for t, c in enumerate(HAND_COUNTS):
        cx = 3 * t - 15
        lo = np.array([cx, 2, -1], D) * leaf
        pts.append(lo + rs.uniform(0.05, 0.95, (c, 3)) * leaf)
        which.append(np.full(c, cx))
    pts, which = np.concatenate(pts), np.concatenate(which)
    o = rs.permutation(len(pts))
    pts, which = pts[o].astype(F), which[o]
    pts.setflags(write=False)
    return pts, which


@functools.lru_cache(maxsize=None)
def one_voxel(n=16385, seed=6):
    """n points inside the one cell (0, 0, 0) of a 4 m lattice."""
    pts = np.random.RandomState(seed).uniform(0.01, 3.99, (n, 3)).astype(F)
    pts.setflags(write=False)
    return pts


def dyadic_lattice():
    """Small dyadic coordinates, on which every sum is exact: at leaf 1 the cell (0, 0, 0) holds the eight corners of a cube of edge
    0.5 at 0.25 .. 0.75 -- all eight exactly equidistant from the centroid (0.5, 0.5, 0.5) -- and the cell (1, 0, 0) the four points
    (1.25, 0.25, 0.5), (1.75, 0.25, 0.5), (1.25, 0.75, 0.5), (1.5, 0.5, 0.5): the last IS the centroid of the other three's box, the
    centroid of the four is (1.4375, 0.4375, 0.5)."""
    cube = [(x, y, z) for z in (0.25, 0.75) for y in (0.25, 0.75) for x in (0.25, 0.75)]
    four = [(1.25, 0.25, 0.5), (1.75, 0.25, 0.5), (1.25, 0.75, 0.5), (1.5, 0.5, 0.5)]
    return F(cube[::-1] + four)                              # (the cube reversed: its first member is (0.75, 0.75, 0.75))


@functools.lru_cache(maxsize=None)
def duplicates(seed=8):
    """200 scattered points, then one point stored 300 times, then 200 more."""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0, 6, (200, 3)), rs.uniform(0, 6, (200, 3))
    pts = np.concatenate([a, np.tile([[2.5, 2.5, 2.5]], (300, 1)), b]).astype(F)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def far_away(seed=9):
    """1 500 points in a 6 m box 10 km from the origin (a float32 step is about 1 mm there)."""
    rs = np.random.RandomState(seed)
    pts = (np.array([10000.0, -10000.0, 250.0]) + rs.uniform(0, 6, (1500, 3))).astype(F)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def with_outside(seed=10):
    """600 points within 5 m of the origin, 50 of them stored twice, and 40 with |x| > 1 100 m: at leaf 0.001 the latter lie
    outside the lattice."""
    rs = np.random.RandomState(seed)
    near = rs.uniform(-5, 5, (550, 3))
    near = np.concatenate([near, near[:50]])
    far = rs.uniform(-5, 5, (40, 3))
    far[:, 0] = np.where(rs.rand(40) < 0.5, -1.0, 1.0) * rs.uniform(1100, 1500, 40)
    pts = np.concatenate([near, far])
    pts = pts[rs.permutation(len(pts))].astype(F)
    pts.setflags(write=False)
    return pts
