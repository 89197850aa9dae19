"""Shared helpers of the cluster tests (flimo_map_clusters / flimo_map_remove_clusters): the definition restated, and the scenes.

The definition (include/flimo_c.h), restated:
 * the vertices are the N stored points in insertion order (the order flimo_map_points returns and flimo_knn_k indexes);
 * {i, j}, i != j, is an edge iff sqdist3(p_i, p_j) < tol * tol -- strict, all float32, sqdist3 = dx*dx + (dy*dy + dz*dz)
   uncontracted, tol * tol one float32 product: flimo_radius_search's predicate with a stored point as the query, symmetric bit for
   bit because a - b and b - a differ by sign only;
 * tol == 0: no edges, every point (exact duplicates included) is its own cluster; with tol > 0 exact duplicates share one;
 * a cluster is a connected component of that graph over the WHOLE map, whatever the range;
 * label[i] = the smallest insertion index in the component of stored point first + i, size[i] = that component's points;
 * a component is selected iff min_size <= size and (max_size == 0 or size <= max_size); mask[i] = 1 iff the component of point
   first + i is selected;
 * stats: n = points of the range; clusters, largest, sel_clusters over the whole map; sel_points = ones of the mask.
Every output is an integer with one correct value, and numpy's float32 arithmetic is the device's bit for bit: no tolerance
anywhere, no pair left out.  ``restate`` is a dense predicate (in blocks of rows) and a plain union-find in Python; it uses no scipy."""
import functools

import numpy as np

F = np.float32
DEFAULTS = dict(tol=0.5, min_size=1, max_size=0)


def sqdist_block(pts, a, b):
    """[b - a, N] float32: sqdist3 of the points a .. b - 1 against all, in the written association."""
    p = np.asarray(pts, F).reshape(-1, 3)
    dx, dy, dz = p[a:b, None, 0] - p[None, :, 0], p[a:b, None, 1] - p[None, :, 1], p[a:b, None, 2] - p[None, :, 2]
    return dx * dx + (dy * dy + dz * dz)


def edges(pts, tol, block=256):
    """(i, j) int64 arrays of every edge with i < j, by the dense predicate in blocks of rows."""
    p = np.asarray(pts, F).reshape(-1, 3)
    r2 = F(tol) * F(tol)                                     # one float32 product
    I, J = [], []
    for a in range(0, len(p), block):
        b = min(a + block, len(p))
        hit = sqdist_block(p, a, b) < r2
        i, j = np.nonzero(hit)
        keep = i + a < j
        I.append(i[keep] + a); J.append(j[keep])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)


def components(n, I, J):
    """label [n]: the smallest index of each vertex' component, by a plain union-find (the smaller root stays a root)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(I.tolist(), J.tolist()):
        a, b = find(i), find(j)
        if a != b:
            if a < b:
                parent[b] = a
            else:
                parent[a] = b
    return np.array([find(x) for x in range(n)], np.int64).reshape(n)


def selected(size, min_size, max_size):
    size = np.asarray(size)
    return (size >= min_size) & ((size <= max_size) if max_size > 0 else np.ones(size.shape, bool))


def finish(label_all, first=0, n=None, min_size=1, max_size=0):
    """The outputs of the call from the whole map's labels."""
    N = len(label_all)
    n = N - first if n is None else n
    cnt = np.bincount(label_all, minlength=max(N, 1))[:N] if N else np.zeros(0, np.int64)
    size_all = cnt[label_all] if N else np.zeros(0, np.int64)
    roots = np.flatnonzero(label_all == np.arange(N))
    sel_all = selected(size_all, min_size, max_size)
    mask = sel_all[first:first + n]
    stats = dict(n=int(n), clusters=int(len(roots)), largest=int(cnt.max()) if N else 0, sel_clusters=int(sel_all[roots].sum()) if N else 0,
                 sel_points=int(mask.sum()))
    return dict(label=label_all[first:first + n].astype(np.int32), size=size_all[first:first + n].astype(np.int32), mask=mask.astype(bool), stats=stats)


def labels(pts, tol):
    p = np.asarray(pts, F).reshape(-1, 3)
    return components(len(p), *edges(p, tol))


def restate(pts, first=0, n=None, tol=0.5, min_size=1, max_size=0):
    return finish(labels(pts, tol), first, n, min_size, max_size)


def labels_bfs(pts, tol):
    """A second form: breadth-first search over the dense matrix, seeds in ascending order (a seed is its component's smallest index)."""
    p = np.asarray(pts, F).reshape(-1, 3)
    N = len(p)
    adj = (sqdist_block(p, 0, N) < F(tol) * F(tol)) if N else np.zeros((0, 0), bool)
    label = np.full(N, -1, np.int64)
    for s in range(N):
        if label[s] >= 0:
            continue
        label[s] = s
        front = [s]
        while front:
            nxt = np.flatnonzero(adj[front].any(0) & (label < 0))
            label[nxt] = s
            front = nxt.tolist()
    return label


def same(got, want, what=""):
    """label, size, mask and every field of stats, with no tolerance."""
    for key in ("label", "size", "mask"):
        if key in got:
            np.testing.assert_array_equal(got[key], want[key], err_msg="%s %s" % (what, key))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


def below(x):
    """One float32 step towards zero."""
    return F(np.nextafter(F(x), F(0)))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    """Two jittered planes and a cylinder (spacing 0.1 m, 5 060 points: tests/fpfh_common.py) plus 40 Gaussian blobs of 1 to 60
    points (sigma 4 cm) on a 1 m lattice set away from the surfaces: 6 000 to 7 000 points in all, in a seeded random order."""
    import fpfh_common as fc
    rs = np.random.RandomState(21)
    slots = np.array([(x, y, z) for x in range(5, 10) for y in range(0, 5) for z in (1, 2, 3, 4)], np.float64)
    centres = slots[rs.permutation(len(slots))[:40]]
    sizes = np.concatenate([[1, 1, 2, 3, 59, 60], rs.randint(1, 61, 34)])
    blobs = np.concatenate([c + rs.normal(0.0, 0.04, (m, 3)) for c, m in zip(centres, sizes)])
    pts = np.concatenate([np.asarray(fc.scene(), np.float64), blobs])
    pts = pts[rs.permutation(len(pts))].astype(F)
    assert 4000 <= len(pts) <= 8000 and len(np.unique(pts, axis=0)) == len(pts)
    pts.setflags(write=False)
    return pts


SCENE_TOLS = (0.06, 0.105, 0.9)     # thousands of single points; the surfaces half joined (the spacing is 0.1 m); blobs joining blobs


def lattice(nx=16, ny=16, nz=8):
    """A unit lattice: neighbours exactly 1 apart in float32."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(F)


def pair_at(d):
    """Two small clusters whose closest points, (0, 1, 1) and (d, 1, 1), are exactly d apart: the difference is d itself."""
    a = F([[0.0, 1.0, 1.0], [-0.25, 1.0, 1.0], [-0.25, 1.25, 1.0]])
    b = F([[F(d), 1.0, 1.0], [F(d) + F(0.25), 1.0, 1.0], [F(d) + F(0.25), 1.0, 1.25]])
    assert F(b[0, 0] - a[0, 0]) == F(d)
    return np.concatenate([a, b]).astype(F)


@functools.lru_cache(maxsize=None)
def chains(tol=0.25, n=5000, seed=4):
    """Two gentle helices in one map, each of n points spaced 0.8 * tol along the curve, the second passing the first at 1.5 * tol
    (the same helix shifted along its axis by 1.5 * tol: the pitch is far larger), in a seeded random order.  Returns (points,
    chain of each point)."""
    step = 0.8 * tol
    R, pitch = 20.0, 6.0                                       # metres of radius, metres of rise per turn
    per_rad = np.hypot(R, pitch / (2 * np.pi))                 # arc length per radian
    th = np.arange(n) * (step / per_rad)
    one = np.stack([R * np.cos(th), R * np.sin(th), th * pitch / (2 * np.pi)], 1)
    two = one + [0.0, 0.0, 1.5 * tol]
    pts = np.concatenate([one, two])
    which = np.repeat([0, 1], n)
    order = np.random.RandomState(seed).permutation(2 * n)
    pts, which = pts[order].astype(F), which[order]
    pts.setflags(write=False)
    return pts, which


@functools.lru_cache(maxsize=None)
def duplicates(seed=8):
    """200 scattered points, then one point stored 300 times, then 200 more."""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0, 6, (200, 3)), rs.uniform(0, 6, (200, 3))
    pts = np.concatenate([a, np.tile([[2.5, 2.5, 2.5]], (300, 1)), b]).astype(F)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def sparse(seed=13):
    """A few hundred points over hundreds of metres: 60 groups of 5 points (0.5 m across) scattered over 800 m x 800 m x 40 m."""
    rs = np.random.RandomState(seed)
    c = np.stack([rs.uniform(-400, 400, 60), rs.uniform(-400, 400, 60), rs.uniform(0, 40, 60)], 1)
    pts = (c[:, None, :] + rs.uniform(-0.25, 0.25, (60, 5, 3))).reshape(-1, 3)
    pts = pts[rs.permutation(len(pts))].astype(F)
    pts.setflags(write=False)
    return pts


def small(n, seed=0):
    """n points of a cloud in which both edges and isolated points occur at tol 0.5."""
    return np.random.RandomState(100 + seed + n).uniform(0, 0.45 * max(n, 2) ** (1 / 3) + 0.5, (n, 3)).astype(F)


def plan(layout, tol):
    """radius_plan (flimo_radius.hip) restated from a context's ``map_index_layout()``: "8", "16", "64" lanes a point, or "tiles"."""
    import math
    span = 2.0 * math.ceil(float(tol) / float(layout["cell"])) + 1.0
    rows = min(span, float(layout["ny"])) * min(span, float(layout["nz"]))
    return "tiles" if rows > 4096.0 else ("8" if rows <= 9.0 else ("16" if rows <= 25.0 else "64"))


CARVE_TOL, M_CARVE = 0.2, 8         # tests/test_clusters_host.py: how they were chosen, and what they cannot do on this scene


@functools.lru_cache(maxsize=None)
def carve_residue_scene():
    """The scene of tests/test_gpu_carve.py's departed object after the standard carve, restated on the CPU: (the stored points
    left, in insertion order; which of them are the ghost's)."""
    import carve_common as cv
    static, ghost, scan, x26, sensor = cv.standard_scene()
    mp = np.concatenate([static, ghost]).astype(F)
    gone = cv.yardstick(cv.standard_world(scan, x26), mp, sensor, **cv.STD_CFG)
    return mp[~gone], (np.arange(len(mp)) >= len(static))[~gone]
