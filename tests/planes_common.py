"""Shared helpers of the plane tests (flimo_map_planes / flimo_map_plane_mask / flimo_map_remove_plane): the definition restated, and
the scenes.

The definition (include/flimo_c.h), restated.  Hypothesis j is the triplet (a, b, c) = tri[j] of insertion indices.  Steps 1-6 are
float64 on the float32 points widened, in exactly the written association; sq(v) = v.x*v.x + (v.y*v.y + v.z*v.z):
 1. e1 = b - a, e2 = c - a, e3 = c - b; DEGENERATE if two indices are equal or a squared edge fails >= min_edge^2;
 2. cr = e1 x e2, q = sq(cr); DEGENERATE unless q > 0 and q >= min_sin^2 * (sq(e1) * sq(e2));
 3. n = cr / sqrt(q); DEGENERATE if an entry is not finite;
 4. the component of largest magnitude is made positive, the lowest axis on equal magnitudes;
 5. REJECTED if min_cos > 0 and not |n . axis| >= min_cos (the axis as given);
 6. d = -(n . a), plane = (n, d), nf = float32(n);
 7. float32, anchored: v = p_i - p_a, t = nf.x*v.x + (nf.y*v.y + nf.z*v.z); inlier iff |t| < dist;
 8. inliers = the count over all stored points;
 9. sum_sq = the float64 sum of float64(t)^2 over the inliers in one shape: slabs of 8192 points; thread T of 256 adds the slab's
    slots T, T + 256, ... in ascending order from +0.0; partial[T] += partial[T + o], o = 128 .. 1; the slabs in ascending order.
numpy's float32 and float64 arithmetic is IEEE and uncontracted, as the device's: every comparison is exact, no tolerance anywhere.
``sum_shape_plain`` is step 9 in plain Python floats, one addition a line of the loop; ``sum_shape`` is the same in numpy."""
import functools

import numpy as np

F = np.float32
D = np.float64
OK, DEGENERATE, REJECTED = 0, 1, 2
SLAB, RED = 8192, 256
SHIPPED_G, SHIPPED_W = 16, 1       # flimo_plane.hip: survivors whose trees share the barriers, groups a workgroup walks
DEFAULTS = dict(dist=0.05, min_edge=0.0, min_sin=0.0, axis=(0.0, 0.0, 1.0), min_cos=0.0)
REC_CFG = dict(dist=0.03, min_edge=0.3, min_sin=0.2, axis=(0.0, 0.0, 1.0), min_cos=0.95)      # the recovery's
REC_NH, REC_REMOVE_DIST, REC_TOL = 1024, 0.05, 0.16

# every cfg flimo_map_planes and flimo_plane_solve_host refuse, as changes to DEFAULTS
BAD_CFGS = [dict(dist=np.nan), dict(dist=-1.0), dict(min_edge=np.nan), dict(min_edge=-0.1), dict(min_sin=np.nan), dict(min_sin=-0.1),
            dict(min_sin=float(np.nextafter(F(1), F(2)))), dict(min_cos=np.nan), dict(min_cos=-0.1), dict(min_cos=1.5),
            dict(min_cos=0.5, axis=(np.nan, 0, 1)), dict(min_cos=0.5, axis=(0, np.inf, 1)), dict(min_cos=0.5, axis=(0, 0, -np.inf))]


def cfg_of(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def sq(x, y, z):
    return x * x + (y * y + z * z)


def solve(p3, min_edge=0.0, min_sin=0.0, axis=(0.0, 0.0, 1.0), min_cos=0.0, dist=None):
    """Steps 1-6 for one triplet of POINTS p3 [3, 3] float32: (status, plane4 float64 [4], nf float32 [3]); NaN unless OK."""
    nanp, nanf = np.full(4, np.nan), np.full(3, np.nan, F)
    p = np.asarray(p3, F).reshape(3, 3).astype(D)
    min_edge, min_sin, min_cos = F(min_edge), F(min_sin), F(min_cos)
    with np.errstate(all="ignore"):
        a, b, c = p[0], p[1], p[2]
        e1, e2, e3 = b - a, c - a, c - b
        l1, l2, l3 = sq(*e1), sq(*e2), sq(*e3)
        min2 = D(min_edge) * D(min_edge)
        if not (l1 >= min2) or not (l2 >= min2) or not (l3 >= min2):
            return DEGENERATE, nanp, nanf
        cr = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], D)
        q = sq(*cr)
        s2 = D(min_sin) * D(min_sin)
        if not (q > 0.0) or not (q >= s2 * (l1 * l2)):
            return DEGENERATE, nanp, nanf
        n = cr / np.sqrt(q)
        if not np.all(np.isfinite(n)):
            return DEGENERATE, nanp, nanf
        k = 0
        if abs(n[1]) > abs(n[k]):
            k = 1
        if abs(n[2]) > abs(n[k]):
            k = 2
        if n[k] < 0.0:
            n = -n
        if min_cos > 0:
            ax = np.asarray(axis, F).astype(D)
            if not (abs(n[0] * ax[0] + (n[1] * ax[1] + n[2] * ax[2])) >= D(min_cos)):
                return REJECTED, nanp, nanf
        d = -(n[0] * a[0] + (n[1] * a[1] + n[2] * a[2]))
    return OK, np.array([n[0], n[1], n[2], d], D), n.astype(F)


def signed_t(pts, nf, anchor):
    """Step 7's t [N] float32 of every point against the plane of float32 normal nf through the float32 anchor."""
    p = np.asarray(pts, F).reshape(-1, 3)
    nf, an = np.asarray(nf, F).reshape(3), np.asarray(anchor, F).reshape(3)
    with np.errstate(all="ignore"):
        vx, vy, vz = p[:, 0] - an[0], p[:, 1] - an[1], p[:, 2] - an[2]
        return (nf[0] * vx + (nf[1] * vy + nf[2] * vz)).astype(F)


def sum_shape(tt):
    """Step 9 in numpy: tt [..., N] float64, the term of every slot (+0.0 for a non-inlier: adding it changes no bit of a partial
    that is never -0.0).  Returns [...] float64."""
    tt = np.asarray(tt, D)
    lead, N = tt.shape[:-1], tt.shape[-1]
    slabs = (N + SLAB - 1) // SLAB
    pad = np.zeros(lead + (slabs * SLAB,), D)
    pad[..., :N] = tt
    x = pad.reshape(lead + (slabs, SLAB // RED, RED))
    part = np.zeros(lead + (slabs, RED), D)
    for r in range(SLAB // RED):
        part = part + x[..., r, :]
    o = RED // 2
    while o >= 1:
        part[..., :o] = part[..., :o] + part[..., o:2 * o]
        o //= 2
    S = np.zeros(lead, D)
    for s in range(slabs):
        S = S + part[..., s, 0]
    return S


def sum_shape_plain(t, inside):
    """Step 9 in plain Python floats: t [N] float32, inside [N] bool."""
    t = [float(v) for v in np.asarray(t, F)]
    inside = [bool(v) for v in inside]
    N = len(t)
    S = 0.0
    for s in range((N + SLAB - 1) // SLAB):
        lo, hi = s * SLAB, min(N, (s + 1) * SLAB)
        partial = [0.0] * RED
        for T in range(RED):
            for i in range(lo + T, hi, RED):
                if inside[i]:
                    partial[T] = partial[T] + t[i] * t[i]
        o = RED // 2
        while o >= 1:
            for T in range(o):
                partial[T] = partial[T] + partial[T + o]
            o //= 2
        S = S + partial[0]
    return S


def restate(pts, tri, **cfg):
    """status, inliers [nh] int32, sum_sq [nh], plane [nh, 4] of the call, from the definition."""
    cfg = cfg_of(**cfg)
    p = np.asarray(pts, F).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nh, N = len(tri), len(p)
    status, inliers = np.zeros(nh, np.int32), np.zeros(nh, np.int32)
    sum_sq, plane = np.zeros(nh, D), np.full((nh, 4), np.nan)
    dist = F(cfg["dist"])
    solve_cfg = {k: cfg[k] for k in ("min_edge", "min_sin", "axis", "min_cos")}
    for j, (a, b, c) in enumerate(tri.tolist()):
        if a == b or b == c or a == c:
            status[j] = DEGENERATE
            continue
        status[j], pl, nf = solve(p[[a, b, c]], **solve_cfg)
        if status[j] != OK:
            continue
        plane[j] = pl
        t = signed_t(p, nf, p[a])
        inside = np.abs(t) < dist
        inliers[j] = int(inside.sum())
        sum_sq[j] = sum_shape(np.where(inside, t.astype(D) * t.astype(D), 0.0)) if N else 0.0
    return dict(status=status, inliers=inliers, sum_sq=sum_sq, plane=plane)


def side_mask(t, dist, side):
    dist = F(dist)
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        return (np.abs(t) < dist) if side == 0 else ((t < dist) if side < 0 else (t > -dist))


def mask_restate(pts, normal, anchor, dist, side=0, first=0, n=None):
    p = np.asarray(pts, F).reshape(-1, 3)
    n = len(p) - first if n is None else n
    return side_mask(signed_t(p[first:first + n], normal, anchor), dist, side)


def rank(out):
    """The OK hypotheses by inliers descending, sum_sq ascending, index ascending (api.plane_consensus' order)."""
    ok = np.nonzero(out["status"] == OK)[0]
    return ok[np.lexsort((ok, out["sum_sq"][ok], -out["inliers"][ok].astype(np.int64)))]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, D)).view(np.uint64)


def same(got, want, what=""):
    """status, inliers with no tolerance; sum_sq and plane bit for bit (every NaN is the same NaN to this test)."""
    np.testing.assert_array_equal(got["status"], want["status"], err_msg="%s status" % what)
    np.testing.assert_array_equal(got["inliers"], want["inliers"], err_msg="%s inliers" % what)
    np.testing.assert_array_equal(bits(got["sum_sq"]), bits(want["sum_sq"]), err_msg="%s sum_sq" % what)
    if "plane" in got and "plane" in want:
        g, w = np.asarray(got["plane"], D), np.asarray(want["plane"], D)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg="%s plane NaN" % what)
        np.testing.assert_array_equal(bits(np.nan_to_num(g, nan=0.0)), bits(np.nan_to_num(w, nan=0.0)), err_msg="%s plane" % what)
        assert np.all(np.isnan(g[got["status"] != OK])), what


def same_bits(a, b, what=""):
    """Two outputs of the library against each other: every byte."""
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def up(x):
    return F(np.nextafter(F(x), F(np.inf)))


def down(x):
    return F(np.nextafter(F(x), F(-np.inf)))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def scene():
    """The clusters' scene (tests/clusters_common.py): a floor of 1 600 points at z = 0, a wall, a cylinder and forty blobs."""
    import clusters_common as cc
    return cc.scene()


def nearest(pts, xyz):
    """The index of the stored point nearest to xyz."""
    d = np.asarray(pts, D) - np.asarray(xyz, D)
    return int(np.argmin((d * d).sum(1)))


def hand_triplets(pts):
    """Hand-made hypotheses on the standard scene with the status each must get under REC_CFG (min_edge 0.3, min_sin 0.2, the z
    axis at min_cos 0.95): [(name, (a, b, c), status)].  The floor is z = 0 over [0, 3.9]^2, the wall x = 0 above it."""
    f = lambda x, y: nearest(pts, (x, y, 0.0))
    w = lambda y, z: nearest(pts, (0.0, y, z))
    return [("floor", (f(0.5, 0.5), f(3.5, 0.7), f(1.8, 3.5)), OK),
            ("floor, b and c swapped", (f(0.5, 0.5), f(1.8, 3.5), f(3.5, 0.7)), OK),
            ("a repeated index", (f(0.5, 0.5), f(3.5, 0.7), f(0.5, 0.5)), DEGENERATE),
            ("one index three times", (f(1.0, 1.0),) * 3, DEGENERATE),
            ("collinear along y = 2", (f(0.5, 2.0), f(2.0, 2.0), f(3.5, 2.0)), DEGENERATE),
            ("a short edge", (f(1.0, 1.0), f(1.1, 1.0), f(2.5, 3.0)), DEGENERATE),
            ("on the wall, under the z-axis constraint", (w(0.5, 0.6), w(3.5, 0.8), w(2.0, 3.6)), REJECTED)]


def random_triplets(n, nh, seed):
    """[nh, 3] int32 indices below n, repeats allowed now and then (a repeated index is DEGENERATE)."""
    return np.random.RandomState(seed).randint(0, n, (nh, 3)).astype(np.int32)


def cloud(n, seed=0, span=4.0):
    """n points: a noisy plane z = 0.2 x (two thirds) and scattered points, in a seeded random order."""
    rs = np.random.RandomState(1000 + 7 * seed + n)
    m = (2 * n) // 3
    xy = rs.uniform(0, span, (m, 2))
    a = np.column_stack([xy, 0.2 * xy[:, 0] + rs.normal(0, 0.01, m)])
    b = rs.uniform(0, span, (n - m, 3))
    pts = np.concatenate([a, b])[rs.permutation(n)].astype(F)
    pts.setflags(write=False)
    return pts


STEP = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def lattice_layers():
    """A map whose coordinates are multiples of 2^-10: a 24 x 24 layer at z = 0 (spacing 1/8), and 24 x 24 layers at heights
    +-dist, +-(dist - 2^-10) ... for dist = 64 * 2^-10.  With the normal (0, 0, 1) from a sample of the z = 0 layer t IS z, exactly.
    Returns (points, z of each point in lattice steps)."""
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 2) * 0.125
    layers = [0, 64, -64, 63, -63, 65, -65, 1, -1, 640]
    pts = np.concatenate([np.column_stack([g + 0.001953125 * k, np.full(len(g), z * STEP)]) for k, z in enumerate(layers)])
    zs = np.repeat(layers, len(g))
    order = np.random.RandomState(5).permutation(len(pts))
    lead = np.array([0, 23, 24 * 23])                                  # three corners of layer 0 lead: the sample (0, 1, 2)
    order = np.concatenate([lead, order[~np.isin(order, lead)]])
    pts, zs = pts[order].astype(F), zs[order]
    assert np.all(pts.astype(D) / STEP == np.round(pts.astype(D) / STEP))
    pts.setflags(write=False)
    return pts, zs
