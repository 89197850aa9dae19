"""Fixtures for the map's insert rule at its thresholds (plain numpy, deterministic, no GPU), shared by the host twin's test
(test_insert_rule_host.py) and the device's (test_gpu_insert_rule.py).

The rule (reference Objects/Octree.hpp:282-432; fast_limo_amd/csrc/hip/flimo_gbook.hip, flimo_insert.cpp), with bucket 32:
  * the first batch is stored completely; the root cube comes from its bounding box;
  * a later batch is routed down to leaves and missing children.  A group of g points that meets a leaf of n points and half edge h:
      n + g > 32 and h > 2 min_extent      -> the leaf is rebuilt (split while > 32 points and h > 2 min_extent), all stored
      else, down-sampling on, h <= 2 min_extent and n > 4   -> the whole group is dropped
      else                                 -> appended
    and a group that meets a missing child is stored completely (a subtree is created);
  * octant of a point: bit a set when p[a] > centre[a] -- a point ON a centre plane goes to the low side;
  * the root doubles towards the batch's max corner, then its min corner, until |corner - centre| <= half on every axis.

Every case pins its root to a dyadic cube with its first batch (points on the cube's extreme coordinates), so that node centres and
half edges are exact and one can say by hand which leaf a point falls in.  With min_extent s and the root [-8s, 8s]^3:
  root             centre 0,            half 8s   (splits: the first batch holds more than 32 points)
  L = child 7      centre (4s, 4s, 4s), half 4s   (4s > 2s: splittable)           = (0, 8s]^3
  M = child 7 of L centre (6s, 6s, 6s), half 2s   (2s > 2s is false: minimal)     = (4s, 8s]^3

A case is a dict: name, batches (list of float32 [n, 3]), min_extent, focus (points around which the k-NN queries are placed),
and where the stored count was worked out by hand, stored = {downsample: count after the last batch}.
"""
from collections import Counter

import numpy as np

F = np.float32
NAN3 = np.full((1, 3), np.nan, F)


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------
def _rows_view(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.dtype((np.void, 12))).reshape(-1)


def _stored_of_batch(batch, pts_before, pts_after):
    """The batch's stored points in insertion (= batch) order: the multiset difference of the octree's points after and before it
    (the octree never drops a stored point), picked out of the batch in its order."""
    need = Counter(_rows_view(pts_after).tolist())
    need.subtract(Counter(_rows_view(pts_before).tolist()))
    assert min(need.values(), default=0) >= 0
    out = []
    for i, key in enumerate(_rows_view(batch).tolist()):
        if need.get(key, 0) > 0:
            need[key] -= 1
            out.append(i)
    assert sum(need.values()) == 0
    return batch[np.array(out, np.int64)] if out else np.zeros((0, 3), np.float32)


def finite_rows(b):
    return b[np.all(np.isfinite(b), axis=1)]


class OracleMap:
    """The oracle octree fed batch by batch, with this project's two statements where the reference has no answer:
      * a batch without a finite point changes nothing (the reference would double its root to infinity);
      * the zero-size root: when every stored point lies at one location and the batch leaves it, the map becomes
        Octree().update(stored points followed by the batch's finite points); later batches go into that octree.  The oracle's
        update is never called with the two-batch sequence itself: it would not return.
    `expect` is the map in insertion order, built from oracle octrees only."""

    def __init__(self, oracle, min_extent, downsample):
        self._new = lambda: oracle.Octree(min_extent, downsample)
        self.oc = self._new()
        self.expect = np.zeros((0, 3), F)
        self.reinits = 0

    def update(self, b):
        fin = finite_rows(b)
        if len(fin) == 0:
            return
        e = self.expect
        if len(e) and np.all(e == e[0]) and not np.all(fin == e[0]):
            both = np.concatenate([e, fin])
            self.oc = self._new()
            self.oc.update(both)
            assert self.oc.size() == len(both)                       # initialize drops nothing
            self.expect = both
            self.reinits += 1
            return
        before = self.oc.points() if self.oc.size() else np.zeros((0, 3), F)
        self.oc.update(b)
        self.expect = np.concatenate([e, _stored_of_batch(b, before, self.oc.points())])
        assert len(self.expect) == self.oc.size()


def queries_of(case, n_per=24, seed=5):
    """A few hundred queries at the case's own edges: the focus points themselves, the same moved by a fraction of min_extent, by
    a few min_extent, and by a sixteenth of the map's size."""
    rng = np.random.default_rng(seed)
    f = np.asarray(case["focus"], np.float64).reshape(-1, 3)
    s = float(case["min_extent"])
    allp = np.concatenate([finite_rows(b) for b in case["batches"]]).astype(np.float64)
    span = float(np.max(allp.max(0) - allp.min(0))) if len(allp) else 1.0
    out = [f]
    for scale in (0.3 * s, 4 * s, span / 16):
        out.append((f[:, None, :] + rng.uniform(-1, 1, (len(f), n_per, 3)) * scale).reshape(-1, 3))
    return np.concatenate(out).astype(F)


def cell_size_of(case):
    """The index's cell for a case (flimo_map_config's cell_size; 0 = its default of 0.5 m).  The index is a grid over the map's
    box and its tables grow with the box's cross-section in cells; the cases that pin a root of kilometres -- thousands of them in
    the deep chains -- take a cell of 1/128 to 1/64 of their extent, a power of two.  The search stays exact whatever the cell;
    what is stored does not depend on it."""
    allp = np.concatenate([finite_rows(b) for b in case["batches"]]).astype(np.float64)
    span = float(np.max(allp.max(0) - allp.min(0)))
    return 0.0 if span <= 256.0 else float(2.0 ** np.ceil(np.log2(span / 128.0)))


# ---- building blocks --------------------------------------------------------------------------------------------------------------
def cube_pts(rng, lo, hi, n):
    """n points of the half-open cube (lo, hi]: lo + j (hi - lo) / 64 with j in 1..64 on each axis -- exact in float32 for the
    dyadic cubes used here, never on the cube's low faces."""
    lo, hi = np.asarray(lo, np.float64) * np.ones(3), np.asarray(hi, np.float64) * np.ones(3)
    j = rng.integers(1, 65, (n, 3))
    p = lo + j * ((hi - lo) / 64.0)
    assert np.all(p.astype(F).astype(np.float64) == p)
    return p.astype(F)


def octant_cube(c, h, k):
    """Child k of the cube (centre c, half h) as (lo, hi]."""
    c = np.asarray(c, np.float64) * np.ones(3)
    bits = np.array([(k >> a) & 1 for a in range(3)])
    return c + np.where(bits, 0.0, -h), c + np.where(bits, h, 0.0)


def corners(h):
    return np.array([[-h, -h, -h], [h, h, h]], F)


def scaffold(rng, s, per=7):
    """The two corners of [-8s, 8s]^3 and `per` points in each of the root's octants 1..6: with anything more than 32 points in the
    first batch the root splits; octant 0 holds the low corner, octant 7 (= L) the high one and whatever the case puts there."""
    parts = [corners(8 * s)]
    for k in range(1, 7):
        parts.append(cube_pts(rng, *octant_cube(0.0, 8 * s, k), per))
    return np.concatenate(parts)


def probe_of_L(rng, s, per=6):
    """`per` points in each of L's eight children."""
    return np.concatenate([cube_pts(rng, *octant_cube(4 * s, 4 * s, k), per) for k in range(8)])


def dense_over(rng, lo, hi, n):
    lo, hi = np.asarray(lo, np.float64) * np.ones(3), np.asarray(hi, np.float64) * np.ones(3)
    return (lo + rng.integers(0, 1025, (n, 3)) * ((hi - lo) / 1024.0)).astype(F)


def _case(name, batches, s, focus, stored=None):
    batches = [np.ascontiguousarray(b, F).reshape(-1, 3) for b in batches]
    assert all(len(b) <= 25000 for b in batches), name
    return dict(name=name, batches=batches, min_extent=float(s), focus=np.asarray(focus, F).reshape(-1, 3), stored=stored)


# ---- 1. leaf counts, splittable leaf ----------------------------------------------------------------------------------------------
def leaf_count_splittable_cases(s=0.25):
    """L holds n points (the high corner and n - 1 more), all in M's cube; a group of g arrives, also in M's cube.  n + g = 32 appends,
    33 splits -- both keep the group.  The difference shows with the probe (6 points into each child of L):
      split:   L has the one child M, a minimal leaf of 33 points.  The probe's 6 points for M are dropped with down-sampling on
               (33 > 4), the other 42 create seven children.
      append:  L holds 32 points; 32 + 48 > 32, L is rebuilt and the probe stored completely."""
    out = []
    for n, g in ((31, 1), (31, 2), (1, 31), (1, 32), (32, 1)):
        rng = np.random.default_rng(100 + 40 * n + g)
        m_lo, m_hi = octant_cube(4 * s, 4 * s, 7)
        first = np.concatenate([scaffold(rng, s), cube_pts(rng, m_lo, m_hi, n - 1)])
        group = cube_pts(rng, m_lo, m_hi, g)
        probe = probe_of_L(rng, s)
        n1 = 2 + 6 * 7 + (n - 1)
        split = n + g > 32
        stored = {True: n1 + g + (42 if split else 48), False: n1 + g + 48}
        out.append(_case("leaf_splittable_%d+%d" % (n, g), [first, group, probe], s, [[6 * s] * 3, [4 * s] * 3, [8 * s] * 3, [0.0] * 3], stored))
    return out


# ---- 2. leaf counts, minimal leaf -------------------------------------------------------------------------------------------------
def _minimal_leaf_first(rng, s, k):
    """First batch that leaves M a minimal leaf of k points (the high corner and k - 1 more): L gets 6 points in each of its children
    0, 1, 2, 4, 5, 6 (child 3 stays missing) and with them more than 32 points, so it splits."""
    parts = [scaffold(rng, s)]
    for c in (0, 1, 2, 4, 5, 6):
        parts.append(cube_pts(rng, *octant_cube(4 * s, 4 * s, c), 6))
    parts.append(cube_pts(rng, *octant_cube(4 * s, 4 * s, 7), k - 1))
    return np.concatenate(parts), 2 + 42 + 36 + (k - 1)


def leaf_count_minimal_cases():
    out = []
    for s in (0.25, 0.125):
        m_lo, m_hi = octant_cube(4 * s, 4 * s, 7)
        focus = [[6 * s] * 3, [4 * s] * 3, [8 * s] * 3]
        for k in (4, 5):
            rng = np.random.default_rng(int(1000 * s) + k)
            first, n1 = _minimal_leaf_first(rng, s, k)
            group = cube_pts(rng, m_lo, m_hi, 40)
            # M's half edge is 2s == 2 min_extent: not splittable, so 4 + 40 and 5 + 40 both stay one leaf; 4 > 4 is false (append),
            # 5 > 4 drops the group when down-sampling is on
            stored = {True: n1 + (40 if k == 4 else 0), False: n1 + 40}
            out.append(_case("leaf_minimal_%d+40_s%g" % (k, s), [first, group], s, focus, stored))
        rng = np.random.default_rng(int(1000 * s) + 77)
        first, n1 = _minimal_leaf_first(rng, s, 5)
        grow = [cube_pts(rng, m_lo, m_hi, g) for g in (40, 100, 200)]
        out.append(_case("leaf_minimal_grows_s%g" % s, [first] + grow, s, focus, {True: n1, False: n1 + 340}))
        rng = np.random.default_rng(int(1000 * s) + 78)
        first, n1 = _minimal_leaf_first(rng, s, 4)
        dup = np.repeat(cube_pts(rng, m_lo, m_hi, 1), 40, axis=0)
        one = cube_pts(rng, m_lo, m_hi, 1)
        # the 40 copies are one group into a leaf of 4: appended.  The single point after them meets a leaf of 44.
        out.append(_case("leaf_minimal_40_duplicates_s%g" % s, [first, dup, one], s, focus, {True: n1 + 40, False: n1 + 41}))
    return out


# ---- 3. points on centre planes ---------------------------------------------------------------------------------------------------
def centre_plane_cases():
    """Dyadic lattices: with min_extent s the root is [-16s, 16s]^3 and the lattice has spacing 2s, so its points lie on the centre
    planes of nodes at every level down to the minimal leaves (half 2s, centres at odd multiples of 2s)."""
    out = []
    for s in (0.25, 0.125):
        g = np.arange(-8, 9) * (2 * s)
        lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
        batches = [lat, lat[::3], lat + F(s), lat[::-1]]
        out.append(_case("centre_planes_s%g" % s, batches, s, [[0.0] * 3, [16 * s] * 3, [-16 * s] * 3, [2 * s, 0.0, -4 * s], [s] * 3]))
    return out


# ---- 4. the whole-block build (kBigItem = 2048) -----------------------------------------------------------------------------------
def big_item_cases(s=0.25):
    out = []
    H = 8 * s
    foc = [[0.0] * 3, [H] * 3, [-H] * 3, [4 * s, 4 * s, -4 * s]]
    for n in (2047, 2048, 2049):                                  # init's n_big: the first batch's finite points
        rng = np.random.default_rng(4000 + n)
        first = np.concatenate([corners(H), dense_over(rng, -H, H, n - 2), NAN3, NAN3])
        rng.shuffle(first)
        out.append(_case("big_first_batch_%d" % n, [first, finite_rows(first)[::2] + F(s / 8), dense_over(rng, -H, H, 3000)], s, foc))
    c3_lo, c3_hi = octant_cube(0.0, H, 3)                         # the root's child 3: x > 0, y > 0, z <= 0
    base_no3 = lambda rng: np.concatenate([corners(H)] + [cube_pts(rng, *octant_cube(0.0, H, k), 8) for k in (1, 2, 4, 5, 6)])
    for n in (2047, 2048, 2049):                                  # a CREATE group into one missing child
        rng = np.random.default_rng(4100 + n)
        grp = dense_over(rng, c3_lo + s / 16, c3_hi, n)
        out.append(_case("big_create_%d" % n, [base_no3(rng), grp, grp[::-1] + F(s / 8)], s, foc))
    for tot in (2048, 2049):                                      # a SPLIT with cnt + g on either side
        rng = np.random.default_rng(4200 + tot)
        first = np.concatenate([scaffold(rng, s), cube_pts(rng, 0.0, H, 19)])          # L: the corner + 19 = 20 points
        grp = dense_over(rng, s / 16, H, tot - 20)
        out.append(_case("big_split_%d" % tot, [first, grp, grp[::2] + F(s / 8)], s, foc))
    for n in (2048, 2049):                                        # a big item one of whose children receives exactly n
        rng = np.random.default_rng(4300 + n)
        sub_lo, sub_hi = octant_cube((c3_lo + c3_hi) / 2, 4 * s, 0)
        grp = np.concatenate([dense_over(rng, sub_lo + s / 16, sub_hi, n)] +
                             [cube_pts(rng, *octant_cube((c3_lo + c3_hi) / 2, 4 * s, k), 40) for k in range(1, 8)])
        rng.shuffle(grp)
        out.append(_case("big_child_of_%d" % n, [base_no3(rng), grp, grp[::-1] + F(s / 8)], s, foc))
    rng = np.random.default_rng(4400)                             # three big items in one batch
    first = np.concatenate([corners(H)] + [cube_pts(rng, *octant_cube(0.0, H, k), 12) for k in (1, 2, 4)])       # 38 points: the root splits
    grp = np.concatenate([dense_over(rng, octant_cube(0.0, H, k)[0] + s / 16, octant_cube(0.0, H, k)[1], 2100 + 50 * k) for k in (3, 5, 6)])
    rng.shuffle(grp)
    out.append(_case("big_three_items", [first, grp, grp[::3] + F(s / 8)], s, foc))
    rng = np.random.default_rng(4500)                             # 20 000 points spread thin around a dense core
    s2 = 0.0625
    core = np.clip(np.round(rng.normal(0, 1.0, (20000, 3)) * 512) / 512, -7.9, 7.9)
    first = np.concatenate([corners(8.0), core.astype(F)])
    out.append(_case("big_first_batch_thin_20000", [first, first[::2] + F(s2 / 2), dense_over(rng, -8, 8, 5000)], s2,
                     [[0.0] * 3, [8.0] * 3, [-8.0] * 3, [1.0, -1.0, 0.5]]))
    return out


# ---- 5. root growth ---------------------------------------------------------------------------------------------------------------
def root_growth_cases(s=0.25):
    out = []
    H = 8 * s

    def base(rng):
        return np.concatenate([corners(H), dense_over(rng, -H, H, 60)])

    def add(name, far, seed):
        rng = np.random.default_rng(seed)
        far = np.asarray(far, F).reshape(-1, 3)
        dense = dense_over(rng, -H, H, 1500)
        out.append(_case(name, [base(rng), far, dense, dense[::2] + F(s / 8)], s, np.concatenate([far, corners(H), [[0.0] * 3]])))

    add("root_on_a_face", [[H, 0.5 * s, -3 * s], [s, -H, 2 * s]], 5000)               # mm == root_half: the root stays
    up = np.nextafter(F(H), F(np.inf))
    add("root_one_ulp_beyond", [[up, 0.5 * s, -3 * s]], 5001)
    add("root_one_ulp_beyond_low", [[s, -up, 2 * s]], 5002)
    add("root_both_sides_in_one_batch", [[20.0, 1.0, 1.0], [-50.0, -3.0, 2.0]], 5003)
    for k in range(8):
        sign = np.array([1.0 if (k >> a) & 1 else -1.0 for a in range(3)])
        add("root_direction_%d" % k, [sign * np.array([20.0, 9.0, 13.0])], 5010 + k)
    add("root_to_2e6_m", [[2.0e6, -3.0, 1.0e3]], 5020)
    return out


# ---- 6. deep trees ----------------------------------------------------------------------------------------------------------------
def _deep_points(depth, s, crowded):
    """The nested corner.  Root [-R, R]^3 with R = 2^e chosen so that exactly `depth` cubes in a row are splittable: halves R,
    R/2, ..., R 2^-(depth-1) are > 2 min_extent and R 2^-depth is not.  At level l the crowded child is octant 7 (towards the corner
    (R, R, R)); each of the seven other children gets one point, at its centre.  The bottom holds 33 points on the last two float32
    values below and at R.  Centres are R (1 - 2^-l): exact in float32 for l <= 24.  crowded == 0 is the mirror image."""
    assert depth <= 24
    two_min = float(F(2) * F(s))
    e = next(e for e in range(-40, 60) if 2.0 ** (e - depth + 1) > two_min >= 2.0 ** (e - depth))
    R = 2.0 ** e
    assert R * 2.0 ** -(depth - 1) > two_min >= R * 2.0 ** -depth, (depth, s, R)
    pts = []
    for l in range(depth):
        c, h = R * (1 - 2.0 ** -l), R * 2.0 ** -l
        for k in range(7):
            pts.append([c + (0.5 if (k >> a) & 1 else -0.5) * h for a in range(3)])
    lo = float(np.nextafter(F(R), F(0)))
    rng = np.random.default_rng(depth)
    bottom = np.where(rng.integers(0, 2, (33, 3)) > 0, R, lo)
    p = np.concatenate([np.array(pts), bottom])
    assert np.all(p.astype(F).astype(np.float64) == p)
    p = p.astype(F)
    pin = np.array([[R, -R, -R], [-R, R, -R], [-R, -R, R], [-R, -R, -R]], F)     # the box [-R, R]^3 without a point in octant 7
    if crowded == 0:
        p, pin = -p, -pin
    return p, pin, R


def deep_tree_cases(depths=(17, 18, 19, 24), extents=(0.2, 0.01)):
    out = []
    for s in extents:
        for depth in depths:
            for crowded in (7, 0):
                p, pin, R = _deep_points(depth, s, crowded)
                sg = 1.0 if crowded == 7 else -1.0
                focus = np.array([[sg * R] * 3, [-sg * R] * 3, [sg * R * (1 - 2.0 ** -(depth - 1))] * 3, [0.0] * 3])
                tag = "d%d_s%g_oct%d" % (depth, s, crowded)
                far = np.array([[sg * R] * 3, [-sg * R] * 3], F)
                # the first batch: Octree::initialize
                out.append(_case("deep_init_" + tag, [np.concatenate([far, p]), p[::-1].copy()], s, focus))
                # the second batch into a map of ten points (the root is a leaf): update's SPLIT
                rng = np.random.default_rng(depth)
                ten = np.concatenate([far, dense_over(rng, -R / 2, R / 2, 8)])
                out.append(_case("deep_split_" + tag, [ten, p, p[::-1].copy()], s, focus))
                # ... and into a map whose root has split and has no child where the chain goes: update's CREATE
                forty = np.concatenate([pin] + [cube_pts(rng, *octant_cube(0.0, R, k if crowded == 7 else 7 - k), 6) for k in range(7)])
                out.append(_case("deep_create_" + tag, [forty, p, p[::-1].copy()], s, focus))
    return out


def too_deep_case():
    """A root more than 48 halvings above 2 min_extent (flimo_gbook.h GB_MAX_DEPTH): min_extent 2^-20, root half 2^30 -> 49."""
    s = 2.0 ** -20
    ok = np.concatenate([corners(8.0), dense_over(np.random.default_rng(9), -8, 8, 200)])
    return dict(min_extent=s, ok=ok, too_deep=np.array([[2.0 ** 30, 1.0, 1.0], [-(2.0 ** 30), 0.0, 2.0]], F),
                first_too_deep=corners(2.0 ** 30))


# ---- 7. zero-size roots -----------------------------------------------------------------------------------------------------------
def zero_root_cases(s=0.25):
    out = []
    P = np.array([[1.5, -0.75, 0.25]], F)
    foc = [P[0], [3.0, 3.0, 3.0], [0.0] * 3]

    def tail(rng):
        return [cube_pts(rng, 2.0, 4.0, 50), dense_over(rng, -4, 4, 3000), dense_over(rng, -4, 4, 3000)[::2] + F(s / 8)]

    rng = np.random.default_rng(7000)
    out.append(_case("zero_root_one_point", [P] + tail(rng), s, foc))
    out.append(_case("zero_root_40_copies", [np.repeat(P, 40, axis=0)] + tail(rng), s, foc))
    out.append(_case("zero_root_one_finite_among_nans", [np.concatenate([NAN3, NAN3, P, NAN3])] + tail(rng), s, foc))
    out.append(_case("zero_root_second_copy_first", [P, P] + tail(rng), s, foc))
    out.append(_case("zero_root_copies_until_dropped", [P, np.repeat(P, 5, axis=0), P, np.repeat(P, 3, axis=0)] + tail(rng), s, foc))
    out.append(_case("zero_root_batch_of_one_elsewhere", [P, P + F(1.0)] + tail(rng), s, foc))
    # tiny but not zero: the root doubles about 100 times; the reference ends here, the oracle is the yardstick
    tiny = np.array([[0.0, 0.0, 0.0], [1e-30, 0.0, 0.0]], F)
    out.append(_case("tiny_root_1e-30", [tiny, np.array([[1.0, 0.0, 0.0]], F)] + tail(rng), s, [[0.0] * 3, [1.0, 0.0, 0.0], [3.0] * 3]))
    return out


# ---- 8. non-finite points and tiny batches ----------------------------------------------------------------------------------------
def nan_and_tiny_cases(s=0.25):
    rng = np.random.default_rng(8000)
    first, _ = _minimal_leaf_first(rng, s, 5)
    m_lo, m_hi = octant_cube(4 * s, 4 * s, 7)
    mostly_nan = np.full((40, 3), np.nan, F)
    mostly_nan[::9] = cube_pts(rng, -8 * s, 8 * s, 5)
    one_nan_coord = cube_pts(rng, -8 * s, 8 * s, 6)
    one_nan_coord[1, 2] = np.nan
    one_nan_coord[4, 0] = np.nan
    batches = [np.repeat(NAN3, 7, axis=0),                             # before the first batch: still no map
               first,
               np.repeat(NAN3, 33, axis=0),                            # only NaNs
               mostly_nan, one_nan_coord,
               cube_pts(rng, *octant_cube(0.0, 8 * s, 1), 1),          # one point into a splittable leaf (the root's child 1, 7 points)
               cube_pts(rng, m_lo, m_hi, 1),                           # ... into a minimal leaf of 5
               cube_pts(rng, *octant_cube(4 * s, 4 * s, 3), 1),        # ... into L's missing child 3
               np.array([[100.0, 1.0, 1.0]], F),                       # ... outside the root
               NAN3,
               dense_over(rng, -8 * s, 8 * s, 2000)]
    return [_case("nan_and_one_point_batches", batches, s, [[6 * s] * 3, [100.0, 1.0, 1.0], [0.0] * 3, [-8 * s] * 3])]


def groups():
    """{group name: cases}, in the order of the sections above."""
    deep = deep_tree_cases()
    g = {
        "leaf_splittable": leaf_count_splittable_cases(),
        "leaf_minimal": leaf_count_minimal_cases(),
        "centre_planes": centre_plane_cases(),
        "big_items": big_item_cases(),
        "root_growth": root_growth_cases(),
        "zero_root": zero_root_cases(),
        "nan_and_tiny": nan_and_tiny_cases(),
    }
    for s in (0.2, 0.01):
        for depth in (17, 18, 19, 24):
            g["deep_d%d_s%g" % (depth, s)] = [c for c in deep if ("_d%d_s%g_" % (depth, s)) in c["name"]]
    return g
