"""GPU suite: map carving -- flimo_map_seen_through marks the stored points the resident scan looks through from the sensor,
flimo_map_carve forgets them (and, with a box, what lies outside it) in the crop's one ordered pass, Localizer::set_map_carving
applies it every n-th inserted sweep.  The yardstick is the definition restated in numpy (tests/carve_common.py), fed the scan's
world points as flimo_scan_to_world downloads them and the map as flimo_map_points does: every comparison below is exact.  After a
carve the map is the reference octree's clear() + initialize(kept), as after a crop (tests/test_gpu_local_map.py), so that part is
checked against a twin context and the oracle's octree."""
import ctypes as C

import numpy as np
import pytest

import carve_common as cc
from common import CAPS, sort_rows
from fast_limo_amd import synth
from scan_fitness_common import x26_of

pytestmark = pytest.mark.gpu

ERR_INVALID = -2
INF = float("inf")
F = np.float32
CROP_TILE = 256 * 32                       # flimo_map.hip: points per tile of the ordered compaction


def _ident(t):
    x = np.zeros(26); x[0:3] = t; x[6] = 1; x[10] = 1
    return x


def _ctx(batches, scan, downsample=True, cell=0.0):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, downsample, cell)
    for k, b in enumerate(batches):
        ctx.map_add(b, stamp=0.5 + k)
    ctx.scan_set(scan)
    return ctx


def _expect(ctx, x26, sensor, **cfg):
    """The yardstick's mask over the context's map, from the context's own world points."""
    return cc.yardstick(ctx.scan_to_world(x26), ctx.map_points(), sensor, **cfg)


def _check(ctx, what=""):
    mm, merges, builds = ctx.grid_selfcheck()
    assert mm == 0, (what, mm, merges, builds)
    return merges, builds


def _inside(pts, lo, hi):
    return np.all((pts >= F(lo)) & (pts <= F(hi)), axis=1)


def _rows(a):
    return np.ascontiguousarray(a, dtype=F).view(np.dtype((np.void, 12))).reshape(-1)


def _knn_indices_address(ctx_pts, q, idx, sqd, cnt):
    """|q - pts[idx]|^2 reproduces sqd.  Recomputed in float64 from the float32 inputs; the device's float32 value differs from that
    by the roundings of one subtraction, one square and two additions per term: a few 2^-24 relative, 2e-6 with room."""
    for k in range(idx.shape[1]):
        ok = cnt > k
        assert np.all(idx[ok, k] >= 0) and np.all(idx[ok, k] < len(ctx_pts))
        d = (q[ok].astype(np.float64) - ctx_pts[idx[ok, k]].astype(np.float64))
        np.testing.assert_allclose((d * d).sum(1), sqd[ok, k].astype(np.float64), rtol=2e-6, atol=1e-12)


def _same_neighbours(idx_a, idx_b, sqd, what):
    """flimo_knn's neighbour indices of two contexts that hold the same points: equal element for element where a row's distances
    are pairwise different, equal as sets within each group of exactly tied distances (their order follows the cell-sorted array's
    history, as tests/test_gpu_local_map.py explains)."""
    diff = np.where(np.any(idx_a != idx_b, axis=1))[0]
    for r in diff:
        assert len(np.unique(sqd[r])) < sqd.shape[1], (what, r, sqd[r], idx_a[r], idx_b[r])
        oa, ob = np.lexsort((idx_a[r], sqd[r])), np.lexsort((idx_b[r], sqd[r]))
        np.testing.assert_array_equal(idx_a[r][oa], idx_b[r][ob], err_msg="%s row %d" % (what, r))
    assert len(diff) <= 0.01 * len(idx_a), (what, len(diff))


@pytest.fixture(scope="module")
def std():
    static, ghost, scan, x26, sensor = cc.standard_scene()
    return dict(static=static, ghost=ghost, scan=scan, x26=x26, sensor=sensor)


CFGS = [dict(res=8, win=0, margin=0.0, rel_margin=0.0), dict(res=8, win=3, margin=0.2, rel_margin=0.02),
        dict(res=64, win=0, margin=0.0, rel_margin=0.0), dict(res=64, win=1, margin=0.2, rel_margin=0.02),
        dict(res=64, win=3, margin=0.05, rel_margin=0.0, max_depth=6.0), dict(res=1024, win=0, margin=0.2, rel_margin=0.02),
        dict(res=1024, win=1, margin=0.0, rel_margin=0.0), dict(res=1024, win=3, margin=1.0, rel_margin=0.1, max_depth=9.5),
        dict(res=300, win=2, margin=0.0, rel_margin=0.05)]


# ---- 1. mask and count against the yardstick ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 300.0])
def test_mask_and_count_equal_the_yardstick(built, std, shift):
    """The standard scene (at the origin, and 300 m from it: coarser float32 coordinates), NaN points in the scan."""
    off = F([shift, -shift, 0.0])
    t = np.float64(synth.T_STAR_T) + off.astype(np.float64)
    x26, sensor = x26_of(tuple(t)), F(t)
    scan = std["scan"].copy()
    scan[::97] = np.nan
    scan[5, 1] = np.nan
    scan[6] = [np.inf, 0.0, 0.0]
    ctx = _ctx([std["static"] + off, std["ghost"] + off], scan)
    try:
        pts = ctx.map_points().copy()
        world = ctx.scan_to_world(x26)
        assert np.isnan(world).any()
        idx0 = ctx.knn(pts[:64], 5)
        for cfg in CFGS:
            want = cc.yardstick(world, pts, sensor, **cfg)
            mask, count = ctx.map_seen_through(x26, sensor, **cfg)
            print("shift %g, %s: %d of %d seen through" % (shift, cfg, want.sum(), len(pts)))
            np.testing.assert_array_equal(mask, want, err_msg=str(cfg))
            assert count == want.sum(), cfg
            assert ctx.map_seen_through(x26, sensor, want_mask=False, **cfg) == (None, count)
        assert any(cc.yardstick(world, pts, sensor, **cfg).sum() > 100 for cfg in CFGS)
        # nothing changed
        np.testing.assert_array_equal(ctx.map_points(), pts)
        np.testing.assert_array_equal(ctx.scan_to_world(x26).view(np.uint32), world.view(np.uint32))
        for a, b in zip(ctx.knn(pts[:64], 5), idx0):
            np.testing.assert_array_equal(a, b)
        assert ctx.map_carve_stats() == dict(carves=0, points_removed=0)
        _check(ctx)
    finally:
        ctx.close()


def _hand_placed(s, far):
    """Stored points at offsets v from a sensor whose coordinates (and the sums) are exact in float32."""
    v = [(2, 2, 0.5), (2, -2, 0.5), (-2, 2, 0.5), (0.5, 2, 2), (0.5, -2, 2), (0.5, 2, -2),       # |vx| == |vy|, |vy| == |vz|
         (2, 2, 2), (-2, -2, -2), (2, -2, 2), (-1.5, 1.5, 1.5),                                   # all three equal
         (2, 0, 0), (2, 1, 0.5), (2, -1, -0.5), (2, 0.0625, -0.0625), (4, 1, 3), (-4, 0.125, 0),  # on pixel boundaries ((u + 1) * hr whole)
         (0, 3, 0), (0, -3, 0.75), (0.375, 0, -1.5), (0, 0, 1.5),
         (0, 0, 0),                                                                               # the sensor itself
         (2, 1.99, 0), (2, -1.99, 0.3), (2, 0.3, 1.97), (-3, 0.1, -2.99), (1.0, 3, -2.95),        # the strip at a face's edge
         (2.5, 0.3, -0.2), (3, -0.4, -0.3), (-2, 0.5, -0.1), (0.3, 4, -0.2), (1, 1.2, -0.9)]      # plain points in front of the walls
    if far:
        v += [(1.0e6, 0, 0), (-1.0e6, 3, -1)]                                                     # 1e6 m away
    v = np.array(v, F)
    pts = (v + s).astype(F)
    np.testing.assert_array_equal((pts - s)[:21], v[:21])                                         # (exact: the ties are ties on the device too)
    return pts


@pytest.mark.parametrize("far", [False, True])
def test_hand_placed_points_on_diagonals_pixel_boundaries_the_sensor_and_the_edge_strip(built, std, far):
    s = F([0.25, -0.5, 0.125])
    hand = _hand_placed(s, far)
    ctx = _ctx([np.concatenate([hand, std["static"]])], std["scan"], downsample=False)
    try:
        pts = ctx.map_points().copy()
        assert len(pts) == len(hand) + len(std["static"])
        np.testing.assert_array_equal(pts[:len(hand)], hand)
        x26 = std["x26"]
        world = ctx.scan_to_world(x26)
        seen = 0
        for cfg in CFGS:
            want = cc.yardstick(world, pts, s, **cfg)
            mask, count = ctx.map_seen_through(x26, s, **cfg)
            np.testing.assert_array_equal(mask, want, err_msg=str(cfg))
            assert count == want.sum()
            seen += want[:len(hand)].sum()
            assert not want[20]                                          # the sensor itself has no pixel
        assert seen > 0
        # the strip: with a window, the points whose pixel touches the face's border are kept
        ok, f, it, iu, m = cc.pixels(hand, s, 64)
        border = ok & ((it == 0) | (it == 63) | (iu == 0) | (iu == 63))
        assert border.sum() >= 5
        assert not cc.yardstick(world, hand, s, res=64, win=1, margin=0.0, rel_margin=0.0)[border].any()
    finally:
        ctx.close()


# ---- 2. invariance ------------------------------------------------------------------------------------------------------------------
def test_the_mask_does_not_depend_on_scan_order_cell_size_or_batching(built, std):
    cfg = cc.STD_CFG
    x26, sensor = std["x26"], std["sensor"]
    allpts = np.concatenate([std["static"], std["ghost"]])
    a = _ctx([allpts], std["scan"], downsample=False)
    b = _ctx([allpts], std["scan"], downsample=False, cell=1.3)
    c = _ctx(np.array_split(allpts, 10), std["scan"], downsample=False)
    try:
        ref, n_ref = a.map_seen_through(x26, sensor, **cfg)
        np.testing.assert_array_equal(ref, _expect(a, x26, sensor, **cfg))
        assert n_ref > 0.7 * cc.N_GHOST
        perm = np.random.default_rng(2).permutation(len(std["scan"]))
        a.scan_set(std["scan"][perm])
        m, n = a.map_seen_through(x26, sensor, **cfg)
        np.testing.assert_array_equal(m, ref); assert n == n_ref
        for other, what in ((b, "cell size"), (c, "ten batches")):
            np.testing.assert_array_equal(other.map_points(), allpts, err_msg=what)
            m, n = other.map_seen_through(x26, sensor, **cfg)
            np.testing.assert_array_equal(m, ref, err_msg=what); assert n == n_ref
    finally:
        a.close(); b.close(); c.close()


def test_the_sweeps_own_insert_does_not_change_the_mask(built, std):
    """Before and after flimo_map_add_scan of the same sweep: the points present in both get the same answer, and the sweep's own
    points are never seen through (margins >= 0) -- also with no margin at all."""
    x26, sensor = std["x26"], std["sensor"]
    ctx = _ctx([std["static"], std["ghost"]], std["scan"])
    try:
        for cfg in (cc.STD_CFG, dict(res=64, win=0, margin=0.0, rel_margin=0.0), dict(res=256, win=1, margin=0.0, rel_margin=0.0)):
            before, _ = ctx.map_seen_through(x26, sensor, **cfg)
            n0 = len(before)
            twin = _ctx([std["static"], std["ghost"]], std["scan"])
            try:
                twin.map_add_scan(x26, 9.0)
                after, _ = twin.map_seen_through(x26, sensor, **cfg)
                assert len(after) > n0 + 1000
                np.testing.assert_array_equal(after[:n0], before, err_msg=str(cfg))
                assert after[n0:].sum() == 0, cfg
                np.testing.assert_array_equal(after, _expect(twin, x26, sensor, **cfg))
            finally:
                twin.close()
    finally:
        ctx.close()


# ---- 3. flimo_map_carve equals the filter ---------------------------------------------------------------------------------------------
def test_carve_is_the_numpy_filter_in_insertion_order(built, std):
    cfg = cc.STD_CFG
    x26, sensor = std["x26"], std["sensor"]
    ctx = _ctx([std["static"], std["ghost"], synth.box_world_map(3000, 9.0, 8)], std["scan"])
    try:
        before = ctx.map_points().copy()
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        mask = _expect(ctx, x26, sensor, **cfg)
        assert mask.sum() > 100
        removed = ctx.map_carve(x26, sensor, **cfg)
        print("carve: %d -> %d points (%d removed)" % (len(before), len(before) - mask.sum(), removed))
        assert removed == mask.sum()
        assert ctx.map_size() == len(before) - mask.sum()
        after = ctx.map_points().copy()
        np.testing.assert_array_equal(after, before[~mask])            # same rows, same (insertion) order
        _check(ctx, "after the carve")
        assert ctx.map_carve_stats() == dict(carves=1, points_removed=removed)
        assert ctx.map_crop_stats() == dict(crops=0, points_removed=0)
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before
        # the same call again removes only what the new map's yardstick says (a window that held a nearer ghost may be free now)
        mask2 = _expect(ctx, x26, sensor, **cfg)
        removed2 = ctx.map_carve(x26, sensor, **cfg)
        assert removed2 == mask2.sum()
        np.testing.assert_array_equal(ctx.map_points(), after[~mask2])
        assert ctx.map_carve_stats() == dict(carves=1 + int(removed2 > 0), points_removed=removed + removed2)
        _check(ctx, "after the second carve")
    finally:
        ctx.close()


def test_carve_with_a_box_is_one_pass_for_crop_and_carve(built, std):
    cfg = cc.STD_CFG
    x26, sensor = std["x26"], std["sensor"]
    batches = [std["static"], std["ghost"]]
    ctx, twin = _ctx(batches, std["scan"]), _ctx(batches, std["scan"])
    try:
        before = ctx.map_points().copy()
        lo, hi = F([-9.0, -12.5, -3.0]), F([10.5, 8.0, 6.0])
        mask, ins = _expect(ctx, x26, sensor, **cfg), _inside(before, lo, hi)
        assert (mask & ins).sum() > 100 and (~ins).sum() > 500
        b0 = _check(ctx)[1]
        removed = ctx.map_carve(x26, sensor, box=(lo, hi), **cfg)
        keep = ~mask & ins
        assert removed == len(before) - keep.sum() > 0
        np.testing.assert_array_equal(ctx.map_points(), before[keep])
        assert _check(ctx, "carve with a box")[1] == b0 + 1             # ONE full layout
        assert ctx.map_carve_stats() == dict(carves=1, points_removed=removed)
        assert ctx.map_crop_stats() == dict(crops=0, points_removed=0)
        # a twin that crops, then carves, holds the same points
        twin.map_crop_box(lo, hi)
        twin.map_carve(x26, sensor, **cfg)
        np.testing.assert_array_equal(twin.map_points(), ctx.map_points())
        _check(twin, "crop, then carve")
    finally:
        ctx.close(); twin.close()


# ---- 4. afterwards the map is a fresh octree of the kept points -----------------------------------------------------------------------
def test_after_a_carve_the_map_is_a_fresh_octree_of_the_kept_points(built, oracle, std):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(11)
    cfg = cc.STD_CFG
    x26, sensor = std["x26"], std["sensor"]
    first = [std["static"], std["ghost"], std["static"][::2] + F(0.01), synth.box_world_map(5000, 14.0, 12) + F([2.5, -1, 0])]
    ctx, twin = _ctx(first, std["scan"]), _ctx(first, std["scan"])
    try:
        before = ctx.map_points().copy()
        kept = before[~_expect(ctx, x26, sensor, **cfg)]
        assert ctx.map_carve(x26, sensor, **cfg) == len(before) - len(kept) > 100
        twin.map_clear()                                               # what a caller without the call would do
        twin.map_add(kept)
        oc = oracle.Octree(0.2, True)
        oc.update(kept)
        assert oc.size() == len(kept)                                  # initialize drops nothing
        q = np.concatenate([rng.uniform(-14, 14, (1500, 3)).astype(F),
                            kept[rng.choice(len(kept), 500)] + rng.normal(0, 0.05, (500, 3)).astype(F),
                            std["ghost"][:200],                                                     # where forgotten points were
                            (rng.uniform(-50, 50, (100, 3)) + [-5000.0, 3000.0, 100.0]).astype(F)])
        mcfg = _lib.default_match_cfg(**CAPS)
        query = np.ascontiguousarray(synth.velodyne_scan(32, 512, 12.0, 5)[:, :3])

        def compare(what):
            assert ctx.map_size() == oc.size() == twin.map_size(), what
            pts, tpts = ctx.map_points(), twin.map_points()
            np.testing.assert_array_equal(sort_rows(pts), sort_rows(oc.points()), err_msg=what)
            np.testing.assert_array_equal(pts, tpts, err_msg=what)      # row for row, not only as sets
            _check(ctx, what); _check(twin, what)
            idx, sqd, cnt = ctx.knn(q, 5)
            onbr, osqd, ocnt, _ = oc.knn(q, 5)
            np.testing.assert_array_equal(sqd, osqd, err_msg=what)
            np.testing.assert_array_equal(cnt, ocnt, err_msg=what)
            _knn_indices_address(pts, q, idx, sqd, cnt)
            tidx, tsqd, tcnt = twin.knn(q, 5)
            np.testing.assert_array_equal(sqd, tsqd, err_msg=what)
            _same_neighbours(idx, tidx, sqd, what)
            (ik, sk, ck), (tik, tsk, tck) = ctx.knn_k(q, 12, 3.0), twin.knn_k(q, 12, 3.0)   # (distance, insertion index) order: indices too
            np.testing.assert_array_equal(sk, tsk, err_msg=what)
            np.testing.assert_array_equal(ck, tck, err_msg=what)
            np.testing.assert_array_equal(ik, tik, err_msg=what)
            # one registration pass: the same sums, bit for bit (the same map layout, the same pass)
            res = []
            for c in (ctx, twin):
                c.scan_set(query)
                res.append(c.match_reduce(x26, mcfg))
            assert res[0][2] == res[1][2] > 2000, what
            np.testing.assert_array_equal(res[0][0], res[1][0], err_msg=what)
            np.testing.assert_array_equal(res[0][1], res[1][1], err_msg=what)

        compare("right after the carve")
        np.testing.assert_array_equal(ctx.map_points(), kept)
        later = [kept[::2] + F(0.01), synth.box_world_map(8000, 12.0, 3), std["ghost"] + F(0.05),
                 rng.uniform(-40, 40, (6000, 3)).astype(F)]
        for k, b in enumerate(later):
            ctx.map_add(b); twin.map_add(b); oc.update(b)
            compare("batch %d after the carve" % k)
    finally:
        ctx.close(); twin.close()


# ---- 5. tile edges of the compaction --------------------------------------------------------------------------------------------------
def _wall_scene(n, through):
    """Sensor at the origin looking along +x at a dense wall of returns at x = 10; stored points in front of it (x = 5: seen through)
    where `through`, behind it (x = 12: kept) elsewhere, all inside the wall's pixels."""
    rng = np.random.default_rng(n)
    g = np.arange(-2.0, 2.0001, 0.1)
    yy, zz = np.meshgrid(g, g, indexing="ij")
    scan = np.stack([np.full(yy.size, 10.0), yy.ravel(), zz.ravel()], 1).astype(F)
    pts = np.stack([np.where(through, 5.0, 12.0), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], 1).astype(F)
    return scan, pts


@pytest.mark.parametrize("n", [CROP_TILE - 1, CROP_TILE, CROP_TILE + 1, 3 * CROP_TILE + 5])
def test_tile_edges_of_the_compaction(built, n):
    through = np.zeros(n, bool)
    slots = [0, 1, 2, n - 3, n - 2, n - 1]
    for b in range(CROP_TILE, n + 1, CROP_TILE):
        slots += [b - 2, b - 1, b, b + 1]
    slots += [64 * k + d for k in (1, 31, 32, 33, 127) for d in (-1, 0)]      # wave and row edges inside a tile
    through[[s for s in slots if 0 <= s < n]] = True
    scan, pts = _wall_scene(n, through)
    x26, sensor = _ident((0.0, 0.0, 0.0)), F([0, 0, 0])
    cfg = dict(res=64, win=1, margin=0.2, rel_margin=0.02)
    ctx = _ctx([pts], scan, downsample=False)
    try:
        np.testing.assert_array_equal(ctx.map_points(), pts)
        want = _expect(ctx, x26, sensor, **cfg)
        np.testing.assert_array_equal(want, through)                    # (the scene is what it was built to be)
        mask, count = ctx.map_seen_through(x26, sensor, **cfg)
        np.testing.assert_array_equal(mask, want); assert count == through.sum()
        assert ctx.map_carve(x26, sensor, **cfg) == through.sum()
        np.testing.assert_array_equal(ctx.map_points(), pts[~through])
        _check(ctx, "n = %d" % n)
        # ... and its complement: almost everything goes, the kept points are the tile edges
        scan2, pts2 = _wall_scene(n, ~through)
        ctx.map_clear()
        ctx.map_add(pts2)
        assert ctx.map_carve(x26, sensor, **cfg) == n - through.sum()
        np.testing.assert_array_equal(ctx.map_points(), pts2[through])
        _check(ctx, "complement, n = %d" % n)
    finally:
        ctx.close()


# ---- 6. nothing removed means nothing changes -----------------------------------------------------------------------------------------
def test_a_carve_that_removes_nothing_changes_nothing(built, std):
    from fast_limo_amd import _lib
    x26, sensor = std["x26"], std["sensor"]
    cfg = cc.STD_CFG
    # an empty map
    ctx = _lib.HipCtx(0)
    try:
        ctx.scan_set(std["scan"])
        assert ctx.map_carve(x26, sensor, **cfg) == 0
        mask, count = ctx.map_seen_through(x26, sensor, **cfg)
        assert len(mask) == 0 and count == 0
        assert ctx.map_carve_stats() == dict(carves=0, points_removed=0)
    finally:
        ctx.close()
    ctx = _ctx([std["static"], std["ghost"]], np.zeros((0, 3), F))
    twin = _ctx([std["static"], std["ghost"]], std["scan"])
    try:
        pts = ctx.map_points().copy()
        q = np.random.default_rng(5).uniform(-13, 13, (2000, 3)).astype(F)
        state0 = (ctx.map_index_layout(), ctx.map_index_bytes(), ctx.grid_selfcheck(), ctx.knn(q, 5))

        def unchanged(what):
            assert ctx.map_index_layout() == state0[0], what
            assert ctx.map_index_bytes() == state0[1], what
            assert ctx.grid_selfcheck() == state0[2] and state0[2][0] == 0, what
            for a, b in zip(ctx.knn(q, 5), state0[3]):
                np.testing.assert_array_equal(a, b, err_msg=what)
            np.testing.assert_array_equal(ctx.map_points(), pts, err_msg=what)
            assert ctx.map_carve_stats() == dict(carves=0, points_removed=0), what
            assert ctx.map_crop_stats() == dict(crops=0, points_removed=0), what

        # an empty scan: no return, nothing is seen through -- also with a box (the box alone is flimo_map_crop_box's business)
        assert ctx.map_carve(x26, sensor, **cfg) == 0
        assert ctx.map_carve(x26, sensor, box=(F([-1, -1, -1]), F([1, 1, 1])), **cfg) == 0
        mask, count = ctx.map_seen_through(x26, sensor, **cfg)
        assert count == 0 and not mask.any() and len(mask) == len(pts)
        unchanged("an empty scan")
        # a scan that sees nothing through: a margin beyond the scene, a depth bound in front of everything
        ctx.scan_set(std["scan"])
        for c in (dict(res=64, win=1, margin=60.0, rel_margin=0.0), dict(res=64, win=1, margin=0.0, rel_margin=0.0, max_depth=1e-3)):
            assert not _expect(ctx, x26, sensor, **c).any()
            assert ctx.map_carve(x26, sensor, **c) == 0
            assert ctx.map_carve(x26, sensor, box=(F([-1e30] * 3), F([1e30] * 3)), **c) == 0
            unchanged(str(c))
        # a following add is decided as if no carve had been called
        nxt = synth.box_world_map(6000, 11.0, 77) + F([1.0, 0.5, 0.0])
        ctx.map_add(nxt); twin.map_add(nxt)
        np.testing.assert_array_equal(ctx.map_points(), twin.map_points())
        assert ctx.grid_selfcheck() == twin.grid_selfcheck()
        assert ctx.map_index_bytes() == twin.map_index_bytes()
    finally:
        ctx.close(); twin.close()


def test_a_carve_that_removes_everything_leaves_the_map_as_such_a_crop_does(built, oracle):
    """Stored points on one ray in front of a wall of returns."""
    from fast_limo_amd import _lib
    scan, _ = _wall_scene(4, np.zeros(4, bool))
    ray = np.stack([1.0 + 0.5 * np.arange(14), np.zeros(14), np.zeros(14)], 1).astype(F) + F([0, 0.01, 0.01])
    x26, sensor = _ident((0.0, 0.0, 0.0)), F([0, 0, 0])
    cfg = dict(res=64, win=1, margin=0.2, rel_margin=0.02)
    ctx, twin = _ctx([ray], scan, downsample=False), _ctx([ray], scan, downsample=False)
    try:
        assert ctx.map_size() == 14
        assert _expect(ctx, x26, sensor, **cfg).all()
        assert ctx.map_carve(x26, sensor, **cfg) == 14
        assert twin.map_crop_box([500.0] * 3, [501.0] * 3) == 14
        q = np.random.default_rng(6).uniform(-5, 9, (500, 3)).astype(F)
        for c in (ctx, twin):
            assert c.map_size() == 0 and len(c.map_points()) == 0
            idx, sqd, cnt = c.knn(q, 5)
            assert np.all(cnt == 0) and np.all(idx == -1)
            assert c._L.flimo_map_last_time(c._h) == 0.5
            assert c.grid_selfcheck()[0] == 0
        assert ctx.map_index_layout() == twin.map_index_layout()
        assert ctx.map_index_bytes() == twin.map_index_bytes()
        assert ctx.map_carve_stats() == dict(carves=1, points_removed=14) and ctx.map_crop_stats() == dict(crops=0, points_removed=0)
        assert ctx.map_carve(x26, sensor, **cfg) == 0                  # an empty map: nothing to remove
        nxt = synth.box_world_map(9000, 14.0, 78)
        oc = oracle.Octree(0.2, False)
        for c in (ctx, twin, oc):
            (c.update if c is oc else c.map_add)(nxt)
        np.testing.assert_array_equal(ctx.map_points(), twin.map_points())
        np.testing.assert_array_equal(ctx.knn(q, 5)[1], oc.knn(q, 5)[1])
        _check(ctx, "first add after everything went")
    finally:
        ctx.close(); twin.close()


# ---- 7. invalid arguments -------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_and_map_are_untouched(built, std):
    from fast_limo_amd import _lib
    ctx = _ctx([std["static"], std["ghost"]], std["scan"])
    try:
        L, h = ctx._L, ctx._h
        pts = ctx.map_points().copy()
        n = len(pts)
        sc = ctx.grid_selfcheck()
        good_x, good_s = np.ascontiguousarray(std["x26"], dtype=np.float64), std["sensor"].copy()
        lo, hi = F([-5, -5, -5]), F([5, 5, 5])

        def bad_x(i, v):
            x = good_x.copy(); x[i] = v
            return x

        def K(**kw):
            return _lib.carve_cfg(**dict(cc.STD_CFG, **kw))

        ptr = lambda a: None if a is None else a.ctypes.data
        cases = [("null x26", None, good_s, K()), ("null sensor", good_x, None, K()), ("null cfg", good_x, good_s, None),
                 ("nan position", bad_x(1, np.nan), good_s, K()), ("inf position", bad_x(0, np.inf), good_s, K()),
                 ("nan rotation", bad_x(4, np.nan), good_s, K()), ("inf rotation", bad_x(6, -np.inf), good_s, K()),
                 ("nan sensor", good_x, F([0, np.nan, 0]), K()), ("inf sensor", good_x, F([np.inf, 0, 0]), K()),
                 ("res 7", good_x, good_s, K(res=7)), ("res 1025", good_x, good_s, K(res=1025)), ("res 0", good_x, good_s, K(res=0)),
                 ("win -1", good_x, good_s, K(win=-1)), ("win 4", good_x, good_s, K(win=4)),
                 ("nan margin", good_x, good_s, K(margin=np.nan)), ("negative margin", good_x, good_s, K(margin=-0.1)),
                 ("nan rel_margin", good_x, good_s, K(rel_margin=np.nan)), ("negative rel_margin", good_x, good_s, K(rel_margin=-1.0)),
                 ("nan max_depth", good_x, good_s, K(max_depth=np.nan)), ("max_depth 0", good_x, good_s, K(max_depth=0.0)),
                 ("negative max_depth", good_x, good_s, K(max_depth=-3.0))]
        for what, x, s, k in cases:
            kp = None if k is None else C.byref(k)
            count, mask = C.c_size_t(5), np.full(n, 7, np.uint8)
            assert L.flimo_map_seen_through(h, ptr(x), ptr(s), kp, mask.ctypes.data, n, C.byref(count)) == ERR_INVALID, what
            assert count.value == 5 and np.all(mask == 7), what
            removed = C.c_size_t(5)
            assert L.flimo_map_carve(h, ptr(x), ptr(s), kp, None, None, C.byref(removed)) == ERR_INVALID, what
            assert L.flimo_map_carve(h, ptr(x), ptr(s), kp, lo.ctypes.data, hi.ctypes.data, C.byref(removed)) == ERR_INVALID, what
            assert removed.value == 5, what
        k = K()
        nan = F([-5, np.nan, -5])
        for what, blo, bhi in (("lo only", lo, None), ("hi only", None, hi), ("nan lo", nan, hi), ("nan hi", lo, F([5, 5, np.nan])),
                               ("lo > hi", hi, lo), ("lo > hi on one axis", F([-5, 6, -5]), hi)):
            removed = C.c_size_t(5)
            assert L.flimo_map_carve(h, good_x.ctypes.data, good_s.ctypes.data, C.byref(k), ptr(blo), ptr(bhi), C.byref(removed)) == ERR_INVALID, what
            assert removed.value == 5, what
        count, mask = C.c_size_t(5), np.full(n, 7, np.uint8)
        assert L.flimo_map_seen_through(h, good_x.ctypes.data, good_s.ctypes.data, C.byref(k), mask.ctypes.data, n - 1, C.byref(count)) == ERR_INVALID
        assert count.value == 5 and np.all(mask == 7)
        with pytest.raises(_lib.FlimoError):
            ctx.map_carve(good_x, good_s, res=4)
        np.testing.assert_array_equal(ctx.map_points(), pts)
        assert ctx.grid_selfcheck() == sc
        assert ctx.map_carve_stats() == dict(carves=0, points_removed=0) and ctx.map_crop_stats() == dict(crops=0, points_removed=0)
        # the limits themselves are accepted; count and removed may be NULL; without a mask cap does not matter
        for kk in (K(res=8, win=3), K(res=1024, win=0), K(max_depth=INF), K(margin=0.0, rel_margin=0.0)):
            assert L.flimo_map_seen_through(h, good_x.ctypes.data, good_s.ctypes.data, C.byref(kk), None, 0, None) == 0
        assert L.flimo_map_carve(h, good_x.ctypes.data, good_s.ctypes.data, C.byref(K(margin=60.0)), None, None, None) == 0
        np.testing.assert_array_equal(ctx.map_points(), pts)
    finally:
        ctx.close()


# ---- 8. the Localizer's policy --------------------------------------------------------------------------------------------------------
N_SWEEPS = 6                                # registered sweeps (the first call of a drive is the reference's null iteration)
SENSOR_SIGMA = 1e-2                         # synth.velodyne_scan's range noise [m]


def _drive(locs, per_sweep):
    """The standard scene's sweep (fresh noise per sweep) from T* into every Localizer of `locs`, a stationary IMU between them;
    per_sweep(j, rcs) after registered sweep j = 1 .. N_SWEEPS."""
    st, w, a = synth.stationary_imu(0.0, 0.1 * (N_SWEEPS + 1) + 0.06)
    i = j = 0
    for k in range(N_SWEEPS + 1):
        until = 0.1 * (k + 1) + 0.005
        while i < len(st) and st[i] <= until:
            for L in locs:
                L.update_imu(st[i], w[i], a[i])
            i += 1
        scan = synth.velodyne_scan(32, 900, 12.0, 9 + k)
        rcs = [L.update_pointcloud(scan, 0.1 * k) for L in locs]
        assert len(set(rcs)) == 1 and rcs[0] == (1 if k == 0 else 0), (k, rcs)
        if rcs[0] == 0:
            j += 1
            per_sweep(j, rcs)
    assert j == N_SWEEPS


def test_policy_carves_every_second_sweep_exactly_as_a_host_replay(built, std):
    """A: set_map_carving(2, cfg).  B: no policy; the test applies the rule (api.CarveRule), the sensor origin (api.carve_sensor)
    and the yardstick's mask by hand after sync() -- flimo_map_carve must remove exactly that mask --: x, P and the map of A and B
    are bit-identical after every sweep.  G: the same policy over a map that never had the ghost."""
    from fast_limo_amd import api
    cfg = cc.STD_CFG
    A, B, G = (api.Localizer(api.default_cfg(**CAPS)) for _ in range(3))
    try:
        for L in (A, B):
            L.map_add(np.concatenate([std["static"], std["ghost"]]))
        G.map_add(std["static"])
        first = B.hip.map_points().copy()
        ghost_rows = set(_rows(std["ghost"]).tolist())
        is_ghost0 = np.array([r in ghost_rows for r in _rows(first).tolist()])
        static0 = first[~is_ghost0]
        assert is_ghost0.sum() > 0.5 * cc.N_GHOST
        A.set_map_carving(2, **cfg)
        G.set_map_carving(2, **cfg)
        rule = api.CarveRule(2)
        log = dict(ghost=[], xa=[], xg=[], carved=[])

        def per_sweep(j, rcs):
            B.sync()
            if rule.step():
                x = B.get_x()
                sensor = api.carve_sensor(x)
                before = B.hip.map_points().copy()
                mask = cc.yardstick(B.hip.scan_to_world(x), before, sensor, **cfg)
                removed = B.hip.map_carve(x, sensor, **cfg)
                assert removed == mask.sum(), j
                np.testing.assert_array_equal(B.hip.map_points(), before[~mask], err_msg="sweep %d" % j)
                log["carved"].append(j)
                assert A.last_carve_removed() == removed, j
            np.testing.assert_array_equal(A.get_x(), B.get_x(), err_msg="sweep %d" % j)
            np.testing.assert_array_equal(A.get_P(), B.get_P(), err_msg="sweep %d" % j)
            np.testing.assert_array_equal(A.hip.map_points(), B.hip.map_points(), err_msg="sweep %d" % j)
            assert A.hip.grid_selfcheck()[0] == 0, j
            now = set(_rows(B.hip.map_points()).tolist())
            log["ghost"].append(sum(1 for r in _rows(first[is_ghost0]).tolist() if r in now))
            log["xa"].append(A.get_x()); log["xg"].append(G.get_x())

        _drive((A, B, G), per_sweep)
        assert log["carved"] == [2, 4, 6]
        assert A.hip.map_carve_stats()["carves"] == B.hip.map_carve_stats()["carves"] >= 1
        assert A.hip.map_crop_stats() == dict(crops=0, points_removed=0)
        final = set(_rows(A.hip.map_points()).tolist())
        assert all(r in final for r in _rows(static0).tolist())         # no static point of the first map is gone
        print("ghost points left after each sweep: %s of %d" % (log["ghost"], is_ghost0.sum()))
        assert log["ghost"][-1] <= is_ghost0.sum() - 0.7 * is_ghost0.sum()
        gone = [j for j, g in enumerate(log["ghost"]) if g == 0]
        xa, xg = np.array(log["xa"]), np.array(log["xg"])
        if gone:
            np.testing.assert_array_equal(xa[gone[0] + 1:], xg[gone[0] + 1:])
        dev = np.abs(xa[:, 0:3] - xg[:, 0:3]).max()
        print("trajectory against the drive whose map never had the ghost: max |dpos| = %.3e m" % dev)
        assert dev <= SENSOR_SIGMA
    finally:
        for L in (A, B, G):
            L.close()


def test_policy_with_the_local_map_due_on_the_same_sweep_pays_one_relayout(built, std):
    from fast_limo_amd import api
    cfg = cc.STD_CFG
    half, recentre = F([9.0, 9.0, 30.0]), 5.0                          # cuts the walls at +-12 m off: the crop removes points
    Cc, D = api.Localizer(api.default_cfg(**CAPS)), api.Localizer(api.default_cfg(**CAPS))
    try:
        for L in (Cc, D):
            L.map_add(np.concatenate([std["static"], std["ghost"]]))
        Cc.set_local_map(half, recentre)
        Cc.set_map_carving(1, **cfg)
        seen = {}

        def per_sweep(j, rcs):
            if j > 1:
                return
            Cc.sync(); D.sync()
            # D: the same insert and nothing else -- what the insert alone costs in layouts
            x = D.get_x()
            before = D.hip.map_points().copy()
            lo, hi = api.LocalMapRule(half, recentre).step(x[0:3])
            sensor = api.carve_sensor(x)
            keep = ~cc.yardstick(D.hip.scan_to_world(x), before, sensor, **cfg) & _inside(before, lo, hi)
            assert 0 < keep.sum() < len(before) - 1000
            seen["builds"] = (Cc.hip.grid_selfcheck()[2], D.hip.grid_selfcheck()[2])
            np.testing.assert_array_equal(Cc.hip.map_points(), before[keep])
            assert Cc.hip.map_carve_stats()["carves"] == 1 and Cc.hip.map_crop_stats()["crops"] == 0
            assert Cc.last_carve_removed() == len(before) - keep.sum()

        b0 = (Cc.hip.grid_selfcheck()[2], D.hip.grid_selfcheck()[2])
        _drive((Cc, D), per_sweep)
        assert b0[0] == b0[1]
        assert seen["builds"][0] - b0[0] == seen["builds"][1] - b0[1] + 1, (b0, seen)      # one relayout, not two
        assert Cc.hip.grid_selfcheck()[0] == 0
    finally:
        Cc.close(); D.close()


def test_policy_switched_off_is_the_plain_localizer(built, std):
    from fast_limo_amd import api
    P, Q, U = (api.Localizer(api.default_cfg(**CAPS)) for _ in range(3))
    try:
        for L in (P, Q, U):
            L.map_add(np.concatenate([std["static"], std["ghost"]]))
        P.set_map_carving(2, **cc.STD_CFG)
        P.set_map_carving(0, **cc.STD_CFG)                              # off again
        Q.set_map_carving(1, **dict(cc.STD_CFG, res=4))                 # an invalid cfg: off

        def per_sweep(j, rcs):
            for L in (P, Q):
                np.testing.assert_array_equal(L.get_x(), U.get_x())
                np.testing.assert_array_equal(L.get_P(), U.get_P())

        _drive((P, Q, U), per_sweep)
        for L in (P, Q):
            np.testing.assert_array_equal(L.hip.map_points(), U.hip.map_points())
            assert L.hip.map_carve_stats() == dict(carves=0, points_removed=0)
            assert L.hip.grid_selfcheck() == U.hip.grid_selfcheck()
    finally:
        for L in (P, Q, U):
            L.close()
