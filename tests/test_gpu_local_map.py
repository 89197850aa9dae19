"""GPU suite: the local map -- flimo_map_crop_box forgets the stored points outside a box, Localizer::set_local_map keeps the box
around the sensor.  The reference's octree has no erase, so the meaning is this project's: the kept points stay in insertion order,
and from then on the map is the reference octree's clear() + initialize(kept) (Objects/Octree.hpp:186-189, 282-298).  That makes
every statement below checkable against the oracle's octree, bit for bit; the one tolerance (the trajectory of a drive with the
policy on, test 5 c) is the synthetic sensor's own range noise.  Everything goes through the C ABI (_lib.HipCtx / api.Localizer)."""
import ctypes as C
import os

import numpy as np
import pytest

from common import CAPS, sort_rows
from fast_limo_amd import synth
from insert_rule_common import _stored_of_batch

pytestmark = pytest.mark.gpu

ERR_INVALID = -2


def _inside(pts, lo, hi):
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return np.all((pts >= lo) & (pts <= hi), axis=1)                  # float32 compares, bounds inclusive


def _check(ctx, what=""):
    mm, merges, builds = ctx.grid_selfcheck()
    assert mm == 0, (what, mm, merges, builds)
    return merges, builds


def _parity_batches(rng):
    """The batches of test_device_insert_rule_matches_octree: dense re-inserts, splits, child creation, root growth, NaNs."""
    base = synth.box_world_map(20000, 12.0, 3)
    batches = [base, base[::2] + np.float32(0.01)]
    batches += [synth.box_world_map(6000, 12.0 + 4 * k, 10 + k) + np.float32([k * 2.5, -k, 0]) for k in range(3)]
    batches.append(np.array([[400.0, 3, 1], [-300.0, 2, 1]], np.float32))
    with_nan = synth.box_world_map(3000, 14.0, 21)
    with_nan[::17] = np.nan
    batches.append(with_nan)
    batches.append(rng.normal(0, 0.05, (5000, 3)).astype(np.float32) + np.float32([3, 3, 0.5]))
    batches.append(rng.uniform(-60, 60, (20000, 3)).astype(np.float32))
    batches.append(base[:1])
    return batches


def _box_through_stored_points(pts, lo_want, hi_want):
    """The bounding box of the stored points inside the wanted box: it keeps the same points, and on each of its six faces lies a
    stored point that is kept (bounds are inclusive)."""
    s = pts[_inside(pts, lo_want, hi_want)]
    return s.min(0).astype(np.float32), s.max(0).astype(np.float32)


def _knn_indices_address(ctx_pts, q, idx, sqd, cnt):
    """|q - pts[idx]|^2 reproduces sqd.  Recomputed in float64 from the float32 inputs; the device's float32 value differs from that
    by the roundings of one subtraction, one square and two additions per term: a few 2^-24 relative, 2e-6 with room."""
    for k in range(idx.shape[1]):
        ok = cnt > k
        assert np.all(idx[ok, k] >= 0) and np.all(idx[ok, k] < len(ctx_pts))
        d = (q[ok].astype(np.float64) - ctx_pts[idx[ok, k]].astype(np.float64))
        np.testing.assert_allclose((d * d).sum(1), sqd[ok, k].astype(np.float64), rtol=2e-6, atol=1e-12)


def _same_neighbours(idx_a, idx_b, sqd, what):
    """The same neighbour indices.  Where float32 distances inside a row tie exactly (queries hundreds of metres from the map: the
    squared distances have a resolution of metres), flimo_knn's order among the tied ones follows their places in the cell-sorted
    array, which depend on the order in which rows were moved by earlier inserts -- two contexts fed the same batches and never
    cropped differ there too.  So: equal element for element where the row's distances are pairwise different, and equal as
    sets within each group of equal distances elsewhere."""
    diff = np.where(np.any(idx_a != idx_b, axis=1))[0]
    for r in diff:
        assert len(np.unique(sqd[r])) < sqd.shape[1], (what, r, sqd[r], idx_a[r], idx_b[r])
        oa, ob = np.lexsort((idx_a[r], sqd[r])), np.lexsort((idx_b[r], sqd[r]))
        np.testing.assert_array_equal(idx_a[r][oa], idx_b[r][ob], err_msg="%s row %d" % (what, r))
    assert len(diff) <= 0.01 * len(idx_a), (what, len(diff))


# ---- 1. crop = filter, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("downsample", [True, False])
def test_crop_is_the_numpy_filter_in_insertion_order(built, oracle, downsample):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(7)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(0.2, 2, downsample)
        for k, b in enumerate(_parity_batches(rng)):
            ctx.map_add(b, stamp=0.5 + k)
        before = ctx.map_points().copy()
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        lo, hi = _box_through_stored_points(before, [-13.0, -10.0, -3.0], [10.0, 13.0, 8.0])
        ins = _inside(before, lo, hi)
        # points exactly on every one of the six bounds, and they are kept
        for a in range(3):
            assert np.any(ins & (before[:, a] == lo[a])) and np.any(ins & (before[:, a] == hi[a])), a
        assert 0.1 * len(before) < ins.sum() < 0.9 * len(before), (ins.sum(), len(before))
        removed = ctx.map_crop_box(lo, hi)
        print("crop: %d -> %d points (%d removed)" % (len(before), ins.sum(), removed))
        assert removed == len(before) - ins.sum()
        assert ctx.map_size() == ins.sum()
        after = ctx.map_points()
        np.testing.assert_array_equal(after, before[ins])              # same rows, same (insertion) order
        _check(ctx, "after the crop")
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before          # a crop is no insert
        assert ctx.map_crop_stats() == dict(crops=1, points_removed=removed)
        # the same box again removes nothing
        assert ctx.map_crop_box(lo, hi) == 0
        np.testing.assert_array_equal(ctx.map_points(), before[ins])
        assert ctx.map_crop_stats() == dict(crops=1, points_removed=removed)
        # a second, smaller box: the filter of the filter
        lo2, hi2 = lo + np.float32(2.0), hi - np.float32(2.5)
        ins2 = _inside(after, lo2, hi2)
        assert ctx.map_crop_box(lo2, hi2) == len(after) - ins2.sum() > 0
        np.testing.assert_array_equal(ctx.map_points(), after[ins2])
        _check(ctx, "after the second crop")
    finally:
        ctx.close()


# ---- 2. afterwards the map is the oracle's fresh octree -------------------------------------------------------------------------
def test_after_a_crop_the_map_is_a_fresh_octree_of_the_kept_points(built, oracle):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(11)
    first = _parity_batches(rng)[:5]
    ctx, twin = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        for c in (ctx, twin):
            c.map_config(0.2, 2, True)
            for b in first:
                c.map_add(b)
        before = ctx.map_points().copy()
        lo, hi = _box_through_stored_points(before, [-13.0, -9.0, -3.0], [9.0, 13.0, 7.0])
        kept = before[_inside(before, lo, hi)]
        assert ctx.map_crop_box(lo, hi) == len(before) - len(kept) > 0
        _check(ctx, "crop")
        twin.map_clear()                                               # what a caller without the crop would do
        twin.map_add(kept)
        oc = oracle.Octree(0.2, True)
        oc.update(kept)
        assert oc.size() == len(kept)                                  # initialize drops nothing

        mid = 0.5 * (lo + hi)
        q = np.concatenate([
            (rng.uniform(0, 1, (1500, 3)) * (hi - lo) + lo).astype(np.float32),                              # inside the box
            kept[rng.choice(len(kept), 500)] + rng.normal(0, 0.05, (500, 3)).astype(np.float32),             # near kept surfaces
            np.stack([np.full(200, lo[0]), rng.uniform(lo[1], hi[1], 200), rng.uniform(lo[2], hi[2], 200)], 1).astype(np.float32),  # on a face
            np.stack([rng.uniform(lo[0], hi[0], 200), np.full(200, hi[1]), rng.uniform(lo[2], hi[2], 200)], 1).astype(np.float32),
            np.array([lo, hi, [lo[0], hi[1], lo[2]]], np.float32),                                              # on corners
            (rng.uniform(-30, 30, (200, 3)) + [400.0, 0.0, 0.0]).astype(np.float32),                          # where forgotten points were
            (rng.uniform(-50, 50, (100, 3)) + [-5000.0, 3000.0, 100.0]).astype(np.float32),                   # far outside everything
            mid[None].astype(np.float32)])

        def compare(what):
            assert ctx.map_size() == oc.size() == twin.map_size(), what
            pts, tpts = ctx.map_points(), twin.map_points()
            np.testing.assert_array_equal(sort_rows(pts), sort_rows(oc.points()), err_msg=what)
            np.testing.assert_array_equal(pts, tpts, err_msg=what)      # row for row, not only as sets
            _check(ctx, what)
            _check(twin, what)
            idx, sqd, cnt = ctx.knn(q, 5)
            onbr, osqd, ocnt, _ = oc.knn(q, 5)
            np.testing.assert_array_equal(sqd, osqd, err_msg=what)
            np.testing.assert_array_equal(cnt, ocnt, err_msg=what)
            _knn_indices_address(pts, q, idx, sqd, cnt)
            tidx, tsqd, tcnt = twin.knn(q, 5)
            np.testing.assert_array_equal(sqd, tsqd, err_msg=what)
            np.testing.assert_array_equal(cnt, tcnt, err_msg=what)
            _same_neighbours(idx, tidx, sqd, what)                      # indices included

        compare("right after the crop")
        np.testing.assert_array_equal(ctx.map_points(), kept)
        with_nan = synth.box_world_map(4000, 10.0, 33) + np.float32([1, -1, 0])
        with_nan[::13] = np.nan
        later = [
            kept[::2] + np.float32(0.01),                                                  # dense over the kept region: whole-leaf drops
            synth.box_world_map(15000, 12.0, 3),                                           # the first batch again: counts restart, leaves split
            rng.normal(0, 0.05, (4000, 3)).astype(np.float32) + mid.astype(np.float32),    # one tight cluster inside the box
            with_nan,
            synth.box_world_map(8000, 20.0, 41) + np.float32([60.0, 5.0, 0.0]),            # outside the old box
            np.array([[700.0, 3, 1], [-900.0, 2, 1]], np.float32),                         # root growth, both corners
            rng.uniform(-60, 60, (15000, 3)).astype(np.float32),                           # sparse: many child creations
            kept[:1],
        ]
        for k, b in enumerate(later):
            ctx.map_add(b)
            twin.map_add(b)
            oc.update(b)
            compare("batch %d after the crop" % k)
        print("after the crop + %d batches: %d points" % (len(later), ctx.map_size()))
    finally:
        ctx.close()
        twin.close()


# ---- 3. a moving box over many batches, against the oracle alone ----------------------------------------------------------------
MOVING_BOX_SIZES = [(35000, 32307), (69027, 56595), (90703, 70085), (102924, 76431), (101780, 70385), (103596, 72704)]


def test_moving_box_over_twelve_batches_against_the_oracle(built, oracle):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(0.2, 2, True)
        oc = oracle.Octree(0.2, True)                                   # one fresh octree per crop epoch
        expect = np.zeros((0, 3), np.float32)                           # the map in insertion order, from oracle octrees only
        crops = []
        for k in range(12):
            b = synth.box_world_map(20000, 12.0, k) + np.float32([4 * k, 0, 0])
            if k % 3 == 1:
                b = np.concatenate([b, b[::2]])                         # half of itself appended again
            pts0 = oc.points() if oc.size() else np.zeros((0, 3), np.float32)
            oc.update(b)
            expect = np.concatenate([expect, _stored_of_batch(b, pts0, oc.points())])
            ctx.map_add(b)
            assert ctx.map_size() == oc.size() == len(expect), k
            if crops:
                _check(ctx, "batch %d" % k)                             # an add that follows a crop
            if k % 2 == 1:
                lo = np.float32([4 * k - 15, -15, -5])
                hi = np.float32([4 * k + 15, 15, 20])
                kept = expect[_inside(expect, lo, hi)]
                removed = ctx.map_crop_box(lo, hi)
                crops.append((len(expect), len(kept)))
                assert removed == len(expect) - len(kept) > 0, (k, removed)
                _check(ctx, "crop after batch %d" % k)
                np.testing.assert_array_equal(ctx.map_points(), kept, err_msg="crop after batch %d" % k)
                oc = oracle.Octree(0.2, True)
                oc.update(kept)
                assert oc.size() == len(kept)                           # initialize drops nothing
                expect = kept
        print("moving box:", crops)
        assert crops == MOVING_BOX_SIZES, crops
        assert ctx.map_crop_stats()["crops"] == 6
        # registration on top: a scan taken inside the last box against the last epoch's octree
        x = np.zeros(26); x[6] = 1; x[10] = 1; x[25] = -9.809; x[0:3] = [44.0, 0.5, 0.0]
        scan = np.ascontiguousarray(synth.velodyne_scan(32, 512, 12.0, 5)[:, :3])
        ctx.scan_set(scan)
        ctx.set_debug_records(True)
        HTH, HTh, M = ctx.match_reduce(x, _lib.default_match_cfg(**CAPS))
        g = ctx.match_fetch()
        ctx.set_debug_records(False)
        recs, H, h, _ = oracle.match_H(oc, oracle.default_cfg(num_threads=4, **CAPS), x, scan)
        dev = ctx.map_points()
        vg, vo = g["valid"] > 0, recs["is_plane"] > 0
        np.testing.assert_array_equal(vg, vo)
        assert M == H.shape[0] and M > 2000, (M, H.shape)
        np.testing.assert_array_equal(g["sqd"][vg], recs["sqd"][vg])
        np.testing.assert_array_equal(dev[g["nbr"]][vg], recs["nbr"][vg])
        np.testing.assert_array_equal(g["n"][vg], recs["n"][vg])
        np.testing.assert_array_equal(g["H"][vg].astype(np.float64), H)
    finally:
        ctx.close()


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------
def test_a_crop_that_removes_nothing_changes_nothing(built, oracle):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(5)
    batches = _parity_batches(rng)[:5]
    nxt = synth.box_world_map(9000, 14.0, 77) + np.float32([2.0, 1.0, 0.0])
    q = rng.uniform(-14, 14, (3000, 3)).astype(np.float32)
    ctx, twin = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        for c in (ctx, twin):
            c.map_config(0.2, 2, True)
            for b in batches:
                c.map_add(b, stamp=2.5)
        pts = ctx.map_points().copy()
        knn0 = ctx.knn(q, 5)
        ib0, sc0 = ctx.map_index_bytes(), ctx.grid_selfcheck()
        big = np.float32([1e30, 1e30, 1e30])
        for lo, hi in ((-big, big), (np.float32([-np.inf] * 3), np.float32([np.inf] * 3)), (pts.min(0), pts.max(0))):
            assert ctx.map_crop_box(lo, hi) == 0
        assert ctx.map_crop_stats() == dict(crops=0, points_removed=0)
        np.testing.assert_array_equal(ctx.map_points(), pts)
        for a, b in zip(ctx.knn(q, 5), knn0):
            np.testing.assert_array_equal(a, b)                          # (the same context, the same array: indices bit for bit)
        assert ctx.map_index_bytes() == ib0
        assert ctx.grid_selfcheck() == sc0 and sc0[0] == 0               # {mismatches, in place, full layouts}
        # a following add is decided as if no crop had been called
        ctx.map_add(nxt)
        twin.map_add(nxt)
        np.testing.assert_array_equal(ctx.map_points(), twin.map_points())
        (ia, sa, ca), (ib, sb, cb) = ctx.knn(q, 5), twin.knn(q, 5)
        np.testing.assert_array_equal(sa, sb); np.testing.assert_array_equal(ca, cb)
        _same_neighbours(ia, ib, sa, "add after a crop that removed nothing")
        assert ctx.grid_selfcheck() == twin.grid_selfcheck()
        assert ctx.map_index_bytes() == twin.map_index_bytes()
    finally:
        ctx.close()
        twin.close()


def test_a_crop_that_removes_everything_leaves_a_cleared_map(built, oracle):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(6)
    nxt = synth.box_world_map(9000, 14.0, 78)
    q = rng.uniform(-14, 14, (2000, 3)).astype(np.float32)
    ctx, fresh = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        ctx.map_config(0.2, 2, True)
        fresh.map_config(0.2, 2, True)
        for b in _parity_batches(rng)[:4]:
            ctx.map_add(b, stamp=3.5)
        n = ctx.map_size()
        assert ctx.map_crop_box([5000.0, 5000.0, 5000.0], [5001.0, 5001.0, 5001.0]) == n
        assert ctx.map_size() == 0 and len(ctx.map_points()) == 0
        idx, sqd, cnt = ctx.knn(q, 5)
        assert np.all(cnt == 0) and np.all(idx == -1)
        assert ctx._L.flimo_map_last_time(ctx._h) == 3.5                 # the one thing flimo_map_clear resets and a crop does not
        assert ctx.grid_selfcheck()[0] == 0
        assert ctx.map_crop_box([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]) == 0   # an empty map: nothing to remove
        # the next add is an initialize, like a fresh context's first add
        ctx.map_add(nxt)
        fresh.map_add(nxt)
        _check(ctx, "first add after everything went")
        np.testing.assert_array_equal(ctx.map_points(), fresh.map_points())
        (ia, sa, ca), (ib, sb, cb) = ctx.knn(q, 5), fresh.knn(q, 5)
        np.testing.assert_array_equal(sa, sb); np.testing.assert_array_equal(ca, cb)
        _same_neighbours(ia, ib, sa, "first add after everything went")
        oc = oracle.Octree(0.2, True)
        oc.update(nxt)
        np.testing.assert_array_equal(ctx.knn(q, 5)[1], oc.knn(q, 5)[1])
        again = nxt[::3] + np.float32(0.02)
        ctx.map_add(again); fresh.map_add(again); oc.update(again)
        _check(ctx, "second add")
        np.testing.assert_array_equal(ctx.map_points(), fresh.map_points())
        np.testing.assert_array_equal(sort_rows(ctx.map_points()), sort_rows(oc.points()))
    finally:
        ctx.close()
        fresh.close()


def test_invalid_boxes_are_refused_and_the_map_is_untouched(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    try:
        lo, hi = np.float32([-5, -5, -5]), np.float32([5, 5, 5])
        removed = C.c_size_t(7)
        assert ctx._L.flimo_map_crop_box(ctx._h, lo.ctypes.data, hi.ctypes.data, C.byref(removed)) == 0 and removed.value == 0   # empty map
        ctx.map_add(synth.box_world_map(20000, 12.0, 3))
        pts = ctx.map_points().copy()
        sc = ctx.grid_selfcheck()
        nan = np.float32([-5, np.nan, -5])
        bad = [(None, hi), (lo, None), (None, None), (nan, hi), (lo, np.float32([5, 5, np.nan])), (hi, lo),
               (np.float32([-5, 6, -5]), hi)]
        for blo, bhi in bad:
            removed = C.c_size_t(7)
            rc = ctx._L.flimo_map_crop_box(ctx._h, None if blo is None else blo.ctypes.data, None if bhi is None else bhi.ctypes.data,
                                           C.byref(removed))
            assert rc == ERR_INVALID and removed.value == 0, (blo, bhi, rc)
        with pytest.raises(_lib.FlimoError):
            ctx.map_crop_box(hi, lo)
        np.testing.assert_array_equal(ctx.map_points(), pts)
        assert ctx.grid_selfcheck() == sc
        assert ctx.map_crop_stats() == dict(crops=0, points_removed=0)
        # lo == hi is a box (of one plane / point), and `removed` may be NULL
        assert ctx._L.flimo_map_crop_box(ctx._h, lo.ctypes.data, hi.ctypes.data, None) == 0
        np.testing.assert_array_equal(ctx.map_points(), pts[_inside(pts, lo, hi)])
        cur = ctx.map_points().copy()
        one = cur[3].copy()
        assert ctx.map_crop_box(one, one) == len(cur) - int(np.all(cur == one, axis=1).sum())
        assert ctx.map_size() >= 1 and np.all(ctx.map_points() == one)
        _check(ctx, "one point left")
    finally:
        ctx.close()


def test_crop_of_a_crowded_map_with_the_second_level_on(built, oracle):
    """test_crowded_cells_second_level_is_exact's recipe (raw sweeps inserted under the sensor: cells with hundreds of points, the
    second-level grid active), then a crop around the sensor: k-NN and a pass's records still equal the fresh octree's."""
    from fast_limo_amd import _lib
    L = 40.0
    mp = synth.box_world_map(150000, L, 5)
    x_true = np.zeros(26); x_true[6] = 1; x_true[10] = 1; x_true[25] = -9.809
    x_true[0:3] = synth.T_STAR_T
    r, p_, y = [np.deg2rad(v) for v in synth.T_STAR_RPY_DEG]
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p_ / 2), np.sin(p_ / 2), np.cos(y / 2), np.sin(y / 2)
    x_true[3:7] = [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]
    sweeps = [np.ascontiguousarray(synth.velodyne_scan(64, 1024, L, 40 + j)[:, :3]) for j in range(6)]
    query = np.ascontiguousarray(synth.velodyne_scan(64, 512, L, 77)[:, :3])
    os.environ["FLIMO_FINE"] = "1"
    os.environ["FLIMO_FINE_THRESHOLD"] = "32"
    os.environ["FLIMO_FINE_MIN_POINTS"] = "0"
    try:
        ctx = _lib.HipCtx(0)
    finally:
        os.environ.pop("FLIMO_FINE"); os.environ.pop("FLIMO_FINE_THRESHOLD"); os.environ.pop("FLIMO_FINE_MIN_POINTS")
    try:
        ctx.map_config()
        ctx.map_add(mp)
        for j, sw in enumerate(sweeps):
            ctx.scan_set(sw)
            ctx.map_add_scan(x_true, 0.1 * (j + 1))
        fs = ctx.fine_stats()
        assert fs["active"] and fs["points"] > 5000, fs
        before = ctx.map_points().copy()
        c3 = np.float32(x_true[0:3])
        lo, hi = c3 - np.float32([22.0, 18.0, 10.0]), c3 + np.float32([22.0, 18.0, 10.0])
        kept = before[_inside(before, lo, hi)]
        assert ctx.map_crop_box(lo, hi) == len(before) - len(kept) > 0
        _check(ctx, "crop of the crowded map")
        np.testing.assert_array_equal(ctx.map_points(), kept)
        print("crowded map: %d -> %d points; second level before %s, after %s" % (len(before), len(kept), fs, ctx.fine_stats()))
        oc = oracle.Octree()
        oc.update(kept)
        rng = np.random.default_rng(9)
        q = np.concatenate([kept[rng.choice(len(kept), 3000)] + rng.normal(0, 0.1, (3000, 3)).astype(np.float32),
                            (rng.uniform(-1, 1, (1000, 3)) * 30).astype(np.float32)])
        idx, sqd, cnt = ctx.knn(q, 5)
        np.testing.assert_array_equal(sqd, oc.knn(q, 5)[1])
        _knn_indices_address(kept, q, idx, sqd, cnt)
        cfg = _lib.default_match_cfg(**CAPS)
        ctx.scan_set(query)
        p1 = ctx.match_reduce(x_true, cfg)                               # first pass (no bound)
        p2 = ctx.match_reduce(x_true, cfg)                               # with the previous pass's bound
        ctx.set_debug_records(True)
        p3 = ctx.match_reduce(x_true, cfg)
        g = ctx.match_fetch()
        ctx.set_debug_records(False)
        for p in (p2, p3):
            assert p[2] == p1[2]                                         # (the sums of different pass layouts differ in summation order)
            np.testing.assert_allclose(p[0], p1[0], rtol=1e-9); np.testing.assert_allclose(p[1], p1[1], rtol=1e-9, atol=1e-9)
        recs, H, h, _ = oracle.match_H(oc, oracle.default_cfg(num_threads=4, **CAPS), x_true, query)
        vg, vo = g["valid"] > 0, recs["is_plane"] > 0
        np.testing.assert_array_equal(vg, vo)
        assert vg.sum() > 2000
        np.testing.assert_array_equal(g["sqd"][vg], recs["sqd"][vg])
        np.testing.assert_array_equal(kept[g["nbr"]][vg], recs["nbr"][vg])
        np.testing.assert_array_equal(g["n"][vg], recs["n"][vg])
        np.testing.assert_array_equal(g["H"][vg].astype(np.float64), H)
        # a sweep inserted after the crop (the crowded cells fill again) and the same questions
        ctx.scan_set(sweeps[0])
        oc.update(ctx.scan_to_world(x_true))
        ctx.map_add_scan(x_true, 0.9)
        _check(ctx, "sweep after the crop")
        assert ctx.map_size() == oc.size()
        np.testing.assert_array_equal(ctx.knn(q, 5)[1], oc.knn(q, 5)[1])
    finally:
        ctx.close()


def test_crop_of_two_places_six_kilometres_apart_to_one_of_them(built, oracle):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(3)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        far = np.float32([6000.0, 6000.0, 0.0])
        a, b = synth.box_world_map(60000, 30.0, 11), synth.box_world_map(60000, 30.0, 12) + far
        ctx.map_add(np.concatenate([a, b]))
        for k in range(4):
            ctx.map_add(synth.box_world_map(3000, 20.0, 20 + k) + (far if k % 2 else np.float32([0, 0, 0])))
        _check(ctx, "two places")
        before = ctx.map_points().copy()
        ib0 = ctx.map_index_bytes()
        lo, hi = far - np.float32([100, 100, 50]), far + np.float32([100, 100, 50])
        kept = before[_inside(before, lo, hi)]
        assert ctx.map_crop_box(lo, hi) == len(before) - len(kept) > 50000
        _check(ctx, "cropped to the far place")
        ib1 = ctx.map_index_bytes()
        print("two places 6 km apart cropped to one: index %d -> %d bytes, tiles %d -> %d, points %d -> %d" %
              (ib0["index"], ib1["index"], ib0["tiles"], ib1["tiles"], len(before), len(kept)))
        assert ib1["index"] < ib0["index"], (ib0, ib1)
        assert ib1["points"] == 16 * len(kept)
        np.testing.assert_array_equal(ctx.map_points(), kept)
        oc = oracle.Octree()
        oc.update(kept)
        q = np.concatenate([(rng.uniform(-25, 25, (1500, 3)) * [1, 1, 0.1] + [0, 0, 2]).astype(np.float32) + far,
                            (rng.uniform(-25, 25, (300, 3)) * [1, 1, 0.1] + [0, 0, 2]).astype(np.float32),      # the forgotten place
                            (rng.uniform(-100, 100, (50, 3)) + [3000.0, 3000.0, 0.0]).astype(np.float32)])
        idx, sqd, cnt = ctx.knn(q, 5)
        np.testing.assert_array_equal(sqd, oc.knn(q, 5)[1])
        _knn_indices_address(kept, q, idx, sqd, cnt)
        extra = synth.box_world_map(3000, 20.0, 31) + far
        ctx.map_add(extra); oc.update(extra)
        _check(ctx, "add after the crop")
        np.testing.assert_array_equal(sort_rows(ctx.map_points()), sort_rows(oc.points()))
        np.testing.assert_array_equal(ctx.knn(q, 5)[1], oc.knn(q, 5)[1])
    finally:
        ctx.close()


# ---- 5. the policy --------------------------------------------------------------------------------------------------------------
# corridor_scan sees 30 m (`view`); INTEGRATION.md: half extent = sensor range + MAX_DIST_PLANE + recentre_dist
SENSOR_RANGE, RECENTRE = 30.0, 5.0
HALF = np.float32([SENSOR_RANGE + 2.0 + RECENTRE] * 3)
RANGE_SIGMA = 0.01                                                      # corridor_scan's range noise [m]


def test_local_map_policy_along_a_corridor_drive(built, oracle):
    """(a) Localizer A with set_local_map against Localizer B without it, to which the test applies flimo_local_map_rule and
    flimo_map_crop_box by hand after sync(): x, P and the map bit-identical after every sweep (asynchronous inserts as shipped).
    (b) every stored point of A inside the last box; the map smaller than an uncropped twin's.
    (c) the trajectory with the policy on against the oracle's UNCROPPED drive: within the sensor's range noise (1 cm).  Measured
    on an MI355X: ATE 8.8e-4 m with the policy on, 6.8e-5 m with it off; the map ends with 58 091 points against 124 560."""
    from fast_limo_amd import api, replay
    n_scans, n_pts, speed = 64, 6000, 10.0
    st, w, a = synth.stationary_imu(0.0, 0.1 * n_scans + 0.06)
    A, B, U = (api.Localizer(api.default_cfg(**CAPS)) for _ in range(3))
    Lo = oracle.Localizer(oracle.default_cfg(num_threads=4, **CAPS))
    try:
        A.set_local_map(HALF, RECENTRE)
        rule = api.LocalMapRule(HALF, RECENTRE)
        x0 = A.get_x(); x0[14] = speed
        for L in (A, B, U, Lo):
            L.set_x(x0)
        i = 0
        box = None
        n_crops = 0
        poses = dict(A=[], U=[], O=[])
        for k in range(n_scans):
            until = 0.1 * (k + 1) + 0.005
            while i < len(st) and st[i] <= until:
                for L in (A, B, U, Lo):
                    L.update_imu(st[i], w[i], a[i])
                i += 1
            scan = synth.corridor_scan(k, n_pts, 77, speed=speed)
            ra, rb, ru, ro = (L.update_pointcloud(scan, 0.1 * k) for L in (A, B, U, Lo))
            assert ra == rb == ru == ro == (1 if k == 0 else 0), (k, ra, rb, ru, ro)
            if rb == 0:                                                  # a registered sweep: its insert, then the rule
                B.sync()
                step = rule.step(B.get_x()[0:3])
                if step is not None:
                    box = step
                    n_crops += 1
                    B.hip.map_crop_box(*box)
                    assert B.hip.grid_selfcheck()[0] == 0, k
            xa, xb = A.get_x(), B.get_x()
            np.testing.assert_array_equal(xa, xb, err_msg="sweep %d" % k)
            np.testing.assert_array_equal(A.get_P(), B.get_P(), err_msg="sweep %d" % k)
            assert A.map_size() == B.map_size(), k
            np.testing.assert_array_equal(A.hip.map_points(), B.hip.map_points(), err_msg="sweep %d" % k)
            assert A.hip.grid_selfcheck()[0] == 0, k
            poses["A"].append(xa); poses["U"].append(U.get_x()); poses["O"].append(Lo.get_x())
        assert A.hip.grid_selfcheck()[0] == 0
        assert A.hip.map_crop_stats()["crops"] == B.hip.map_crop_stats()["crops"] > 3
        assert n_crops >= 10, n_crops                                     # 63 m at 5 m per re-centring
        # (b)
        pts = A.hip.map_points()
        assert box is not None and np.all(_inside(pts, box[0], box[1]))
        assert abs(0.5 * (box[0][0] + box[1][0]) - poses["A"][-1][0]) <= RECENTRE + 1e-3
        size_a, size_u = A.map_size(), U.map_size()
        ib_a, ib_u = A.hip.map_index_bytes(), U.hip.map_index_bytes()
        print("corridor drive, %d sweeps: map %d points with the policy, %d without; index %d / %d bytes" %
              (n_scans, size_a, size_u, ib_a["index"], ib_u["index"]))
        assert size_a < size_u
        # (c)
        ate_cropped = replay.ate(poses["A"], poses["O"])
        ate_uncropped = replay.ate(poses["U"], poses["O"])
        print("ATE against the oracle's uncropped drive: policy on %.3e m, policy off %.3e m" % (ate_cropped, ate_uncropped))
        assert ate_cropped <= RANGE_SIGMA, (ate_cropped, ate_uncropped)
    finally:
        for L in (A, B, U):
            L.close()


def test_local_map_policy_switched_off_by_its_arguments_is_the_plain_localizer(built):
    """A non-positive extent switches the policy off: the drive is bit-identical to a Localizer that never heard of it."""
    from fast_limo_amd import api
    n_scans, n_pts, speed = 12, 6000, 10.0
    st, w, a = synth.stationary_imu(0.0, 0.1 * n_scans + 0.06)
    A, B = api.Localizer(api.default_cfg(**CAPS)), api.Localizer(api.default_cfg(**CAPS))
    try:
        A.set_local_map(HALF, RECENTRE)
        A.set_local_map([HALF[0], 0.0, HALF[2]], RECENTRE)                # off again
        x0 = A.get_x(); x0[14] = speed
        A.set_x(x0); B.set_x(x0)
        i = 0
        for k in range(n_scans):
            until = 0.1 * (k + 1) + 0.005
            while i < len(st) and st[i] <= until:
                A.update_imu(st[i], w[i], a[i]); B.update_imu(st[i], w[i], a[i]); i += 1
            scan = synth.corridor_scan(k, n_pts, 77, speed=speed)
            assert A.update_pointcloud(scan, 0.1 * k) == B.update_pointcloud(scan, 0.1 * k)
            np.testing.assert_array_equal(A.get_x(), B.get_x())
        np.testing.assert_array_equal(A.hip.map_points(), B.hip.map_points())
        assert A.hip.map_crop_stats() == dict(crops=0, points_removed=0)
    finally:
        A.close(); B.close()
