"""GPU: flimo_radius_search (Octree::radiusSearch, reference Objects/Octree.hpp:453-523) through the C ABI.

"Brute force" is numpy over ctx.map_points() with the call's arithmetic (float32, dx*dx + (dy*dy + dz*dz), strict <).  Comparisons
are per query on index arrays sorted by index (unsorted mode) or as returned (sorted mode); distances are compared as bits, never
with a tolerance; every query of a test's input is in its comparison (test 10 states its sample)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from common import CAPS, cfg1_scene, drive_two_scans
from fast_limo_amd import synth
from radius_common import (RADII, PointIds, RadiusRef, bits, box_batches, brute_force, brute_force_multi, by_index, disagreeing_queries,
                           query_mix, sorted_order)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5


def _raw(ctx, q, radius, flags, off, idx, sqd, xyz, cap, total):
    """The C entry itself (arrays or None)."""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    p = lambda a: None if a is None else a.ctypes.data
    return ctx._L.flimo_radius_search(ctx._h, q.ctypes.data, q.size // 3, float(radius), int(flags), p(off), p(idx), p(sqd), p(xyz), int(cap),
                                      None if total is None else C.byref(total))


def _parity(ctx, q, radii, tag, sorted_too=False):
    """Every query of q at every radius against brute force over the map as it is stored: offsets, total, indices, distance bits,
    xyz.  Returns the number of results."""
    mp = ctx.map_points()
    n = 0
    for radius, (boff, bidx, bsqd) in zip(radii, brute_force_multi(q, mp, radii)):
        off, idx, sqd, xyz = ctx.radius_search(q, radius, want_xyz=True)
        assert off.dtype == np.uint64 and off[0] == 0 and off[-1] == len(idx) == len(sqd) == len(xyz), (tag, radius)
        np.testing.assert_array_equal(off, boff, err_msg=f"{tag}: offsets at radius {radius}")
        np.testing.assert_array_equal(xyz, mp[idx], err_msg=f"{tag}: xyz at radius {radius}")
        i2, s2 = by_index(off, idx, sqd)
        np.testing.assert_array_equal(i2, bidx, err_msg=f"{tag}: indices at radius {radius}")
        np.testing.assert_array_equal(bits(s2), bits(bsqd), err_msg=f"{tag}: distance bits at radius {radius}")
        np.testing.assert_array_equal(ctx.radius_count(q, radius), np.diff(boff).astype(np.int64))
        if sorted_too:
            soff, sidx, ssqd, sxyz = ctx.radius_search(q, radius, sorted=True, want_xyz=True)
            eidx, esqd = sorted_order(boff, bidx, bsqd)
            np.testing.assert_array_equal(soff, boff)
            np.testing.assert_array_equal(sidx, eidx, err_msg=f"{tag}: sorted indices at radius {radius}")
            np.testing.assert_array_equal(bits(ssqd), bits(esqd), err_msg=f"{tag}: sorted distance bits at radius {radius}")
            np.testing.assert_array_equal(sxyz, mp[sidx])
        n += int(boff[-1])
    return n


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scene(hip):
    """Box world at cfg1_scene's scale, fed in batches so that the insert rule drops points; the query mix of test_knn_bit_exact."""
    batches = box_batches(10, 6000)
    hip.map_clear(); hip.map_config()
    for b in batches:
        hip.map_add(b)
    mp = hip.map_points()
    assert 0 < mp.shape[0] == hip.map_size() < sum(b.shape[0] for b in batches)
    q = query_mix(mp, np.random.RandomState(5))
    return dict(batches=batches, mp=mp, q=q)


# 1
def test_radius_search_equals_brute_force(hip, scene):
    n = _parity(hip, scene["q"], RADII, "box world")
    print(f"box world: {scene['q'].shape[0]} queries x {len(RADII)} radii over {scene['mp'].shape[0]} points: {n} results")
    assert n > 100000
    # the walk examines at least what it returns, and not the whole map for a 1 m ball
    cand, cnt = hip.radius_candidates(scene["q"], 1.0), hip.radius_count(scene["q"], 1.0)
    assert np.all(cand.astype(np.int64) >= cnt) and cand.mean() < 0.05 * scene["mp"].shape[0]
    # the unsorted order is a function of the map's layout: two calls on an unchanged map agree element for element
    a, b = hip.radius_search(scene["q"], 1.0), hip.radius_search(scene["q"], 1.0)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


# 2
def test_sorted_output_is_brute_force_in_distance_then_index_order(hip, scene):
    q = scene["q"]
    for radius, (boff, bidx, bsqd) in zip(RADII, brute_force_multi(q, scene["mp"], RADII)):
        off, idx, sqd, xyz = hip.radius_search(q, radius, sorted=True, want_xyz=True)
        eidx, esqd = sorted_order(boff, bidx, bsqd)
        np.testing.assert_array_equal(off, boff)
        np.testing.assert_array_equal(idx, eidx)
        np.testing.assert_array_equal(bits(sqd), bits(esqd))
        np.testing.assert_array_equal(xyz, scene["mp"][idx])


# 3
def test_same_answer_as_the_references_traversal(hip, scene):
    ref = RadiusRef()
    for b in scene["batches"]:
        ref.update(b)
    assert ref.size() == hip.map_size()
    ids = PointIds(scene["mp"])
    q = scene["q"]
    results = shortcut = 0
    for radius in RADII:
        off, idx, sqd, xyz = hip.radius_search(q, radius, want_xyz=True)
        roff, rxyz, rsqd, sc = ref.radius_search(q, radius)
        assert disagreeing_queries(ids, off, xyz, sqd, roff, rxyz, rsqd) == 0, radius
        results += int(roff[-1]); shortcut += sc
    print(f"GPU vs the reference's traversal: {results} results, {shortcut} of them through the whole-octant shortcut")
    assert shortcut > 0


# 4
def test_the_bound_is_strict(built):
    from fast_limo_amd import _lib
    g = np.arange(7, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        ctx.map_add(lattice)                                  # ONE batch: the first build never down-samples
        mp = ctx.map_points()
        assert mp.shape[0] == 343
        q = np.float32([[3, 3, 3]])
        me = int(np.where(np.all(mp == q[0], axis=1))[0][0])
        off, idx, sqd = ctx.radius_search(q, np.float32(1.0))
        assert list(off) == [0, 1] and list(idx) == [me] and sqd[0] == 0.0      # the six neighbours lie at exactly 1: 1 < 1 is false
        up = np.nextafter(np.float32(1), np.float32(2))
        assert np.float32(up * up) == np.float32(1 + 2.0 ** -22)
        off, idx, sqd = ctx.radius_search(q, up, sorted=True)
        assert list(off) == [0, 7] and idx[0] == me and list(sqd) == [0.0] + [1.0] * 6
        assert sorted(np.abs(mp[idx[1:]] - q[0]).sum(1)) == [1.0] * 6 and list(idx[1:]) == sorted(idx[1:])
        off, idx, sqd = ctx.radius_search(q, 0.0)
        assert list(off) == [0, 0] and len(idx) == 0
        _parity(ctx, np.concatenate([q, lattice[::5], lattice[::7] + np.float32(0.5)]), (0.0, 0.5, 1.0, float(up), 2.0, 3.0), "lattice", sorted_too=True)
    finally:
        ctx.close()


# 5
def test_the_five_nearest_of_a_sorted_search_are_flimo_knns(hip, scene):
    q = scene["q"]
    off, idx, sqd = hip.radius_search(q, 3.0, sorted=True)
    kidx, ksqd, kcnt = hip.knn(q, 5)
    cnt = np.diff(off).astype(np.int64)
    sel = np.where(cnt >= 5)[0]
    assert len(sel) > 3000
    first5 = sqd[off[sel].astype(np.int64)[:, None] + np.arange(5)[None, :]]
    assert np.all(kcnt[sel] == 5)
    np.testing.assert_array_equal(bits(first5), bits(ksqd[sel]))      # (indices may differ on exact ties)


# 6
def test_capacity_protocol(hip, scene):
    q = scene["q"]
    radius = 1.0
    off, idx, sqd, xyz = hip.radius_search(q, radius, want_xyz=True)
    n = int(off[-1])
    assert n > 1000
    np.testing.assert_array_equal(hip.radius_count(q, radius), np.diff(off).astype(np.int64))
    # count only: offsets and total, nothing else
    coff = np.full(len(off), 99, np.uint64)
    total = C.c_uint64(0)
    assert _raw(hip, q, radius, 0, coff, None, None, None, 0, total) == 0
    np.testing.assert_array_equal(coff, off)
    assert total.value == n
    # one too small: FLIMO_ERR_TOO_LARGE, offsets / total right, the arrays untouched
    for flags in (0, 1):
        coff = np.full(len(off), 99, np.uint64)
        total = C.c_uint64(0)
        i1, s1, x1 = np.full(n, -7, np.int32), np.full(n, -7.0, np.float32), np.full((n, 3), -7.0, np.float32)
        assert _raw(hip, q, radius, flags, coff, i1, s1, x1, n - 1, total) == ERR_TOO_LARGE
        np.testing.assert_array_equal(coff, off)
        assert total.value == n
        assert np.all(i1 == -7) and np.all(s1 == -7.0) and np.all(x1 == -7.0)
        # exact room succeeds (a NULL total and a NULL xyz are fine)
        assert _raw(hip, q, radius, flags, coff, i1, s1, None, n, None) == 0
        if flags == 0:
            np.testing.assert_array_equal(i1, idx)
            np.testing.assert_array_equal(bits(s1), bits(sqd))
        assert np.all(x1 == -7.0)
    # only xyz asked for
    x2 = np.full((n, 3), -7.0, np.float32)
    assert _raw(hip, q, radius, 0, coff, None, None, x2, n, None) == 0
    np.testing.assert_array_equal(x2, xyz)


# 7
def test_edges(hip, scene):
    from fast_limo_amd import _lib
    mp = scene["mp"]
    off = np.full(4, 99, np.uint64)
    total = C.c_uint64(5)
    q3 = np.float32([mp[100] + np.float32(0.1), [np.nan, 0, 0], mp[200] - np.float32(0.1)])      # two near stored points, a NaN between
    # arguments
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        assert _raw(hip, q3, bad, 0, off, None, None, None, 0, total) == ERR_INVALID, bad
    assert _raw(hip, q3, 1.0, 2, off, None, None, None, 0, total) == ERR_INVALID               # unknown flag bits
    assert _raw(hip, q3, 1.0, 0, None, None, None, None, 0, total) == ERR_INVALID              # offsets are required
    assert hip._L.flimo_radius_search(hip._h, np.zeros(0, np.float32).ctypes.data, 0, 1.0, 0, off.ctypes.data, None, None, None, 0, C.byref(total)) == 0
    assert off[0] == 0 and total.value == 0                                                    # nq == 0
    # a NaN query among valid ones is empty; the others are not disturbed
    o, idx, sqd = hip.radius_search(q3, 2.0)
    bo, bidx, bsqd = brute_force(q3, mp, 2.0)
    np.testing.assert_array_equal(o, bo)
    assert o[2] == o[1] and o[1] > 0 and o[3] > o[2]
    np.testing.assert_array_equal(by_index(o, idx, sqd)[0], bidx)
    # a radius larger than the map's diameter: every query returns the whole map
    big = float(2.0 * np.linalg.norm(mp.max(0).astype(np.float64) - mp.min(0)) + 10.0)
    inside = np.float32([[0, 0, 1], mp[17], mp.max(0)])
    o, idx, sqd = hip.radius_search(inside, big)
    assert list(np.diff(o)) == [hip.map_size()] * 3
    for k in range(3):
        assert sorted(idx[int(o[k]):int(o[k + 1])]) == list(range(hip.map_size()))
    _parity(hip, inside, (big, 1.0e30), "larger than the map", sorted_too=True)
    # a far query whose ball reaches nothing; radius 0 on a stored point
    o, idx, sqd = hip.radius_search(np.float32([[900, 900, 0], [-4000, 12, 3]]), 100.0)
    assert list(o) == [0, 0, 0] and len(idx) == 0
    assert list(hip.radius_search(mp[:3], 0.0)[0]) == [0, 0, 0, 0]
    # an empty map: all offsets 0, FLIMO_OK
    c = _lib.HipCtx(0)
    try:
        o, idx, sqd = c.radius_search(q3, 5.0)
        assert list(o) == [0, 0, 0, 0] and len(idx) == 0
        assert list(c.radius_count(q3, 5.0)) == [0, 0, 0]
    finally:
        c.close()


# 8
def test_every_state_of_the_index(built):
    from fast_limo_amd import _lib
    rs = np.random.RandomState(8)
    radii = (0.05, 0.3, 1.0, 3.0, 10.0)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        mp0 = synth.box_world_map(30000, 25.0, 3)
        ctx.map_add(mp0)
        # the grid grows towards -x and +z: regrid, rows moved to the array's end
        for k in range(3):
            ctx.map_add(synth.box_world_map(4000, 20.0, 30 + k) + np.float32([-30.0 - 25.0 * k, 0.0, 12.0 + 15.0 * k]))
            ctx.map_add(synth.box_world_map(2000, 25.0, 40 + k))
        mm, merges, builds = ctx.grid_selfcheck()
        assert mm == 0, (mm, merges, builds)
        mp = ctx.map_points()
        q = np.concatenate([query_mix(mp, rs, 600, 100, 10, 20), mp[-200:] + rs.normal(0, 0.1, (200, 3)).astype(np.float32)])
        _parity(ctx, q, radii, "grown grid (%d merges, %d builds)" % (merges, builds), sorted_too=True)
        # after a crop: indices renumbered
        lo, hi = np.float32([-60, -15, -5]), np.float32([10, 30, 40])
        assert ctx.map_crop_box(lo, hi) > 1000
        assert ctx.grid_selfcheck()[0] == 0
        _parity(ctx, q, radii, "cropped")
        ctx.map_add(synth.box_world_map(3000, 25.0, 50))
        assert ctx.grid_selfcheck()[0] == 0
        _parity(ctx, q, (0.3, 3.0), "insert after the crop")
    finally:
        ctx.close()
    # escape columns: a dense cluster inserted without down-sampling, far more than 15 points per fine column
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(downsample=False)
        ctx.map_add(synth.box_world_map(20000, 25.0, 4))
        cluster = (rs.uniform(-0.15, 0.15, (6000, 3)) + [2.0, 3.0, 1.0]).astype(np.float32)
        ctx.map_add(cluster[:3000]); ctx.map_add(cluster[3000:])
        assert ctx.map_size() == 26000 and ctx.grid_selfcheck()[0] == 0
        q = np.concatenate([cluster[::40] + rs.normal(0, 0.05, (150, 3)).astype(np.float32), np.float32([[2, 3, 1], [2.4, 3, 1], [0, 0, 1]]),
                            query_mix(ctx.map_points(), rs, 200, 30, 5, 10)])
        n = _parity(ctx, q, (0.02, 0.05, 0.3, 1.0, 3.0), "escape columns", sorted_too=True)
        assert n > 500000
    finally:
        ctx.close()
    # the second level active (a copy of main-grid points: not consulted, results must not change)
    env = {"FLIMO_FINE": "1", "FLIMO_FINE_THRESHOLD": "32", "FLIMO_FINE_MIN_POINTS": "0"}
    os.environ.update(env)
    try:
        ctx = _lib.HipCtx(0)
    finally:
        for k in env:
            os.environ.pop(k)
    try:
        L = 40.0
        x = np.zeros(26); x[6] = 1; x[10] = 1; x[25] = -9.809; x[0:3] = synth.T_STAR_T
        ctx.map_config()
        ctx.map_add(synth.box_world_map(150000, L, 5))
        for j in range(6):
            ctx.scan_set(np.ascontiguousarray(synth.velodyne_scan(64, 1024, L, 40 + j)[:, :3]))
            ctx.map_add_scan(x, 0.1 * (j + 1))
        fs = ctx.fine_stats()
        assert fs["active"] and fs["points"] > 5000, fs
        assert ctx.grid_selfcheck()[0] == 0
        mp = ctx.map_points()
        under = mp[np.linalg.norm(mp - np.float32(synth.T_STAR_T), axis=1) < 4.0]
        q = np.concatenate([under[rs.choice(len(under), 200)] + rs.normal(0, 0.05, (200, 3)).astype(np.float32), query_mix(mp, rs, 200, 30, 5, 10, L)])
        _parity(ctx, q, (0.05, 0.3, 1.0, 3.0), "second level active", sorted_too=True)
    finally:
        ctx.close()


# 9
def test_two_places_six_kilometres_apart(built):
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
        assert ctx.grid_selfcheck()[0] == 0
        mp = ctx.map_points()
        mid = (rng.uniform(-100, 100, (4, 3)) + [3000.0, 3000.0, 0.0]).astype(np.float32)
        here = (rng.uniform(-25, 25, (4, 3)) * [1, 1, 0.1] + [0, 0, 2]).astype(np.float32)
        cases = (("100 m in the empty middle", mid, 100.0), ("4.5 km in the middle", mid, 4500.0), ("50 m at the first place", here, 50.0),
                 ("50 m at the second place", here + far, 50.0))
        for tag, q, radius in cases:
            ctx.radius_count(q, radius)                       # (warm)
            t0 = time.perf_counter()
            off, idx, sqd = ctx.radius_search(q, radius)
            ms = 1e3 * (time.perf_counter() - t0)
            print(f"two places 6 km apart, {tag}: {len(q)} queries, {int(off[-1])} results, {ms:.2f} ms (count + fill calls)")
            _parity(ctx, q, (radius,), tag, sorted_too=True)
            if tag.startswith("100 m"):
                assert off[-1] == 0
            if tag.startswith("4.5 km"):
                assert list(np.diff(off)) == [ctx.map_size()] * len(q)      # reaches both places
            if tag.startswith("50 m"):
                assert np.all(np.diff(off) > 10000)
    finally:
        ctx.close()


# 10
def test_a_million_points_65536_queries(built):
    from fast_limo_amd import _lib
    rs = np.random.RandomState(10)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        ctx.map_add(synth.box_world_map(1000000, 100.0, 1))
        mp = ctx.map_points()
        q = (mp[rs.choice(mp.shape[0], 65536)] + rs.normal(0, 0.3, (65536, 3))).astype(np.float32)
        sample = np.sort(np.random.RandomState(1024).choice(65536, 1024, replace=False))      # full parity: this seeded sample
        brute = brute_force_multi(q[sample], mp, (0.5, 2.0), chunk=16)
        for radius, (boff, bidx, bsqd) in zip((0.5, 2.0), brute):
            cnt = ctx.radius_count(q, radius)                 # (also the warm-up of the timed calls)
            t0 = time.perf_counter()
            off, idx, sqd = ctx.radius_search(q, radius)
            t1 = time.perf_counter()
            soff, sidx, ssqd = ctx.radius_search(q, radius, sorted=True)
            t2 = time.perf_counter()
            print(f"1M points, 65536 queries, radius {radius}: {int(off[-1])} results ({off[-1] / 65536.0:.1f} per query); "
                  f"count + fill {1e3 * (t1 - t0):.1f} ms, count + fill + sort {1e3 * (t2 - t1):.1f} ms (host clock, numpy allocation included)")
            # every query: counts equal the count-only call and sum to the total
            np.testing.assert_array_equal(np.diff(off).astype(np.int64), cnt)
            assert int(cnt.sum()) == int(off[-1]) == len(idx) == len(sqd)
            np.testing.assert_array_equal(soff, off)
            # the sample: full parity, both orders
            o64 = off.astype(np.int64)
            take = np.concatenate([np.arange(o64[s], o64[s + 1]) for s in sample]) if len(sample) else np.zeros(0, np.int64)
            np.testing.assert_array_equal(np.diff(boff).astype(np.int64), cnt[sample])
            i2, s2 = by_index(boff, idx[take], sqd[take])
            np.testing.assert_array_equal(i2, bidx)
            np.testing.assert_array_equal(bits(s2), bits(bsqd))
            eidx, esqd = sorted_order(boff, bidx, bsqd)
            np.testing.assert_array_equal(sidx[take], eidx)
            np.testing.assert_array_equal(bits(ssqd[take]), bits(esqd))
    finally:
        ctx.close()


# 11
def test_invisible_to_registration(built):
    from fast_limo_amd import _lib, api
    mp, scan, _ = cfg1_scene()
    imu = synth.stationary_imu(0.0, 0.45)
    rs = np.random.RandomState(4)
    q = (mp[rs.choice(mp.shape[0], 2000)] + rs.normal(0, 0.2, (2000, 3))).astype(np.float32)

    def drive(search):
        loc = api.Localizer(api.default_cfg(**CAPS))
        try:
            loc.set_async_insert(True)
            found = []
            rcs = drive_two_scans(loc, mp, scan, imu)
            if search:
                found.append(loc.map_radius_search(q, 1.0))                       # (an insert may still be running: the call waits)
            st, w, a = imu
            for i in np.where((st > 0.205) & (st <= 0.305))[0]:
                loc.update_imu(st[i], w[i], a[i])
            if search:
                found.append(loc.map_radius_search(q, 0.3, sorted=True, want_xyz=True))
            rcs.append(loc.update_pointcloud(scan, 0.2))
            if search:
                found.append(loc.map_radius_search(q, 2.0))
            loc.sync()
            return rcs, loc.get_x().copy(), loc.get_P().copy(), loc.hip.map_points().copy(), found
        finally:
            loc.close()

    rc0, x0, P0, m0, _ = drive(False)
    rc1, x1, P1, m1, found = drive(True)
    assert rc0 == rc1
    assert x0.tobytes() == x1.tobytes() and P0.tobytes() == P1.tobytes() and m0.tobytes() == m1.tobytes()
    assert all(int(f[0][-1]) > 1000 for f in found)
    # the last search saw the final map
    boff, bidx, bsqd = brute_force(q, m1, 2.0)
    np.testing.assert_array_equal(found[2][0], boff)
    np.testing.assert_array_equal(by_index(*found[2])[0], bidx)

    # a search issued while a pipelined pass is queued ahead of its pose leaves that pass's sums as they are
    scan3 = np.ascontiguousarray(scan[:, :3])
    cfg = _lib.default_match_cfg(**CAPS)
    xs = []
    for k in range(4):
        x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
        x[0] += 0.004 * k; x[1] -= 0.003 * k
        qq = x[3:7] + np.array([0.0, 0.0, 0.0008 * k, 0.0]); x[3:7] = qq / np.linalg.norm(qq)
        xs.append(x)

    def passes(search):
        h = _lib.HipCtx(0)
        try:
            h.set_update_mode(1)
            h.map_add(np.ascontiguousarray(mp[:, :3]))
            h.scan_set(scan3)
            h.set_pass_pipeline(True)
            out = []
            for k, xk in enumerate(xs):
                out.append(h.match_reduce(xk, cfg))
                if search and k < len(xs) - 1:
                    off, idx, sqd = h.radius_search(q, 0.5, sorted=bool(k & 1))
                    assert off[-1] > 1000
            h.pass_pipeline_end()
            return out, h.pass_pipeline_stats()
        finally:
            h.close()

    plain, st0 = passes(False)
    with_search, st1 = passes(True)
    print("pipeline counters without / with radius searches between the passes:", st0, st1)
    for k, (a, b) in enumerate(zip(plain, with_search)):
        assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), k
    assert plain[0][2] > 1000
