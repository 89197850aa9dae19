"""GPU: flimo_knn_k (Octree::knn for any k up to 64, with a distance gate; reference Objects/Octree.hpp:526-555) through the C ABI.

"Brute force" is numpy over ctx.map_points() with the call's arithmetic (float32, dx*dx + (dy*dy + dz*dz)) in the call's unique
order: ascending by (squared-distance bits, insertion index).  idx, the bits of sqd, and cnt are compared with no tolerance, on
every query of a test's input."""
import os
import time

import numpy as np
import pytest

from common import CAPS, cfg1_scene, drive_two_scans
from fast_limo_amd import synth
from knn_k_common import brute_knn
from radius_common import bits, box_batches, query_mix

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -5, -6
INF = float("inf")
KS = (1, 2, 5, 6, 8, 13, 16, 17, 32, 33, 64)


def _raw(ctx, q, k, max_dist, idx, sqd, xyz, cnt):
    """The C entry itself (arrays or None)."""
    q = None if q is None else np.ascontiguousarray(q, np.float32).reshape(-1)
    p = lambda a: None if a is None else a.ctypes.data
    return ctx._L.flimo_knn_k(ctx._h, p(q), 0 if q is None else q.size // 3, int(k), float(max_dist), p(idx), p(sqd), p(xyz), p(cnt))


def _check(ctx, q, k, max_dist=INF, tag="", mp=None, chunk=64):
    """Every query of q against the brute force over the map as it is stored: idx, distance bits, cnt, xyz, padding."""
    mp = ctx.map_points() if mp is None else mp
    idx, sqd, cnt, xyz = ctx.knn_k(q, k, max_dist, want_xyz=True)
    bidx, bsqd, bcnt = brute_knn(q, mp, k, max_dist, chunk=chunk)
    msg = f"{tag}: k = {k}, max_dist = {max_dist}"
    np.testing.assert_array_equal(cnt, bcnt, err_msg=msg + " (cnt)")
    np.testing.assert_array_equal(bits(sqd), bits(bsqd), err_msg=msg + " (distance bits)")
    np.testing.assert_array_equal(idx, bidx, err_msg=msg + " (idx)")
    pad = idx < 0
    assert np.all(pad == (np.arange(k)[None, :] >= cnt[:, None])), msg
    if mp.shape[0]:
        np.testing.assert_array_equal(xyz[~pad], mp[idx[~pad]], err_msg=msg + " (xyz)")
    assert np.all(xyz[pad] == 0) and np.all(sqd[pad] == 0), msg
    return idx, sqd, cnt


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scene(hip):
    """Box world fed in batches so that the insert rule drops points; the query mix of test_knn_bit_exact."""
    batches = box_batches(10, 6000)
    hip.map_clear(); hip.map_config()
    for b in batches:
        hip.map_add(b)
    mp = hip.map_points()
    assert 0 < mp.shape[0] == hip.map_size() < sum(b.shape[0] for b in batches)
    q = query_mix(mp, np.random.RandomState(5))
    return dict(batches=batches, mp=mp, q=q)


# 1
def test_knn_k_equals_brute_force_and_the_oracle_octree(hip, scene, oracle):
    oc = oracle.Octree()
    for b in scene["batches"]:
        oc.update(b)
    assert oc.size() == hip.map_size()
    q = scene["q"]
    for k in KS:
        idx, sqd, cnt = _check(hip, q, k, INF, "box world", scene["mp"])
        assert np.all(cnt == k)
        _, osqd, ocnt, _ = oc.knn(q, k, num_threads=8)
        assert np.all(ocnt == k)
        np.testing.assert_array_equal(bits(sqd), bits(osqd), err_msg=f"oracle octree, k = {k}")
    cand = hip.knn_k_candidates(q[:3000], 16)
    print(f"box world: {q.shape[0]} queries over {scene['mp'].shape[0]} points; k = 16 examines {cand.mean():.0f} stored points per near query")
    assert np.all(cand >= 16) and cand.mean() < 0.05 * scene["mp"].shape[0]


# 2
def test_exact_ties_follow_the_unique_order(built):
    from fast_limo_amd import _lib
    rs = np.random.RandomState(2)
    g = (np.arange(20, dtype=np.float32) * np.float32(0.25))
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[rs.permutation(lattice.shape[0])]
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        for a in range(0, lattice.shape[0], 1000):
            ctx.map_add(lattice[a:a + 1000])
        mp = ctx.map_points()
        assert mp.shape[0] > 1000
        q = np.concatenate([mp[::9], mp[::11] + np.float32(0.125)]).astype(np.float32)
        for k in (6, 8, 16, 33, 64):
            bidx, bsqd, bcnt = brute_knn(q, mp, k, extra=1)
            tied = bits(bsqd[:, k - 1]) == bits(bsqd[:, k])
            print(f"lattice, k = {k}: {tied.mean():.2f} of {q.shape[0]} queries have the k-th and (k+1)-th distance bit-equal")
            assert np.all(bidx[:, k] >= 0) and tied.mean() >= 0.5
            _check(ctx, q, k, INF, "lattice", mp)
    finally:
        ctx.close()


# 3
def test_agrees_with_flimo_knn_for_k_up_to_5(hip, scene):
    q, mp = scene["q"], scene["mp"]
    for k in (1, 2, 3, 4, 5):
        idx, sqd, cnt = hip.knn_k(q, k)
        kidx, ksqd, kcnt = hip.knn(q, k)
        np.testing.assert_array_equal(cnt, kcnt)
        np.testing.assert_array_equal(bits(sqd), bits(ksqd))
        _, bsqd, _ = brute_knn(q, mp, k, extra=1)
        distinct = np.all(np.diff(bits(bsqd).astype(np.int64), axis=1) > 0, axis=1)      # the first k + 1 distances pairwise different
        assert (~distinct).mean() <= 0.01, (k, (~distinct).sum())
        np.testing.assert_array_equal(idx[distinct], kidx[distinct])


# 4
def test_gate_is_the_first_k_of_a_sorted_radius_search(hip, scene):
    q, mp = scene["q"], scene["mp"]
    for max_dist in (0.0, 0.05, 0.3, 1.0, 3.0):
        off, ridx, rsqd = hip.radius_search(q, max_dist, sorted=True)
        o64 = off.astype(np.int64)
        n = np.diff(o64)
        for k in (4, 16, 64):
            idx, sqd, cnt = _check(hip, q, k, max_dist, "gate", mp)
            np.testing.assert_array_equal(cnt, np.minimum(n, k))
            col = np.arange(k)[None, :]
            take = col < cnt[:, None]
            at = (o64[:-1, None] + col)[take]
            np.testing.assert_array_equal(idx[take], ridx[at])
            np.testing.assert_array_equal(bits(sqd[take]), bits(rsqd[at]))
            assert np.all(idx[~take] == -1) and np.all(sqd[~take] == 0)
        if max_dist == 0.0:
            assert np.all(n == 0)
    for k in (4, 16, 64):
        a, b = hip.knn_k(q, k, INF), hip.knn_k(q, k)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
        _check(hip, q, k, INF, "no gate", mp)
        # a gate beyond every distance admits everything
        c = hip.knn_k(q, k, 1.0e4)
        np.testing.assert_array_equal(c[0], a[0])


# 5
def test_edges(hip, scene):
    from fast_limo_amd import _lib
    mp = scene["mp"]
    q3 = np.float32([mp[100] + np.float32(0.1), [np.nan, 0, 0], mp[200] - np.float32(0.1)])
    k = 8
    idx, sqd, cnt = np.full((3, k), -7, np.int32), np.full((3, k), -7, np.float32), np.full(3, -7, np.int32)
    # arguments
    assert _raw(hip, q3, 0, INF, idx, sqd, None, cnt) == ERR_UNSUPPORTED
    assert _raw(hip, q3, 65, INF, idx, sqd, None, cnt) == ERR_UNSUPPORTED
    assert _raw(hip, q3, -1, INF, idx, sqd, None, cnt) == ERR_UNSUPPORTED
    for bad in (np.nan, -1.0, -np.inf):
        assert _raw(hip, q3, k, bad, idx, sqd, None, cnt) == ERR_INVALID, bad
    assert _raw(hip, q3, k, INF, None, sqd, None, cnt) == ERR_INVALID
    assert _raw(hip, q3, k, INF, idx, None, None, cnt) == ERR_INVALID
    assert _raw(hip, q3, k, INF, idx, sqd, None, None) == ERR_INVALID
    assert hip._L.flimo_knn_k(hip._h, None, 3, k, INF, idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data) == ERR_INVALID
    assert np.all(idx == -7) and np.all(sqd == -7) and np.all(cnt == -7)
    assert hip._L.flimo_knn_k(hip._h, None, 0, k, INF, idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data) == 0      # nq == 0
    assert np.all(idx == -7) and np.all(cnt == -7)
    i0, s0, c0 = hip.knn_k(np.zeros((0, 3), np.float32), k)
    assert i0.shape == (0, k) and c0.shape == (0,)
    # a NaN query among valid ones is empty; the others are not disturbed
    i, s, c = _check(hip, q3, k, INF, "NaN query", mp)
    assert list(c) == [k, 0, k] and np.all(i[1] == -1)
    i, s, c = _check(hip, q3, 64, 0.5, "NaN query, gate", mp)
    assert c[1] == 0 and c[0] > 0 and c[2] > 0
    # an empty map: all cnt 0, FLIMO_OK
    ctx = _lib.HipCtx(0)
    try:
        i, s, c, x = ctx.knn_k(q3, k, want_xyz=True)
        assert np.all(c == 0) and np.all(i == -1) and np.all(s == 0) and np.all(x == 0)
        # three points, k = 64; from anywhere: 40 km and 2 000 km away (test_knn_small_k_and_empty_map)
        pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 1, 1], [0, 1, 0]], np.float32)
        ctx.map_add(pts)
        assert ctx.map_size() == 3
        far = np.array([[0.1, 0, 0], [40000.0, -3.0, 2.0], [2.0e6, 2.0e6, -1.0e6], [np.nan, 0, 0], [-7.5, 0.2, 0.1]], np.float32)
        for kk in (1, 2, 3, 5, 16, 17, 64):
            i, s, c = _check(ctx, far, kk, INF, "three points")
            assert list(c) == [min(kk, 3)] * 3 + [0, min(kk, 3)]
        i, s, c = _check(ctx, far, 64, 1.0, "three points, 1 m gate")
        assert list(c) == [2, 0, 0, 0, 0]
        i, s, c = _check(ctx, far, 64, 1.0e5, "three points, 100 km gate")
        assert list(c) == [3, 3, 0, 0, 3]
    finally:
        ctx.close()


# 6
def test_a_map_that_changes(built):
    from fast_limo_amd import _lib
    rs = np.random.RandomState(8)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        ctx.map_add(synth.box_world_map(30000, 25.0, 3))
        # inserts that move rows to the array's end; the grid grows towards -x and +z (index_regrid)
        for j in range(3):
            ctx.map_add(synth.box_world_map(4000, 20.0, 30 + j) + np.float32([-30.0 - 25.0 * j, 0.0, 12.0 + 15.0 * j]))
            ctx.map_add(synth.box_world_map(2000, 25.0, 40 + j))
        mm, merges, builds = ctx.grid_selfcheck()
        assert mm == 0, (mm, merges, builds)
        mp = ctx.map_points()
        q = np.concatenate([query_mix(mp, rs, 600, 100, 10, 20), mp[-200:] + rs.normal(0, 0.1, (200, 3)).astype(np.float32)])
        for k in (8, 16, 64):
            _check(ctx, q, k, INF, "grown grid (%d merges, %d builds)" % (merges, builds), mp)
        _check(ctx, q, 33, 1.0, "grown grid, gate", mp)
        # after a crop: indices renumbered
        assert ctx.map_crop_box(np.float32([-60, -15, -5]), np.float32([10, 30, 40])) > 1000
        assert ctx.grid_selfcheck()[0] == 0
        for k in (16, 64):
            _check(ctx, q, k, INF, "cropped")
        ctx.map_add(synth.box_world_map(3000, 25.0, 50))
        _check(ctx, q, 64, INF, "insert after the crop")
        _check(ctx, q, 16, 3.0, "insert after the crop, gate")
        # cleared and filled again
        ctx.map_clear()
        assert np.all(ctx.knn_k(q[:10], 16)[2] == 0)
        ctx.map_config()
        ctx.map_add(synth.box_world_map(20000, 25.0, 60))
        ctx.map_add(synth.box_world_map(3000, 25.0, 61))
        for k in (16, 64):
            _check(ctx, q, k, INF, "cleared and filled again")
    finally:
        ctx.close()


# 7
def test_two_places_six_kilometres_apart_at_bounded_cost(built):
    from fast_limo_amd import _lib
    rng = np.random.default_rng(3)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config()
        far = np.float32([6000.0, 6000.0, 0.0])
        a, b = synth.box_world_map(60000, 30.0, 11), synth.box_world_map(60000, 30.0, 12) + far
        ctx.map_add(np.concatenate([a, b]))
        for j in range(4):
            ctx.map_add(synth.box_world_map(3000, 20.0, 20 + j) + (far if j % 2 else np.float32([0, 0, 0])))
        assert ctx.grid_selfcheck()[0] == 0
        mp = ctx.map_points()
        mid = (rng.uniform(-100, 100, (40, 3)) + [3000.0, 3000.0, 0.0]).astype(np.float32)          # the empty middle
        outside = (rng.uniform(-100, 100, (40, 3)) + [-9000.0, 2000.0, 50.0]).astype(np.float32)    # kilometres outside
        beside = (rng.uniform(-1, 1, (20, 3)) * [200, 200, 5] + [0, 0, 2]).astype(np.float32)       # around the first place
        q = np.concatenate([mid, outside, beside, beside + far]).astype(np.float32)
        _check(ctx, q, 64, INF, "two places", mp, chunk=8)
        _check(ctx, q, 64, 4300.0, "two places, 4.3 km gate", mp, chunk=8)
        i, s, c = ctx.knn_k(mid, 64, 100.0)
        assert np.all(c == 0)
        # cost guard: flimo_knn (k = 5) on the same queries and map is the scale; ring after ring of empty cells would be a
        # thousand-fold and more
        t5, t64 = [], []
        ctx.knn(q, 5); ctx.knn_k(q, 64)
        for _ in range(5):
            t0 = time.perf_counter(); ctx.knn(q, 5); t1 = time.perf_counter(); ctx.knn_k(q, 64); t2 = time.perf_counter()
            t5.append(1e3 * (t1 - t0)); t64.append(1e3 * (t2 - t1))
        m5, m64 = float(np.median(t5)), float(np.median(t64))
        cand = ctx.knn_k_candidates(q, 64)
        print(f"two places 6 km apart, {q.shape[0]} queries: flimo_knn k = 5 {m5:.2f} ms, flimo_knn_k k = 64 {m64:.2f} ms "
              f"(ratio {m64 / m5:.2f}); {cand.mean():.0f} stored points examined per query")
        assert m64 <= 20.0 * m5
    finally:
        ctx.close()


# 8
def test_crowded_cells(built):
    from fast_limo_amd import _lib
    rs = np.random.RandomState(8)
    # escape columns: a dense cluster inserted without down-sampling, far more than 15 points per fine column
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(downsample=False)
        ctx.map_add(synth.box_world_map(20000, 25.0, 4))
        cluster = (rs.uniform(-0.15, 0.15, (6000, 3)) + [2.0, 3.0, 1.0]).astype(np.float32)
        ctx.map_add(cluster[:3000]); ctx.map_add(cluster[3000:])
        assert ctx.map_size() == 26000 and ctx.grid_selfcheck()[0] == 0
        mp = ctx.map_points()
        q = np.concatenate([cluster[::40] + rs.normal(0, 0.05, (150, 3)).astype(np.float32), np.float32([[2, 3, 1], [2.4, 3, 1], [0, 0, 1]]),
                            query_mix(mp, rs, 200, 30, 5, 10)])
        _check(ctx, q, 64, INF, "escape columns", mp)
        _check(ctx, q, 16, INF, "escape columns", mp)
        _check(ctx, q, 64, 0.05, "escape columns, gate", mp)
    finally:
        ctx.close()
    # a map crowded by raw sweeps under the sensor, the second level active
    env = {"FLIMO_FINE": "1", "FLIMO_FINE_THRESHOLD": "32", "FLIMO_FINE_MIN_POINTS": "0"}
    os.environ.update(env)
    try:
        ctx = _lib.HipCtx(0)
    finally:
        for name in env:
            os.environ.pop(name)
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
        _check(ctx, q, 64, INF, "second level active", mp, chunk=16)
        _check(ctx, q, 13, INF, "second level active", mp, chunk=16)
    finally:
        ctx.close()


# 9
def test_a_million_points_65536_queries(built, oracle):
    from fast_limo_amd import _lib
    rs = np.random.RandomState(10)
    ctx = _lib.HipCtx(0)
    try:
        mp = synth.box_world_map(1000000, 100.0, 1)
        ctx.map_config()
        ctx.map_add(mp)
        oc = oracle.Octree(); oc.update(mp)
        assert oc.size() == ctx.map_size()
        stored = ctx.map_points()
        q = (stored[rs.choice(stored.shape[0], 65536)] + rs.normal(0, 0.3, (65536, 3))).astype(np.float32)
        ctx.knn_k(q, 16)                                   # (warm)
        t0 = time.perf_counter()
        idx, sqd, cnt = ctx.knn_k(q, 16)
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"1M points, 65536 queries, k = 16: {ms:.1f} ms (host clock, numpy allocation included)")
        assert np.all(cnt == 16)
        _, osqd, ocnt, _ = oc.knn(q, 16, num_threads=16)
        assert np.all(ocnt == 16)
        np.testing.assert_array_equal(bits(sqd), bits(osqd))
        # the indices name the points at those distances
        d = ((q[:, None, :] - stored[idx]) ** 2)
        np.testing.assert_array_equal(bits(d[..., 0] + (d[..., 1] + d[..., 2])), bits(sqd))
    finally:
        ctx.close()


# 10
def test_through_the_localizer_and_invisible_to_registration(built):
    from fast_limo_amd import _lib, api
    mp, scan, _ = cfg1_scene()
    imu = synth.stationary_imu(0.0, 0.45)
    rs = np.random.RandomState(4)
    q = (mp[rs.choice(mp.shape[0], 2000)] + rs.normal(0, 0.2, (2000, 3))).astype(np.float32)
    # no map yet: all cnt 0
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        i, s, c = loc.map_knn(q[:5], 16)
        assert np.all(c == 0) and np.all(i == -1) and np.all(s == 0)
    finally:
        loc.close()

    def drive(search):
        loc = api.Localizer(api.default_cfg(**CAPS))
        try:
            loc.set_async_insert(True)
            found = []
            rcs = drive_two_scans(loc, mp, scan, imu)
            if search:
                found.append(loc.map_knn(q, 16))                                  # (an insert may still be running: the call waits)
            st, w, a = imu
            for i in np.where((st > 0.205) & (st <= 0.305))[0]:
                loc.update_imu(st[i], w[i], a[i])
            if search:
                found.append(loc.map_knn(q, 64, 1.0, want_xyz=True))
            rcs.append(loc.update_pointcloud(scan, 0.2))
            if search:
                found.append(loc.map_knn(q, 33))                                  # right after a sweep whose insert is still running
                loc.sync()
                found.append(loc.hip.knn_k(q, 33))                                # the quiescent context
            loc.sync()
            return rcs, loc.get_x().copy(), loc.get_P().copy(), loc.hip.map_points().copy(), found
        finally:
            loc.close()

    rc0, x0, P0, m0, _ = drive(False)
    rc1, x1, P1, m1, found = drive(True)
    assert rc0 == rc1
    assert x0.tobytes() == x1.tobytes() and P0.tobytes() == P1.tobytes() and m0.tobytes() == m1.tobytes()
    assert np.all(found[0][2] == 16) and found[1][2].max() > 0
    for u, v in zip(found[2], found[3]):
        np.testing.assert_array_equal(u, v)
    bidx, bsqd, bcnt = brute_knn(q, m1, 33)
    np.testing.assert_array_equal(found[2][0], bidx)
    np.testing.assert_array_equal(bits(found[2][1]), bits(bsqd))

    # a registration pass run before and after a knn_k call gives the same bits; so do pipelined passes with calls between them
    scan3 = np.ascontiguousarray(scan[:, :3])
    cfg = _lib.default_match_cfg(**CAPS)
    xs = []
    for j in range(4):
        x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
        x[0] += 0.004 * j; x[1] -= 0.003 * j
        qq = x[3:7] + np.array([0.0, 0.0, 0.0008 * j, 0.0]); x[3:7] = qq / np.linalg.norm(qq)
        xs.append(x)

    def passes(search):
        h = _lib.HipCtx(0)
        try:
            h.set_update_mode(1)
            h.map_add(np.ascontiguousarray(mp[:, :3]))
            h.scan_set(scan3)
            h.set_pass_pipeline(True)
            out = []
            for j, xj in enumerate(xs):
                out.append(h.match_reduce(xj, cfg))
                if search and j < len(xs) - 1:
                    i, s, c = h.knn_k(q, (16, 64, 5)[j], INF if j & 1 else 2.0)
                    assert c.sum() > 1000
            h.pass_pipeline_end()
            return out
        finally:
            h.close()

    plain, with_search = passes(False), passes(True)
    for j, (a, b) in enumerate(zip(plain, with_search)):
        assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), j
    assert plain[0][2] > 1000


# 11
def test_a_worklist_longer_than_the_walks_grid(built):
    """20 001 queries of which 18 000 lie 50 - 500 m outside a 2 m box of about 300 points: every one of those is left to the walk
    over the tiles, more entries than its 4096 x 4 waves, so its grid stride runs; near queries and a NaN one lie between them,
    and 20 001 is a multiple of neither 4 nor 16.  Every query is compared; the candidate counter is a function of the query alone."""
    from fast_limo_amd import _lib
    rs = np.random.RandomState(21)
    centre = np.float32([10.0, -5.0, 3.0])
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(downsample=False)
        ctx.map_add((rs.uniform(-1.0, 1.0, (300, 3)) + centre).astype(np.float32))
        mp = ctx.map_points()
        assert mp.shape[0] == 300
        nq = 20001
        d = rs.normal(0, 1, (nq, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        q = (centre + d * rs.uniform(50.0, 500.0, (nq, 1))).astype(np.float32)
        near = np.arange(0, nq, 10)                                               # every tenth query lies inside the box
        q[near] = (rs.uniform(-1.0, 1.0, (near.size, 3)) + centre).astype(np.float32)
        nan_at = int(near[near.size // 2])
        q[nan_at] = np.float32([np.nan, 0.0, 0.0])
        far = np.setdiff1d(np.arange(nq), near)
        assert far.size == 18000 > 4096 * 4 and nq % 4 and nq % 16
        dist = np.linalg.norm(q.astype(np.float64) - centre, axis=1)
        assert dist[far].min() > 49.0 and np.nanmax(dist[near]) < 1.8
        chosen = np.concatenate([far[:21], far[-21:], near[:10], near[-11:], [nan_at]])
        assert chosen.size == 64
        for max_dist in (INF, 0.6, 120.0):                                        # 0.6 m cuts near lists short, 120 m the far ones
            bidx, bsqd, bcnt = brute_knn(q, mp, 64, max_dist, chunk=2048)         # the k-list is the first k of the 64-list
            if max_dist == 0.6:
                assert np.any((bcnt[near] > 0) & (bcnt[near] < 16)) and 17 < bcnt[near].max() < 64 and np.all(bcnt[far] == 0)
            elif max_dist == 120.0:
                assert np.any(bcnt[far] == 0) and np.any((bcnt[far] > 0) & (bcnt[far] < 64)) and np.any(bcnt[far] == 64)
            else:
                assert np.all(np.delete(bcnt, nan_at) == 64)
            assert bcnt[nan_at] == 0
            for k in (3, 16, 17, 64):
                msg = f"worklist: k = {k}, max_dist = {max_dist}"
                idx, sqd, cnt, xyz = ctx.knn_k(q, k, max_dist, want_xyz=True)
                np.testing.assert_array_equal(cnt, np.minimum(bcnt, k), err_msg=msg + " (cnt)")
                np.testing.assert_array_equal(bits(sqd), bits(bsqd[:, :k]), err_msg=msg + " (distance bits)")
                np.testing.assert_array_equal(idx, bidx[:, :k], err_msg=msg + " (idx)")
                pad = idx < 0
                assert np.all(pad == (np.arange(k)[None, :] >= cnt[:, None])), msg
                np.testing.assert_array_equal(xyz[~pad], mp[idx[~pad]], err_msg=msg + " (xyz)")
                assert np.all(xyz[pad] == 0) and np.all(sqd[pad] == 0), msg
                cand = ctx.knn_k_candidates(q, k, max_dist)
                np.testing.assert_array_equal(ctx.knn_k_candidates(q, k, max_dist), cand, err_msg=msg + " (cand, second call)")
                alone = np.concatenate([ctx.knn_k_candidates(q[i:i + 1], k, max_dist) for i in chosen])
                np.testing.assert_array_equal(cand[chosen], alone, err_msg=msg + " (cand, each query alone)")
                assert np.all(cand >= cnt.astype(np.uint64)), msg
    finally:
        ctx.close()
