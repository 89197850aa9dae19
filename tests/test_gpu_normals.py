"""GPU: flimo_map_normals / flimo_map_normals_range (plane normal, curvature, centroid, covariance and eigen-decomposition of the
k-NN neighbourhoods of the resident map) through the C ABI.

The yardstick and the bounds -- derived, not measured -- are tests/normals_common.py: brute-force neighbourhoods over
ctx.map_points(), moments summed with math.fsum, numpy.linalg.eigh.  Wherever two calls must give the same result the arrays are
compared byte for byte."""
import numpy as np
import pytest

import normals_common as nc
from common import CAPS, cfg1_scene, drive_two_scans
from fast_limo_amd import synth
from radius_common import box_batches

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -5, -6
INF = float("inf")
NAMES = ("normal", "cnt", "centroid", "cov", "eig")


def same_bytes(a, b, tag=""):
    for name in NAMES:
        assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), f"{tag}: {name} differs"


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    yield ctx
    ctx.close()


def fresh_map(batches, cell_size=0.0, downsample=True):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(cell_size=cell_size, downsample=downsample)
    for b in batches:
        ctx.map_add(b)
    return ctx


@pytest.fixture(scope="module")
def scene(hip, oracle):
    """12 000 stored points fed in four batches; 550 queries (normals_common.scene_queries: those of the CPU cap test): near the
    surfaces, in the air, 500 m away (the walk over the tiles), on map points.  The yardstick of a (k, gate) is computed once."""
    hip.map_clear(); hip.map_config()
    for b in nc.scene_batches():
        hip.map_add(b)
    mp = hip.map_points()
    assert mp.shape[0] == hip.map_size() == 12000 and np.array_equal(mp, nc.scene_map())      # (the CPU cap test's inputs)
    q = nc.scene_queries(oracle)
    refs = {}

    def ref(k, gate=INF, min_pts=3, viewpoint=None):
        key = (k, gate, min_pts, None if viewpoint is None else tuple(viewpoint))
        if key not in refs:
            refs[key] = nc.reference(q, mp, k, gate, min_pts, viewpoint)
        return refs[key]
    return dict(mp=mp, q=q, ref=ref)


# 1
@pytest.mark.parametrize("k,gate", nc.SCENE_KS)
def test_against_the_yardstick(hip, scene, k, gate):
    q = scene["q"]
    got = hip.normals(q, k, gate)
    ref = scene["ref"](k, gate)
    nc.check(got, ref, f"k = {k}, gate {gate}")
    # the neighbourhood is flimo_knn_k's
    np.testing.assert_array_equal(got["cnt"], hip.knn_k(q, k, gate)[2])
    if np.isinf(gate):
        assert np.all(got["cnt"] == k)
    else:
        assert (got["cnt"] < 3).sum() > 0 and np.all(np.isnan(got["normal"][got["cnt"] < 3]))
    # the outputs asked for do not change the others
    only = hip.normals(q, k, gate, want=())
    assert set(only) == {"normal", "cnt"}
    assert only["normal"].tobytes() == got["normal"].tobytes() and only["cnt"].tobytes() == got["cnt"].tobytes()


# 2
def test_the_result_depends_on_the_neighbour_list_alone(hip, scene):
    q = scene["q"]
    vp = np.float32([1.0, -2.0, 3.0])
    maps = [fresh_map(nc.scene_batches(), cell) for cell in (0.25, 0.5, 2.0)]
    try:
        for m in maps:
            assert np.array_equal(m.map_points(), scene["mp"])
        for k, gate, view in ((5, INF, None), (16, INF, vp), (20, INF, None), (64, 2.0, vp)):
            outs = [m.normals(q, k, gate, viewpoint=view) for m in maps]
            for o in outs[1:]:
                same_bytes(outs[0], o, f"cell size, k = {k}")
            same_bytes(outs[0], hip.normals(q, k, gate, viewpoint=view), f"default cell size, k = {k}")
            assert np.all(outs[0]["cnt"][500:520] == (k if np.isinf(gate) else 0))      # (the queries 500 m away)
            # chunks of 128 queries against one chunk
            maps[0].set_normals_chunk(128)
            same_bytes(outs[0], maps[0].normals(q, k, gate, viewpoint=view), f"chunks of 128, k = {k}")
            same_bytes(maps[0].normals_range(100, 1000, k, gate, viewpoint=view), maps[1].normals_range(100, 1000, k, gate, viewpoint=view), "range, chunks")
            maps[0].set_normals_chunk(0)
    finally:
        for m in maps:
            m.close()


# 3
def test_range_form(built):
    ctx = fresh_map(box_batches(3, 3000))
    try:
        def both(tag):
            mp = ctx.map_points()
            n = mp.shape[0]
            for first, cnt, k, gate in ((n // 3, n // 4, 20, INF), (0, n, 16, INF), (n - 50, 50, 33, 0.6)):
                a = ctx.normals_range(first, cnt, k, gate)
                same_bytes(a, ctx.normals(mp[first:first + cnt], k, gate), f"{tag}: [{first}, +{cnt}), k = {k}")
                assert np.all(a["cnt"] >= 1)                     # a stored point is its own first neighbour
            return n
        n0 = both("three batches")
        ctx.map_add(synth.box_world_map(2000, 25.0, 77))
        n1 = both("one more insert")
        assert n1 > n0
        assert ctx.map_crop_box(np.float32([-30, -10, -5]), np.float32([12, 30, 30])) > 500      # indices are renumbered
        assert both("after a crop") < n1
        # beyond the map
        n = ctx.map_size()
        out = [np.full((4, 4), -7, np.float32), np.full(4, -7, np.int32)]
        for first, cnt in ((n, 1), (n - 3, 4), (n + 1, 0), (2 ** 40, 4)):
            assert ctx._L.flimo_map_normals_range(ctx._h, first, cnt, 8, INF, 3, None, out[0].ctypes.data, out[1].ctypes.data, None, None, None) == ERR_INVALID
        assert np.all(out[0] == -7) and np.all(out[1] == -7)
        assert ctx.normals_range(n, 0, 8)["cnt"].shape == (0,)
    finally:
        ctx.close()


# 4
def test_analytic_plane_sphere_and_sign_rule(hip, scene):
    pts, nrm = nc.tilted_plane()
    ctx = fresh_map([pts], downsample=False)
    try:
        assert ctx.map_size() == pts.shape[0]
        q = np.concatenate([pts[::5], (pts[3::11].astype(np.float64) + nrm * 0.25).astype(np.float32)])
        above = np.float32([1.0, 1.0, 100.0])
        for k in (9, 16, 20, 64):
            got = ctx.normals(q, k, viewpoint=above)
            assert np.all(got["cnt"] == k)
            e = np.abs(got["normal"][:, :3].astype(np.float64) - nrm[None, :]).max()
            print(f"plane, k = {k}: normal off by {e / nc.F32:.3f} x 2^-23, curvature up to {got['normal'][:, 3].max():.3g}")
            assert e <= nc.F32 and np.abs(got["normal"][:, 3]).max() <= nc.F32
            below = ctx.normals(q, k, viewpoint=np.float32([1.0, 1.0, -100.0]))
            assert np.abs(below["normal"][:, :3].astype(np.float64) + nrm[None, :]).max() <= nc.F32
            free = ctx.normals(q, k)                              # no viewpoint: the largest component (z) is positive
            assert np.abs(free["normal"][:, :3].astype(np.float64) - nrm[None, :]).max() <= nc.F32
    finally:
        ctx.close()
    # a sphere shell seen from its centre
    rs = np.random.RandomState(12)
    d = rs.normal(0, 1, (6000, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    centre = np.float32([3.0, -2.0, 1.5])
    shell = (centre.astype(np.float64) + 4.0 * d).astype(np.float32)
    ctx = fresh_map([shell], downsample=False)
    try:
        q = shell[::6]
        got = ctx.normals(q, 20, viewpoint=centre)
        inward = centre.astype(np.float64)[None, :] - q.astype(np.float64)
        dots = np.einsum("ij,ij->i", got["eig"][:, 3:], inward)
        assert np.all(got["cnt"] == 20) and np.all(dots > 0)
        assert np.all(np.einsum("ij,ij->i", got["normal"][:, :3].astype(np.float64), inward) / 4.0 > 0.9)      # and they are the radii
    finally:
        ctx.close()
    # the rule without a viewpoint, on the scene
    q = scene["q"]
    for k in (5, 20):
        ref = scene["ref"](k)
        got = hip.normals(q, k)
        a = np.sort(np.abs(ref["normal"]), axis=1)
        clear = ref["well"] & ((a[:, 2] - a[:, 1]) > 1e-3)
        assert clear.sum() > 300
        big = np.argmax(np.abs(ref["normal"]), axis=1)
        assert np.all(got["normal"][np.arange(q.shape[0]), big][clear] > 0)
        assert np.abs(got["normal"][clear, :3].astype(np.float64) - ref["normal"][clear]).max() <= nc.F32      # the sign included
    # ... and with one
    vp = np.float32([0.0, 0.0, 1.0])
    got = hip.normals(q, 20, viewpoint=vp)
    dots = np.einsum("ij,ij->i", got["eig"][:, 3:], vp.astype(np.float64)[None, :] - q.astype(np.float64))
    assert np.all(dots >= 0)


# 5
def test_degenerate_and_edge_cases(hip, scene):
    from fast_limo_amd import _lib
    mp, q = scene["mp"], scene["q"]
    # k = 1, 2: never three neighbours
    for k in (1, 2):
        got = hip.normals(q[:64], k)
        assert np.all(got["cnt"] == k)
        for name in ("normal", "centroid", "cov", "eig"):
            assert np.all(np.isnan(got[name]))
    # min_pts above what the gate admits
    got = hip.normals(q, 32, 1.0, min_pts=10)
    nc.check(got, scene["ref"](32, 1.0, 10), "min_pts = 10")
    few = (got["cnt"] >= 3) & (got["cnt"] < 10)
    assert few.sum() > 0 and np.all(np.isnan(got["normal"][few])) and np.all(np.isfinite(got["normal"][got["cnt"] >= 10]))
    # a NaN query among valid ones
    q3 = np.float32([mp[100] + np.float32(0.1), [np.nan, 0, 0], mp[200] - np.float32(0.1)])
    got = hip.normals(q3, 8)
    assert list(got["cnt"]) == [8, 0, 8] and np.all(np.isnan(got["normal"][1])) and np.all(np.isfinite(got["normal"][[0, 2]]))
    same_bytes({n: got[n][[0, 2]] for n in NAMES}, hip.normals(q3[[0, 2]], 8), "beside a NaN query")
    # nq == 0
    z = hip.normals(np.zeros((0, 3), np.float32), 8)
    assert z["normal"].shape == (0, 4) and z["cnt"].shape == (0,) and z["cov"].shape == (0, 6)
    # arguments: every error leaves the outputs as they were
    out = dict(normal=np.full((3, 4), -7, np.float32), cnt=np.full(3, -7, np.int32), centroid=np.full((3, 3), -7.0), cov=np.full((3, 6), -7.0),
               eig=np.full((3, 6), -7.0))
    p = {n: a.ctypes.data for n, a in out.items()}

    def raw(qp=q3.ctypes.data, nq=3, k=8, gate=INF, min_pts=3, vp=None, normal=p["normal"], cnt=p["cnt"]):
        return hip._L.flimo_map_normals(hip._h, qp, nq, k, gate, min_pts, vp, normal, cnt, p["centroid"], p["cov"], p["eig"])
    assert raw(qp=None) == ERR_INVALID
    assert raw(normal=None) == ERR_INVALID and raw(cnt=None) == ERR_INVALID
    for bad in (np.nan, -1.0, -np.inf):
        assert raw(gate=bad) == ERR_INVALID, bad
    nan_vp = np.float32([0, np.nan, 0])
    assert raw(vp=nan_vp.ctypes.data) == ERR_INVALID
    for k in (0, -1, 65):
        assert raw(k=k) == ERR_UNSUPPORTED, k
    assert hip._L.flimo_map_normals(None, q3.ctypes.data, 3, 8, INF, 3, None, p["normal"], p["cnt"], None, None, None) == ERR_INVALID
    assert hip._L.flimo_map_normals_range(hip._h, 0, 3, 65, INF, 3, None, p["normal"], p["cnt"], None, None, None) == ERR_UNSUPPORTED
    assert hip._L.flimo_map_normals_range(hip._h, 0, 3, 8, np.nan, 3, None, p["normal"], p["cnt"], None, None, None) == ERR_INVALID
    for a in out.values():
        assert np.all(a == -7)
    assert raw(qp=None, nq=0) == 0 and np.all(out["cnt"] == -7)
    # nq * k >= 2^31 is no limit of this call: nothing of nq * k entries exists.  The path that makes it so -- chunks -- at k = 64
    hip.set_normals_chunk(100)
    try:
        a = hip.normals(q, 64)
    finally:
        hip.set_normals_chunk(0)
    same_bytes(a, hip.normals(q, 64), "chunks of 100 against one chunk")
    # an empty map: cnt 0 everywhere, NaN, FLIMO_OK
    ctx = _lib.HipCtx(0)
    try:
        got = ctx.normals(q3, 8)
        assert np.all(got["cnt"] == 0)
        for name in ("normal", "centroid", "cov", "eig"):
            assert np.all(np.isnan(got[name]))
        assert ctx.normals_range(0, 0, 8)["cnt"].shape == (0,)
        # 20 identical stored points: C = 0, curvature 0, a finite unit normal
        ctx.map_config(downsample=False)
        ctx.map_add(np.tile(np.float32([[1.5, -2.25, 0.75]]), (20, 1)))
        assert ctx.map_size() == 20
        got = ctx.normals(np.float32([[1.5, -2.25, 0.75], [2.0, 0.0, 0.0]]), 20)
        assert np.all(got["cnt"] == 20) and np.all(got["cov"] == 0) and np.all(got["eig"][:, :3] == 0) and np.all(got["normal"][:, 3] == 0)
        assert np.all(np.abs(np.linalg.norm(got["eig"][:, 3:], axis=1) - 1.0) <= nc.U_EIG)
        np.testing.assert_array_equal(got["centroid"], np.tile([[1.5, -2.25, 0.75]], (2, 1)))
    finally:
        ctx.close()
    # collinear points: the normal is orthogonal to the line
    t = np.arange(40, dtype=np.float64) * 0.125
    line = (np.float64([1.0, 2.0, -1.0])[None, :] + t[:, None] * np.float64([1.0, 0.5, 0.25])[None, :]).astype(np.float32)
    ctx = fresh_map([line], downsample=False)
    try:
        assert ctx.map_size() == 40
        got = ctx.normals(line[::3], 12)
        direction = np.float64([1.0, 0.5, 0.25]) / np.linalg.norm([1.0, 0.5, 0.25])
        assert np.all(got["cnt"] == 12)
        assert np.all(np.abs(np.linalg.norm(got["eig"][:, 3:], axis=1) - 1.0) <= nc.U_EIG)
        assert np.abs(got["eig"][:, 3:] @ direction).max() <= 1e-12
    finally:
        ctx.close()


# 6
def test_through_the_localizer_and_invisible_to_registration(built):
    from fast_limo_amd import api
    mp, scan, _ = cfg1_scene()
    imu = synth.stationary_imu(0.0, 0.45)
    rs = np.random.RandomState(4)
    q = (mp[rs.choice(mp.shape[0], 1000)] + rs.normal(0, 0.2, (1000, 3))).astype(np.float32)
    # no map yet: all cnt 0, NaN
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        got = loc.map_normals(q[:5], 16)
        assert np.all(got["cnt"] == 0) and np.all(np.isnan(got["normal"]))
        assert loc.map_normals_range(0, 0, 16)["cnt"].shape == (0,)
    finally:
        loc.close()

    def drive(call):
        loc = api.Localizer(api.default_cfg(**CAPS))
        try:
            loc.set_async_insert(True)
            found = []
            rcs = drive_two_scans(loc, mp, scan, imu)
            if call:
                sensor = np.float32(loc.get_x()[0:3])
                found.append(loc.map_normals(q, 20, viewpoint=sensor))                       # (an insert may still be running: the call waits)
                found.append(loc.map_normals_range(10, 500, 20, viewpoint=sensor))
            st, w, a = imu
            for i in np.where((st > 0.205) & (st <= 0.305))[0]:
                loc.update_imu(st[i], w[i], a[i])
            rcs.append(loc.update_pointcloud(scan, 0.2))
            if call:
                found.append(loc.map_normals(q, 20, viewpoint=sensor))                       # right after a sweep whose insert is still running
                loc.sync()
                found.append(loc.hip.normals(q, 20, viewpoint=sensor))                       # the quiescent context
            loc.sync()
            return rcs, loc.get_x().copy(), loc.get_P().copy(), loc.hip.map_points().copy(), found
        finally:
            loc.close()

    rc0, x0, P0, m0, _ = drive(False)
    rc1, x1, P1, m1, found = drive(True)
    assert rc0 == rc1
    assert x0.tobytes() == x1.tobytes() and P0.tobytes() == P1.tobytes() and m0.tobytes() == m1.tobytes()
    assert np.all(found[0]["cnt"] == 20) and np.all(np.isfinite(found[0]["normal"])) and found[1]["cnt"].shape == (500,)
    same_bytes(found[2], found[3], "behind a running insert")
    nc.check(found[3], nc.reference(q, m1, 20), "through the Localizer")
