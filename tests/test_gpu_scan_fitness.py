"""GPU: flimo_scan_fitness (how well the resident scan fits the map at each of a batch of pose hypotheses) through the C ABI.

The yardstick (tests/scan_fitness_common.py) is the route the call replaces: the world points of the existing
``ctx.scan_to_world(x26_j)``, their nearest stored point by knn_k_common.brute_knn over ``ctx.map_points()``, math.fsum of the
float32 distances.  inliers, nn_idx and the bits of nn_sqd are compared with no tolerance, sum_sqd within n * 2^-52 * fsum (the bound
of any summation order of n non-negative terms).  Wherever two calls must give the same result the arrays are compared byte for
byte, sum_sqd included."""
import numpy as np
import pytest

import front_end_common as fc
import scan_fitness_common as sf
from common import CAPS, cfg1_scene, drive_two_scans
pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5
INF = float("inf")


def same_bytes(a, b, tag=""):
    assert len(a) == len(b)
    for name, x, y in zip(("inliers", "sum_sqd", "nn_sqd", "nn_idx"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{tag}: {name} differs"


def fresh(batches, scan=None, cell_size=0.0, downsample=True):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    ctx.map_config(cell_size=cell_size, downsample=downsample)
    for b in batches:
        ctx.map_add(b)
    if scan is not None:
        ctx.scan_set(scan)
    return ctx


def reference(ctx, poses, gate):
    """The yardstick of `poses` for the context's resident scan and map."""
    return sf.yardstick([ctx.scan_to_world(x) for x in poses], ctx.map_points(), gate)


@pytest.fixture(scope="module")
def hip(built):
    ctx = fresh(sf.standard_batches(), sf.standard_scan())
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scene(hip):
    """The standard scene: 20 000 map points fed in four batches, a 1024-point scan, 125 poses around the true one.  The world points
    come from scan_to_world once; the yardstick of a gate is computed once."""
    mp = hip.map_points()
    assert 0 < mp.shape[0] == hip.map_size() <= sf.N_MAP and hip.scan_size() == sf.N_SCAN
    poses = sf.standard_poses()
    worlds = [hip.scan_to_world(x) for x in poses]
    refs = {}

    def ref(gate):
        if gate not in refs:
            refs[gate] = sf.yardstick(worlds, mp, gate)
        return refs[gate]
    return dict(mp=mp, poses=poses, worlds=worlds, ref=ref, ref_gpu=lambda gate: hip.scan_fitness(poses, gate), n=sf.N_SCAN)


# ---- 1. correctness on the standard scene --------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [0.5, 1.0, INF, 0.0])
def test_against_the_yardstick(hip, scene, gate):
    from fast_limo_amd import api
    poses, n = scene["poses"], scene["n"]
    ref = scene["ref"](gate)
    got = hip.scan_fitness(poses, gate, want_nn=True)
    sf.check(got, ref, n, f"gate {gate}")
    only = hip.scan_fitness(poses, gate)
    assert len(only) == 2
    same_bytes(only, got[:2], f"gate {gate}, without nn")
    inl, s = only
    print(f"gate {gate}: inliers {inl.min()} .. {inl.max()}, true pose {inl[sf.TRUE_POSE]}, sum_sqd {s[sf.TRUE_POSE]!r}")
    if gate == 0.0:
        assert np.all(inl == 0) and np.all(s == 0.0) and np.all(got[2] == -1) and np.all(got[3] == -1)
    elif np.isinf(gate):
        assert np.all(inl == n) and np.all(got[3] >= 0)
    else:
        cost = api.fitness_cost(inl, s, n, gate)
        assert int(np.argmin(cost)) == sf.TRUE_POSE and inl[sf.TRUE_POSE] == inl.max()
        if gate == 0.5:      # (the gate whose premise tests/test_scan_fitness_host.py holds: strictly the most inliers, a clear winner)
            others = np.arange(len(inl)) != sf.TRUE_POSE
            assert int(np.argmax(inl)) == sf.TRUE_POSE and inl[sf.TRUE_POSE] > inl[others].max()
            assert cost[others].min() >= 1.5 * cost[sf.TRUE_POSE]


# ---- 2. invariance of the bits ---------------------------------------------------------------------------------------------------
def test_the_bits_do_not_depend_on_the_batch_or_the_chunks(hip, scene):
    poses, n = scene["poses"], scene["n"]
    for gate in (0.5, INF):
        first = hip.scan_fitness(poses, gate, want_nn=True)
        same_bytes(first, hip.scan_fitness(poses, gate, want_nn=True), "called twice")
        single = [hip.scan_fitness(x[None, :], gate, want_nn=True) for x in poses]
        same_bytes(first, tuple(np.concatenate([r[i] for r in single]) for i in range(4)), "np = 1 per pose")
        try:
            for pairs in (1, 3 * n, 0):
                hip.set_fitness_chunk(pairs)
                same_bytes(first, hip.scan_fitness(poses, gate, want_nn=True), f"chunks of {pairs} pairs")
        finally:
            hip.set_fitness_chunk(0)
        # a pose's numbers do not depend on its neighbours in the batch
        some = [100, 3, sf.TRUE_POSE, 3]
        same_bytes(tuple(a[some] for a in first), hip.scan_fitness(poses[some], gate, want_nn=True), "another batch")


def test_the_bits_do_not_depend_on_the_cell_size(hip, scene):
    poses, mp = scene["poses"][::4], scene["mp"]
    maps = [fresh(sf.standard_batches(), sf.standard_scan(), cell) for cell in (0.25, 0.5, 1.0)]
    try:
        for gate in (0.5, INF):
            base = hip.scan_fitness(poses, gate, want_nn=True)
            has = base[3] >= 0
            for m, cell in zip(maps, (0.25, 0.5, 1.0)):
                got = m.scan_fitness(poses, gate, want_nn=True)
                for i, name in enumerate(("inliers", "sum_sqd", "nn_sqd")):
                    assert got[i].tobytes() == base[i].tobytes(), f"cell size {cell}, gate {gate}: {name} differs"
                # the indices against each map's own points
                own = m.map_points()
                assert np.array_equal(got[3] >= 0, has)
                assert own[got[3][has]].tobytes() == mp[base[3][has]].tobytes(), f"cell size {cell}: nn_idx"
    finally:
        for m in maps:
            m.close()


# ---- 3. search paths ---------------------------------------------------------------------------------------------------------------
def test_poses_far_from_the_map_take_the_walk_over_the_tiles(hip, scene):
    n = scene["n"]
    poses = np.stack([sf.displaced(dx=3000.0), sf.displaced(), sf.displaced(dy=-40.0), sf.displaced(dx=40.0, dy=3000.0, dyaw_deg=90.0)])
    far = [0, 2, 3]
    got = hip.scan_fitness(poses, INF, want_nn=True)
    sf.check(got, reference(hip, poses, INF), n, "far poses, no gate")
    assert np.all(got[0] == n) and np.all(got[2][far] > 15.0 ** 2)
    got = hip.scan_fitness(poses, 1.0, want_nn=True)
    assert np.all(got[0][far] == 0) and got[1][far].tobytes() == np.zeros(3).tobytes() and np.all(got[2][far] == -1) and np.all(got[3][far] == -1)
    same_bytes(tuple(a[1:2] for a in got), hip.scan_fitness(poses[1:2], 1.0, want_nn=True), "the near pose among far ones")
    sf.check(got, reference(hip, poses, 1.0), n, "far poses, gate 1.0")


@pytest.mark.parametrize("n", [1000, 1])
def test_scan_sizes_off_the_block_and_chunk_borders(scene, n):
    """A scan that does not fill the last workgroup of a pose (32 queries per workgroup), chunks of two poses: poses 1 and 2 lie on
    either side of a chunk border, the last chunk holds one pose."""
    poses = scene["poses"][[sf.TRUE_POSE, 0, 124, 37, 88]]
    ctx = fresh(sf.standard_batches(), sf.standard_scan(1024)[:n])
    try:
        assert ctx.scan_size() == n
        ref = reference(ctx, poses, 0.5)
        whole = ctx.scan_fitness(poses, 0.5, want_nn=True)
        sf.check(whole, ref, n, f"n = {n}")
        ctx.set_fitness_chunk(2 * n)
        same_bytes(whole, ctx.scan_fitness(poses, 0.5, want_nn=True), f"n = {n}, chunks of two poses")
        sf.check(ctx.scan_fitness(poses, INF, want_nn=True), reference(ctx, poses, INF), n, f"n = {n}, no gate")
    finally:
        ctx.close()


# ---- 4. edge cases -----------------------------------------------------------------------------------------------------------------
def test_nan_points_empty_map_empty_scan_and_no_pose(scene):
    from fast_limo_amd import _lib
    poses = scene["poses"][[sf.TRUE_POSE, 7]]
    scan = sf.standard_scan()[:300].copy()
    scan[17] = np.nan
    scan[200, 1] = np.nan
    ctx = fresh(sf.standard_batches(), scan)
    try:
        for gate in (1.0, INF):
            got = ctx.scan_fitness(poses, gate, want_nn=True)
            assert np.all(got[2][:, [17, 200]] == -1) and np.all(got[3][:, [17, 200]] == -1)
            sf.check(got, reference(ctx, poses, gate), 300, f"NaN points, gate {gate}")
        assert np.all(ctx.scan_fitness(poses, INF)[0] == 298)
        # np == 0: nothing is touched
        inl, s = np.full(2, -7, np.int32), np.full(2, -7.0)
        assert ctx._L.flimo_scan_fitness(ctx._h, None, 0, 1.0, inl.ctypes.data, s.ctypes.data, None, None) == 0
        assert np.all(inl == -7) and np.all(s == -7)
        z = ctx.scan_fitness(np.zeros((0, 26)), 1.0, want_nn=True)
        assert z[0].shape == (0,) and z[1].shape == (0,) and z[2].shape == (0, 300)
    finally:
        ctx.close()
    # an empty map
    ctx = _lib.HipCtx(0)
    try:
        ctx.scan_set(scan)
        got = ctx.scan_fitness(poses, INF, want_nn=True)
        assert np.all(got[0] == 0) and np.all(got[1] == 0.0) and got[2].shape == (2, 300) and np.all(got[2] == -1) and np.all(got[3] == -1)
    finally:
        ctx.close()
    # an empty scan
    ctx = fresh(sf.standard_batches())
    try:
        got = ctx.scan_fitness(poses, INF, want_nn=True)
        assert np.all(got[0] == 0) and np.all(got[1] == 0.0) and got[2].shape == (2, 0) and got[3].shape == (2, 0)
    finally:
        ctx.close()


def test_every_error_leaves_the_outputs_untouched(hip, scene):
    n = scene["n"]
    good = np.ascontiguousarray(scene["poses"][:3])
    out = dict(inl=np.full(3, -7, np.int32), s=np.full(3, -7.0), sqd=np.full((3, n), -7, np.float32), idx=np.full((3, n), -7, np.int32))
    p = {k: a.ctypes.data for k, a in out.items()}

    def raw(x=good, m=3, gate=1.0, inl=p["inl"], s=p["s"], h=hip._h):
        return hip._L.flimo_scan_fitness(h, None if x is None else x.ctypes.data, m, gate, inl, s, p["sqd"], p["idx"])
    assert raw(h=None) == ERR_INVALID
    assert raw(x=None) == ERR_INVALID
    assert raw(inl=None) == ERR_INVALID and raw(s=None) == ERR_INVALID
    for bad in (np.nan, -1.0, -np.inf):
        assert raw(gate=bad) == ERR_INVALID, bad
    for j, t, v in ((0, 1, np.nan), (2, 0, np.nan), (2, 5, np.nan), (2, 6, np.inf), (1, 3, -np.inf), (2, 2, np.inf)):
        x = good.copy()
        x[j, t] = v
        assert raw(x=x) == ERR_INVALID, (j, t, v)
    assert raw(m=2 ** 31) == ERR_TOO_LARGE and raw(m=2 ** 40) == ERR_TOO_LARGE
    for a in out.values():
        assert np.all(a == -7)
    # only pos and rot of a pose are read
    x = good.copy()
    x[:, 7:] = np.nan
    same_bytes(hip.scan_fitness(x, 1.0, want_nn=True), hip.scan_fitness(good, 1.0, want_nn=True), "the rest of a pose")
    with pytest.raises(Exception, match="invalid argument"):
        hip.scan_fitness(good, -2.0)


# ---- 5. the state of the scan and the map ----------------------------------------------------------------------------------------
def test_a_scan_made_resident_by_a_deskew_is_flushed_first(scene):
    """After deskew_resident the deskew still rides on the next launch: the call must run it first.  A second context is given
    scan_get() of the first -- read only AFTER the call under test, because scan_get itself runs a pending deskew."""
    case = fc.deskew_case(3)
    poses = np.stack([fc.REST_X26, sf.displaced(dx=5.0, dyaw_deg=30.0)])
    a = fresh(sf.standard_batches(), sf.standard_scan())      # (what a missing flush would score instead)
    b = fresh(sf.standard_batches())
    try:
        a.raw_scan_set(case["xyz"], case["t"])
        a.deskew_resident(case["frames"], case["L2B"], case["x26"])
        got = a.scan_fitness(poses, INF, want_nn=True)
        body = a.scan_get()
        assert body.shape == (fc.N_DESKEW, 3) and got[2].shape == (2, fc.N_DESKEW)
        b.scan_set(body)
        same_bytes(got, b.scan_fitness(poses, INF, want_nn=True), "after a deskew")
        same_bytes(got, a.scan_fitness(poses, INF, want_nn=True), "once more")
        assert np.all(got[0] == fc.N_DESKEW)
    finally:
        a.close()
        b.close()


def test_after_an_insert_and_after_a_crop(scene):
    poses = scene["poses"][[sf.TRUE_POSE, 30, 99]]
    ctx = fresh(sf.standard_batches()[:2], sf.standard_scan())
    try:
        n0 = ctx.map_size()
        sf.check(ctx.scan_fitness(poses, 0.5, want_nn=True), reference(ctx, poses, 0.5), sf.N_SCAN, "two batches")
        for b in sf.standard_batches()[2:]:
            ctx.map_add(b)
        assert ctx.map_size() > n0
        after = ctx.scan_fitness(poses, 0.5, want_nn=True)
        sf.check(after, reference(ctx, poses, 0.5), sf.N_SCAN, "after a second insert")
        assert after[0][0] == scene["ref"](0.5)[0][sf.TRUE_POSE]      # (now the standard map)
        assert ctx.map_crop_box(np.float32([-30, -4, -5]), np.float32([6, 30, 30])) > 500      # indices are renumbered
        cropped = ctx.scan_fitness(poses, 0.5, want_nn=True)
        sf.check(cropped, reference(ctx, poses, 0.5), sf.N_SCAN, "after a crop")
        assert np.all(cropped[0] < after[0])
        sf.check(ctx.scan_fitness(poses, INF, want_nn=True), reference(ctx, poses, INF), sf.N_SCAN, "after a crop, no gate")
    finally:
        ctx.close()


def test_the_call_leaves_a_measurement_pass_alone(scene):
    """Three passes on a fresh context, with and without calls between them: the same HTH / HTh / M bits.  (A context per sequence,
    as the k-NN suite does: both then start from the same state.)"""
    from fast_limo_amd import _lib
    cfg = _lib.default_match_cfg(**CAPS)
    poses = scene["poses"]

    def passes(call):
        ctx = fresh(sf.standard_batches(), sf.standard_scan())
        try:
            out, fit = [ctx.match_reduce(poses[sf.TRUE_POSE], cfg)], []
            if call:
                fit.append(ctx.scan_fitness(poses[:8], 1.0, want_nn=True))
            out.append(ctx.match_reduce(poses[sf.TRUE_POSE], cfg))
            if call:
                fit.append(ctx.scan_fitness(poses[:8], INF))
            out.append(ctx.match_reduce(poses[61], cfg))
            if call:
                fit.append(ctx.scan_fitness(poses, 0.5, want_nn=True))
            return out, fit
        finally:
            ctx.close()
    (plain, _), (mixed, fit) = passes(False), passes(True)
    assert plain[0][2] > 100
    for j, (a, b) in enumerate(zip(plain, mixed)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], f"pass {j}"
    # ... and the passes leave the call alone
    sf.check(fit[2], scene["ref"](0.5), scene["n"], "between passes")
    same_bytes(fit[0][:2], tuple(a[:8] for a in scene["ref_gpu"](1.0)), "between passes, gate 1.0")


# ---- 6. the Localizer layer --------------------------------------------------------------------------------------------------------
def test_through_the_localizer(built):
    from fast_limo_amd import api
    mp, scan, imu = cfg1_scene()
    poses = np.stack([sf.displaced(), sf.displaced(dx=0.5), sf.displaced(dy=-1.0, dyaw_deg=5.0), sf.displaced(dx=60.0)])
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        # no map yet: nothing is resident
        got = loc.scan_fitness(poses, 1.0, want_nn=True)
        assert np.all(got[0] == 0) and np.all(got[1] == 0.0) and got[2].shape == (4, 0)
        loc.set_async_insert(True)
        assert drive_two_scans(loc, mp, scan, imu)[1] == 0      # (the first sweep is a null iteration, the second one is registered)
        found = {gate: loc.scan_fitness(poses, gate, want_nn=True) for gate in (1.0, INF)}      # (an insert may still be running: the call waits)
        loc.sync()
        pc = loc.pc2match().copy()
        stored = loc.hip.map_points().copy()
        n = pc.shape[0]
        assert n > 1000 and found[1.0][2].shape == (4, n)
        ctx = fresh([stored], pc, downsample=False)
        try:
            assert np.array_equal(ctx.map_points(), stored)
            for gate in (1.0, INF):
                same_bytes(found[gate], ctx.scan_fitness(poses, gate, want_nn=True), f"Localizer against HipCtx, gate {gate}")
                sf.check(found[gate], reference(ctx, poses, gate), n, f"through the Localizer, gate {gate}")
            assert np.all(found[1.0][0][3] == 0) and np.all(found[INF][0] == n)
        finally:
            ctx.close()
    finally:
        loc.close()
