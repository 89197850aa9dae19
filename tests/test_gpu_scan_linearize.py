"""GPU: flimo_scan_linearize (the point-to-plane normal equations of the resident scan at each of a batch of pose hypotheses) through
the C ABI, and api.scan_align over it.

The yardstick (tests/scan_linearize_common.py) is the route the call replaces: per pose the existing ``ctx.scan_to_world``, the
existing ``ctx.normals(w, k, gate, min_pts)`` with centroid and eig, the terms of flimo_c.h in numpy float64, math.fsum.  pair_cnt,
valid and every bit of rows (the NaN pattern included) are compared with no tolerance; H, g and cost within n * 2^-52 * sum|term|
of fsum (the bound of any summation order of n terms) and, in the first test and the test of the scan sizes, byte for byte against
the sums' one shape over the returned rows (``sl.pinned``, tests/sums_common.py).  Wherever two calls must give the same result the arrays are compared byte
for byte, the sums included."""
import numpy as np
import pytest

import front_end_common as fc
import scan_fitness_common as sf
import scan_linearize_common as sl
from common import CAPS, cfg1_scene, drive_two_scans
pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_TOO_LARGE = -2, -6, -5
INF = float("inf")


def fresh(batches, scan=None, cell_size=0.0, downsample=True):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    ctx.map_config(cell_size=cell_size, downsample=downsample)
    for b in batches:
        ctx.map_add(b)
    if scan is not None:
        ctx.scan_set(scan)
    return ctx


@pytest.fixture(scope="module")
def hip(built):
    ctx = fresh(sf.standard_batches(), sf.standard_scan())
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scene(hip):
    """The standard scene: 20 000 map points fed in four batches, a 1024-point scan, the 125 poses around the true one; 16 of them
    (every eighth, the true one among them) carry the comparisons with the composed route."""
    assert 0 < hip.map_size() <= sf.N_MAP and hip.scan_size() == sf.N_SCAN
    poses = sf.standard_poses()
    some = list(range(0, 125, 8))
    some[7] = sf.TRUE_POSE
    assert len(some) == 16
    return dict(poses=poses, some=some, n=sf.N_SCAN)


def test_the_error_codes_are_the_headers(built):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flimo_c.h")).read()
    for name, v in (("FLIMO_ERR_INVALID", ERR_INVALID), ("FLIMO_ERR_UNSUPPORTED", ERR_UNSUPPORTED), ("FLIMO_ERR_TOO_LARGE", ERR_TOO_LARGE)):
        m = re.search(r"#define " + name + r" \((-?\d+)\)", hdr)
        assert m and int(m.group(1)) == v, name


# ---- 1. against the composed route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,gate,min_pts,max_curv", [(5, 1.0, 3, 0.05), (3, INF, 3, INF), (16, 1.0, 5, 0.05), (20, 0.5, 3, 0.1)])
def test_against_the_composed_route(hip, scene, k, gate, min_pts, max_curv):
    poses, n = scene["poses"][scene["some"]], scene["n"]
    ref = sl.composed(hip, poses, k, gate, min_pts, max_curv)
    got = hip.scan_linearize(poses, k, gate, min_pts, max_curv, want_rows=True)
    worst = sl.check(got, ref, n, f"k {k}, gate {gate}")
    sl.pinned(got, f"k {k}, gate {gate}")
    only = hip.scan_linearize(poses, k, gate, min_pts, max_curv)
    assert sorted(only) == ["H", "cost", "g", "valid"]
    sl.same_bytes(only, got, "without rows", names=("valid", "H", "g", "cost"))
    print(f"k {k}, gate {gate}: valid {got['valid'].min()} .. {got['valid'].max()}, sums at most {worst:.3g} of the bound")
    assert got["valid"].max() > n // 2 and np.all(got["pair_cnt"] <= k)
    if np.isinf(gate):
        assert np.all(got["pair_cnt"] == k)


def test_the_curvature_gate_and_min_pts_bind(hip, scene):
    poses, n = scene["poses"][[sf.TRUE_POSE, 40]], scene["n"]
    valid = {}
    for tag, gate, min_pts, max_curv in (("open", 1.0, 3, INF), ("curv", 1.0, 3, 0.01), ("pts3", 0.3, 3, INF), ("pts5", 0.3, 5, INF)):
        got = hip.scan_linearize(poses, 5, gate, min_pts, max_curv, want_rows=True)
        sl.check(got, sl.composed(hip, poses, 5, gate, min_pts, max_curv), n, tag)      # (the numpy rule on the same eig, exactly)
        valid[tag] = got["valid"]
    print(valid)
    assert np.all(valid["curv"] < valid["open"]) and np.all(valid["curv"] > 0)
    assert np.all(valid["pts5"] < valid["pts3"]) and np.all(valid["pts5"] > 0)


# ---- 2. the bits of a pose's 28 numbers do not move --------------------------------------------------------------------------------
def test_the_bits_do_not_depend_on_the_batch_or_the_chunks(hip, scene):
    poses, n, some = scene["poses"], scene["n"], scene["some"]
    for k, gate in ((5, 1.0), (20, INF)):
        first = hip.scan_linearize(poses, k, gate, 3, 0.05, want_rows=True)
        sl.same_bytes(first, hip.scan_linearize(poses, k, gate, 3, 0.05, want_rows=True), "called twice")
        single = [hip.scan_linearize(poses[j][None, :], k, gate, 3, 0.05, want_rows=True) for j in some]
        sl.same_bytes({a: first[a][some] for a in first}, {a: np.concatenate([r[a] for r in single]) for a in first}, "the pose alone")
        try:
            for pairs in (125 * n, 18 * n, 1, 0):      # 1, 7 and 125 chunks, the default
                hip.set_linearize_chunk(pairs)
                sl.same_bytes(first, hip.scan_linearize(poses, k, gate, 3, 0.05, want_rows=True), f"chunks of {pairs} pairs")
        finally:
            hip.set_linearize_chunk(0)
        other = [100, 3, sf.TRUE_POSE, 3]
        sl.same_bytes({a: first[a][other] for a in first}, hip.scan_linearize(poses[other], k, gate, 3, 0.05, want_rows=True), "another batch")


def test_the_bits_do_not_depend_on_the_cell_size(hip, scene):
    poses = scene["poses"][scene["some"]]
    maps = [fresh(sf.standard_batches(), sf.standard_scan(), cell) for cell in (0.5, 1.0, 0.25)]
    try:
        for k, gate in ((5, 1.0), (20, INF)):
            base = hip.scan_linearize(poses, k, gate, 3, 0.05, want_rows=True)
            for m, cell in zip(maps, (0.5, 1.0, 0.25)):
                sl.same_bytes(base, m.scan_linearize(poses, k, gate, 3, 0.05, want_rows=True), f"cell size {cell}, k {k}")
    finally:
        for m in maps:
            m.close()


def test_poses_far_from_the_map_take_the_walk_over_the_tiles(hip, scene):
    """As the fitness suite's test of that name: poses that throw the scan tens of metres to kilometres from the map.  With no gate
    the far poses still get neighbourhoods, so their sums are checked against the composed route; the near pose among them has the
    bits it has alone."""
    n = scene["n"]
    poses = np.stack([sf.displaced(dx=3000.0), sf.displaced(), sf.displaced(dy=-40.0), sf.displaced(dx=40.0, dy=3000.0, dyaw_deg=90.0)])
    far = [0, 2, 3]
    for k in (5, 20):
        got = hip.scan_linearize(poses, k, INF, 3, INF, want_rows=True)
        sl.check(got, sl.composed(hip, poses, k, INF, 3, INF), n, f"far poses, no gate, k {k}")
        assert np.all(got["pair_cnt"] == k) and np.all(got["valid"] == n)
        assert np.all(np.abs(got["rows"][far][:, :, 6]).max(1) > 5.0)      # (residuals of a scan far from its planes)
        gated = hip.scan_linearize(poses, k, 1.0, 3, INF, want_rows=True)
        assert np.all(gated["valid"][far] == 0) and np.all(gated["pair_cnt"][far] == 0) and np.all(np.isnan(gated["rows"][far]))
        for name in ("H", "g", "cost"):
            assert gated[name][far].tobytes() == np.zeros_like(gated[name][far]).tobytes(), name      # (+0.0, every bit)
        sl.same_bytes({a: gated[a][1:2] for a in gated}, hip.scan_linearize(poses[1:2], k, 1.0, 3, INF, want_rows=True), "the near pose among far ones")
        sl.check(gated, sl.composed(hip, poses, k, 1.0, 3, INF), n, f"far poses, gate 1.0, k {k}")


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 1023, 1025, 4097, 8200])
def test_scan_sizes_off_the_lane_block_and_reduction_borders(scene, n):
    """Scans that do not fill the last group of lanes, the last workgroup of a pose (16 or 4 pairs per workgroup) or the last
    segment of the sums' first level (4096 slots; 4097 and 8200 have two and three segments), at k = 5 (16 lanes per pair) and
    k = 20 (a wave per pair); chunks of two poses put poses 1 and 2 on either side of a chunk border."""
    poses = scene["poses"][[sf.TRUE_POSE, 0, 124]]
    ctx = fresh(sf.standard_batches(), sf.standard_scan(n))
    try:
        assert ctx.scan_size() == n
        for k in (5, 20):
            ref = sl.composed(ctx, poses, k, 1.0, 3, 0.05)
            whole = ctx.scan_linearize(poses, k, 1.0, 3, 0.05, want_rows=True)
            sl.check(whole, ref, n, f"n = {n}, k = {k}")
            sl.pinned(whole, f"n = {n}, k = {k}")
            ctx.set_linearize_chunk(2 * n)
            sl.same_bytes(whole, ctx.scan_linearize(poses, k, 1.0, 3, 0.05, want_rows=True), f"n = {n}, k = {k}, chunks of two poses")
            ctx.set_linearize_chunk(0)
    finally:
        ctx.close()


# ---- 3. edges, against the contract ------------------------------------------------------------------------------------------------
def zeros_of(got, m, n):
    assert np.all(got["valid"] == 0) and got["valid"].shape == (m,)
    for name, shape in (("H", (m, 21)), ("g", (m, 6)), ("cost", (m,))):
        assert got[name].shape == shape and got[name].tobytes() == np.zeros(shape).tobytes(), name
    assert got["rows"].shape == (m, n, 7) and np.all(np.isnan(got["rows"])) and got["pair_cnt"].shape == (m, n) and np.all(got["pair_cnt"] == 0)


def test_nan_points_empty_map_empty_scan_no_pose_and_a_gate_of_zero(scene):
    from fast_limo_amd import _lib
    poses = scene["poses"][[sf.TRUE_POSE, 7]]
    scan = sf.standard_scan()[:300].copy()
    scan[17] = np.nan
    scan[200, 1] = np.nan
    ctx = fresh(sf.standard_batches(), scan)
    try:
        for gate in (1.0, INF):
            got = ctx.scan_linearize(poses, 5, gate, 3, INF, want_rows=True)
            assert np.all(got["pair_cnt"][:, [17, 200]] == 0) and np.all(np.isnan(got["rows"][:, [17, 200]]))
            sl.check(got, sl.composed(ctx, poses, 5, gate, 3, INF), 300, f"NaN points, gate {gate}")
        assert np.all(ctx.scan_linearize(poses, 5, INF)["valid"] == 298)
        zeros_of(ctx.scan_linearize(poses, 5, 0.0, want_rows=True), 2, 300)
        # np == 0: nothing is touched
        out = [np.full(2, -7, np.int32), np.full((2, 21), -7.0), np.full((2, 6), -7.0), np.full(2, -7.0)]
        assert ctx._L.flimo_scan_linearize(ctx._h, None, 0, 5, 1.0, 3, 0.05, *[a.ctypes.data for a in out], None, None) == 0
        assert all(np.all(a == -7) for a in out)
        z = ctx.scan_linearize(np.zeros((0, 26)), 5, 1.0, want_rows=True)
        assert z["valid"].shape == (0,) and z["H"].shape == (0, 21) and z["rows"].shape == (0, 300, 7)
    finally:
        ctx.close()
    ctx = _lib.HipCtx(0)      # an empty map
    try:
        ctx.scan_set(scan)
        zeros_of(ctx.scan_linearize(poses, 5, INF, want_rows=True), 2, 300)
    finally:
        ctx.close()
    ctx = fresh(sf.standard_batches())      # an empty scan
    try:
        zeros_of(ctx.scan_linearize(poses, 5, INF, want_rows=True), 2, 0)
    finally:
        ctx.close()


def test_every_error_leaves_the_outputs_untouched(hip, scene):
    n = scene["n"]
    good = np.ascontiguousarray(scene["poses"][:3])
    out = dict(valid=np.full(3, -7, np.int32), H=np.full((3, 21), -7.0), g=np.full((3, 6), -7.0), cost=np.full(3, -7.0),
               rows=np.full((3, n, 7), -7.0), cnt=np.full((3, n), -7, np.int32))
    p = {k: a.ctypes.data for k, a in out.items()}

    def raw(x=good, m=3, k=5, gate=1.0, min_pts=3, curv=0.05, h=hip._h, **null):
        q = dict(p, **{name: None for name in null})
        return hip._L.flimo_scan_linearize(h, None if x is None else x.ctypes.data, m, k, gate, min_pts, curv, q["valid"], q["H"], q["g"], q["cost"],
                                           q["rows"], q["cnt"])
    assert raw(h=None) == ERR_INVALID and raw(x=None) == ERR_INVALID
    for name in ("valid", "H", "g", "cost"):
        assert raw(**{name: True}) == ERR_INVALID, name
    for bad in (np.nan, -1.0, -np.inf):
        assert raw(gate=bad) == ERR_INVALID and raw(curv=bad) == ERR_INVALID, bad
    for j, t, v in ((0, 1, np.nan), (2, 0, np.nan), (2, 5, np.nan), (2, 6, np.inf), (1, 3, -np.inf), (2, 2, np.inf)):
        x = good.copy()
        x[j, t] = v
        assert raw(x=x) == ERR_INVALID, (j, t, v)
    for k in (2, 0, -1, 65):
        assert raw(k=k) == ERR_UNSUPPORTED, k
    assert raw(m=2 ** 31) == ERR_TOO_LARGE and raw(m=2 ** 40) == ERR_TOO_LARGE
    for a in out.values():
        assert np.all(a == -7)
    assert raw(k=3) == 0 and raw(k=64) == 0 and np.all(out["valid"] >= 0)
    # only pos and rot of a pose are read
    x = good.copy()
    x[:, 7:] = np.nan
    sl.same_bytes(hip.scan_linearize(x, 5, 1.0, want_rows=True), hip.scan_linearize(good, 5, 1.0, want_rows=True), "the rest of a pose")
    with pytest.raises(Exception, match="invalid argument"):
        hip.scan_linearize(good, 5, -2.0)


def test_a_scan_made_resident_by_a_deskew_is_flushed_first(scene):
    """After deskew_resident the deskew still rides on the next launch: the call must run it first.  A second context is given
    scan_get() of the first -- read only AFTER the call under test, because scan_get itself runs a pending deskew."""
    case = fc.deskew_case(3)
    poses = np.stack([fc.REST_X26, sf.displaced(dx=5.0, dyaw_deg=30.0)])
    a = fresh(sf.standard_batches(), sf.standard_scan())      # (what a missing flush would linearise instead)
    b = fresh(sf.standard_batches())
    try:
        a.raw_scan_set(case["xyz"], case["t"])
        a.deskew_resident(case["frames"], case["L2B"], case["x26"])
        got = a.scan_linearize(poses, 5, INF, want_rows=True)
        body = a.scan_get()
        assert body.shape == (fc.N_DESKEW, 3) and got["rows"].shape == (2, fc.N_DESKEW, 7)
        b.scan_set(body)
        sl.same_bytes(got, b.scan_linearize(poses, 5, INF, want_rows=True), "after a deskew")
        sl.same_bytes(got, a.scan_linearize(poses, 5, INF, want_rows=True), "once more")
        assert np.all(got["pair_cnt"] == 5)
    finally:
        a.close()
        b.close()


def test_after_an_insert_and_after_a_crop(scene):
    poses = scene["poses"][[sf.TRUE_POSE, 30, 99]]
    ctx = fresh(sf.standard_batches()[:2], sf.standard_scan())
    arg = (5, 1.0, 3, 0.05)
    try:
        n0 = ctx.map_size()
        before = ctx.scan_linearize(poses, *arg, want_rows=True)
        sl.check(before, sl.composed(ctx, poses, *arg), sf.N_SCAN, "two batches")
        for b in sf.standard_batches()[2:]:
            ctx.map_add(b)
        assert ctx.map_size() > n0
        after = ctx.scan_linearize(poses, *arg, want_rows=True)
        sl.check(after, sl.composed(ctx, poses, *arg), sf.N_SCAN, "after a second insert")
        assert after["pair_cnt"].sum() > before["pair_cnt"].sum()
        assert ctx.map_crop_box(np.float32([-30, -4, -5]), np.float32([6, 30, 30])) > 500      # indices are renumbered
        cropped = ctx.scan_linearize(poses, *arg, want_rows=True)
        sl.check(cropped, sl.composed(ctx, poses, *arg), sf.N_SCAN, "after a crop")
        assert np.all(cropped["valid"] < after["valid"])
    finally:
        ctx.close()


def test_the_call_leaves_a_measurement_pass_alone(hip, scene):
    """Three passes on a fresh context, with and without calls between them: the same HTH / HTh / M bits."""
    from fast_limo_amd import _lib
    cfg = _lib.default_match_cfg(**CAPS)
    poses = scene["poses"]

    def passes(call):
        ctx = fresh(sf.standard_batches(), sf.standard_scan())
        try:
            out, lin = [ctx.match_reduce(poses[sf.TRUE_POSE], cfg)], []
            if call:
                lin.append(ctx.scan_linearize(poses[:8], 5, 1.0, 3, 0.05, want_rows=True))
            out.append(ctx.match_reduce(poses[sf.TRUE_POSE], cfg))
            if call:
                lin.append(ctx.scan_linearize(poses[:8], 20, INF))
            out.append(ctx.match_reduce(poses[61], cfg))
            if call:
                lin.append(ctx.scan_linearize(poses[:8], 5, 1.0, 3, 0.05, want_rows=True))
            return out, lin
        finally:
            ctx.close()
    (plain, _), (mixed, lin) = passes(False), passes(True)
    assert plain[0][2] > 100
    for j, (a, b) in enumerate(zip(plain, mixed)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], f"pass {j}"
    # ... and the passes leave the call alone
    sl.same_bytes(lin[0], lin[2], "between passes")
    sl.same_bytes(lin[0], hip.scan_linearize(poses[:8], 5, 1.0, 3, 0.05, want_rows=True), "against a context without passes")


def test_through_the_localizer(built):
    from fast_limo_amd import api
    mp, scan, imu = cfg1_scene()
    poses = np.stack([sf.displaced(), sf.displaced(dx=0.5), sf.displaced(dy=-1.0, dyaw_deg=5.0), sf.displaced(dx=60.0)])
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        zeros_of(loc.scan_linearize(poses, 5, 1.0, want_rows=True), 4, 0)      # no map yet: nothing is resident
        loc.set_async_insert(True)
        assert drive_two_scans(loc, mp, scan, imu)[1] == 0
        found = {gate: loc.scan_linearize(poses, 5, gate, 3, 0.05, want_rows=True) for gate in (1.0, INF)}      # (an insert may still be running: the call waits)
        loc.sync()
        pc = loc.pc2match().copy()
        stored = loc.hip.map_points().copy()
        n = pc.shape[0]
        assert n > 1000 and found[1.0]["rows"].shape == (4, n, 7)
        ctx = fresh([stored], pc, downsample=False)
        try:
            assert np.array_equal(ctx.map_points(), stored)
            for gate in (1.0, INF):
                sl.same_bytes(found[gate], ctx.scan_linearize(poses, 5, gate, 3, 0.05, want_rows=True), f"Localizer against HipCtx, gate {gate}")
                sl.check(found[gate], sl.composed(ctx, poses, 5, gate, 3, 0.05), n, f"through the Localizer, gate {gate}")
            assert found[1.0]["valid"][3] == 0 and found[1.0]["valid"][0] > n // 2
        finally:
            ctx.close()
    finally:
        loc.close()


# ---- 4. the loop over the call ------------------------------------------------------------------------------------------------------
def test_scan_align_converges_from_the_nine_starts(hip, scene):
    from fast_limo_amd import api
    start = sl.start_poses(sl.STARTS)
    res = api.scan_align(hip, start, k=5, max_dist=1.0, max_curv=0.05, iters=12)      # ONE batch
    again = api.scan_align(hip, start, k=5, max_dist=1.0, max_curv=0.05, iters=12)
    errs = [sl.pose_error(x) for x in res["x26"]]
    for s, (dp, dr), it, v, c in zip(sl.STARTS, errs, res["iters"], res["valid"], res["cost"]):
        print(f"start {s}: iterations {it}, valid {v}, cost {c:.3f}; {dp * 1e3:.2f} mm, {dr:.4f} deg")
    for name in res:
        assert res[name].tobytes() == again[name].tobytes(), f"two runs: {name} differs"
    assert np.all(res["status"] == api.ALIGN_RUNNING) and np.all(res["iters"] == 12)
    for s, (dp, dr) in zip(sl.STARTS, errs):
        assert dp <= sl.POS_BAR and dr <= sl.ROT_BAR_DEG, s


def test_rank_then_refine(hip, scene):
    from fast_limo_amd import api
    poses, n = scene["poses"], scene["n"]
    inl, s = hip.scan_fitness(poses, 0.5)
    best = np.argsort(api.fitness_cost(inl, s, n, 0.5), kind="stable")[:3]
    assert best[0] == sf.TRUE_POSE
    res = api.scan_align(hip, poses[best], k=5, max_dist=1.0, max_curv=0.05, iters=12)
    for j, x in zip(best, res["x26"]):
        dp, dr = sl.pose_error(x)
        print(f"pose {j}: {sl.pose_error(poses[j])} -> {dp * 1e3:.2f} mm, {dr:.4f} deg")
        assert dp <= sl.POS_BAR and dr <= sl.ROT_BAR_DEG, j
