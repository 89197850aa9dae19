"""GPU suite: outliers by neighbour statistics -- flimo_map_outliers marks the stored points whose k nearest neighbours are too few
inside the gate or too far away on average, flimo_map_remove_outliers forgets them in the crop's one ordered pass.  The yardstick is the
definition restated in numpy (tests/outliers_common.py): the neighbour counts and the bits of every mean distance are compared
exactly; mu, sigma and the threshold within the bound derived there (4 * N * 2^-52 relative) and bit for bit against the sums' one
shape (tests/sums_common.py) over the returned means and counts; and because no mean distance of any
configuration run here lies within 1e-9 relative of its threshold (tests/test_outliers_host.py asserts that), the masks and their
counts exactly.  After a removal the map is clear() + initialize(kept), as after a crop: that part is checked against a twin context."""
import ctypes as C
import math

import numpy as np
import pytest

import outliers_common as oc
from common import CAPS
from fast_limo_amd import synth
from radius_common import bits

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -2, -6
INF = float("inf")
F = np.float32
CFG_IDS = lambda c: "k%d-g%s-m%d-s%g" % (c["k"], c["max_dist"], c["min_pts"], c["std_mul"])


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_outliers", "flimo_map_remove_outliers", "flimo_set_outlier_chunk"):
        getattr(L, name)
    for name in ("flimo_loc_map_outliers", "flimo_loc_map_remove_outliers"):
        getattr(H, name)


def _ctx(pts, cell=0.0):
    """The whole scene as the first add: the first build neither drops points nor merges duplicates."""
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, True, cell)
    ctx.map_add(pts, stamp=0.5)
    assert ctx.map_size() == len(pts)
    return ctx


@pytest.fixture(scope="module")
def scene_ctx(built):
    ctx = _ctx(oc.scene())
    np.testing.assert_array_equal(ctx.map_points(), oc.scene())
    yield ctx
    ctx.close()


def _dbits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_as_yardstick(out, m, c, st, what, cfg):
    """cnt and the bits of mean_dist exact (every NaN is the quiet NaN 0x7ff8...), the stats within the bound of the yardstick and bit
    for bit what the returned mean_dist and cnt give through the sums' one shape (oc.device_stats), the mask and its counts exact.
    Each figure is printed before it is asserted."""
    got = out["stats"]
    print(what, "n_stat", got["n_stat"], "mu", repr(got["mu"]), repr(st["mu"]), "sigma", repr(got["sigma"]), repr(st["sigma"]), "threshold",
          repr(got["threshold"]), repr(st["threshold"]), "few", got["few"], st["few"], "far", got["far"], st["far"], "bound", oc.bound(st["n_stat"]),
          "gap", oc.rel_gap(m, st))
    np.testing.assert_array_equal(out["cnt"], c, err_msg=what)
    want = np.where(np.isnan(m), np.float64("nan"), m)
    bad = np.where(_dbits(out["mean_dist"]) != _dbits(want))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], out["mean_dist"][bad[:5]], want[bad[:5]])
    oc.same_stats(got, st, what)
    pin = oc.device_stats(out["mean_dist"], out["cnt"], cfg["min_pts"], cfg["std_mul"])
    print(what, "the shape's", pin)
    oc.same_bits(got, pin, what)
    np.testing.assert_array_equal(out["mask"], st["mask"], err_msg=what)


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", oc.CONFIGS, ids=CFG_IDS)
def test_counts_means_stats_and_mask_equal_the_yardstick(scene_ctx, cfg):
    m, c, st = oc.yardstick("scene", **cfg)
    _same_as_yardstick(scene_ctx.map_outliers(**cfg), m, c, st, CFG_IDS(cfg), cfg)


# ---- 2. the pure forms ----------------------------------------------------------------------------------------------------------------
def test_the_pure_forms_are_the_radius_filter_and_the_statistical_filter(scene_ctx):
    pts = oc.scene()
    k, r, need = 16, 1.0, 5
    out = scene_ctx.map_outliers(k=k, max_dist=r, min_pts=need, std_mul=INF)
    cnt = scene_ctx.radius_count(pts, r) - 1                     # flimo_radius_search's count, the point itself taken off
    small = cnt <= k
    assert small.sum() > 1000
    np.testing.assert_array_equal(out["cnt"][small], cnt[small])
    assert np.all(out["cnt"][~small] == k)
    np.testing.assert_array_equal(out["mask"], cnt < need)       # (need <= k: a count beyond k is never below need)
    assert out["stats"]["far"] == 0 and out["stats"]["few"] == int((cnt < need).sum()) == out["stats"]["outliers"]
    m, c, st = oc.yardstick("scene", k=k, max_dist=r, min_pts=need, std_mul=INF)
    _same_as_yardstick(out, m, c, st, "radius form", dict(min_pts=need, std_mul=INF))
    # the plain statistical filter: no gate, no count rule
    out = scene_ctx.map_outliers(k=8, max_dist=INF, min_pts=0, std_mul=1.0)
    s = out["stats"]
    assert s["few"] == 0 and s["n_stat"] == oc.N_SCENE and np.all(out["cnt"] == 8)
    np.testing.assert_array_equal(out["mask"], out["mean_dist"] > s["threshold"])
    assert out["mask"][8000:8300].mean() > 0.8 and out["mask"][:8000].mean() < 0.05


# ---- 3. points whose search is the walk over the tiles --------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(k=8, max_dist=INF, min_pts=0, std_mul=1.0), dict(k=17, max_dist=INF, min_pts=0, std_mul=2.0),
                                 dict(k=16, max_dist=1.0, min_pts=3, std_mul=1.0), dict(k=63, max_dist=2.0, min_pts=0, std_mul=1.0)], ids=CFG_IDS)
def test_far_points_take_the_walk_and_are_exact(built, cfg):
    ctx = _ctx(oc.far_scene())
    try:
        m, c, st = oc.yardstick("far", **cfg)
        out = ctx.map_outliers(**cfg)
        _same_as_yardstick(out, m, c, st, "far " + CFG_IDS(cfg), cfg)
        if math.isinf(cfg["max_dist"]) and cfg["std_mul"] == 1.0:
            np.testing.assert_array_equal(np.where(out["mask"])[0], oc.N_SCENE + np.arange(3))      # ungated: the three, and only they
            assert np.all(out["mean_dist"][oc.N_SCENE:] > 400.0)
    finally:
        ctx.close()


# ---- 4. invariance --------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_chunk_the_cell_size_or_the_call(scene_ctx):
    cfgs = [dict(k=8, max_dist=INF, min_pts=0, std_mul=1.0), dict(k=16, max_dist=1.0, min_pts=3, std_mul=1.0),
            dict(k=63, max_dist=2.0, min_pts=0, std_mul=2.0)]

    def sig(out):
        s = out["stats"]
        return (_dbits(out["mean_dist"]).tobytes(), out["cnt"].tobytes(), out["mask"].tobytes(), _dbits([s["mu"], s["sigma"], s["threshold"]]).tobytes(),
                s["n_stat"], s["few"], s["far"])

    base = [sig(scene_ctx.map_outliers(**cfg)) for cfg in cfgs]
    assert [sig(scene_ctx.map_outliers(**cfg)) for cfg in cfgs] == base                 # a second call
    scene_ctx.set_outlier_chunk(1000)                                                   # nine uneven chunks
    try:
        assert [sig(scene_ctx.map_outliers(**cfg)) for cfg in cfgs] == base
    finally:
        scene_ctx.set_outlier_chunk(0)
    for cell in (0.25, 0.5, 1.0):
        ctx = _ctx(oc.scene(), cell)
        try:
            assert [sig(ctx.map_outliers(**cfg)) for cfg in cfgs] == base, cell
        finally:
            ctx.close()


# ---- 5. the range form ----------------------------------------------------------------------------------------------------------------
def test_a_range_has_the_whole_maps_neighbours_and_its_own_statistics(scene_ctx):
    cfg = dict(k=8, max_dist=INF, min_pts=0, std_mul=1.0)
    whole = scene_ctx.map_outliers(**cfg)
    full = scene_ctx.map_outliers(0, oc.N_SCENE, **cfg)
    assert _dbits(full["mean_dist"]).tobytes() == _dbits(whole["mean_dist"]).tobytes() and full["stats"] == whole["stats"]
    np.testing.assert_array_equal(full["mask"], whole["mask"])
    for first, n in ((8000, 300), (8191, 3)):                    # the specks; three points across a compaction tile's edge
        for c in (cfg, dict(k=16, max_dist=1.0, min_pts=3, std_mul=1.0)):
            m, cc, st = oc.yardstick("scene", first, n, **c)
            out = scene_ctx.map_outliers(first, n, **c)
            assert len(out["mask"]) == n and out["stats"]["n"] == n
            _same_as_yardstick(out, m, cc, st, "range %d+%d %s" % (first, n, CFG_IDS(c)), c)
            assert _dbits(out["mean_dist"]).tobytes() == _dbits(scene_ctx.map_outliers(**c)["mean_dist"][first:first + n]).tobytes()
    assert abs(scene_ctx.map_outliers(8000, 300, **cfg)["stats"]["mu"] - whole["stats"]["mu"]) > 0.1      # the specks' own mean
    empty = scene_ctx.map_outliers(oc.N_SCENE, 0, **cfg)
    assert len(empty["mask"]) == 0 and empty["stats"]["n"] == 0 and math.isnan(empty["stats"]["mu"])
    from fast_limo_amd import _lib
    for first, n in ((0, oc.N_SCENE + 1), (oc.N_SCENE, 1), (oc.N_SCENE + 1, 0), (8000, 400)):
        with pytest.raises(_lib.FlimoError, match="invalid"):
            scene_ctx.map_outliers(first, n, **cfg)
        with pytest.raises(_lib.FlimoError, match="invalid"):
            scene_ctx.map_remove_outliers(first, n, **cfg)
    assert scene_ctx.map_size() == oc.N_SCENE


@pytest.mark.parametrize("first,n", [(8000, 1), (4095, 2), (100, 256), (8099, 257), (0, 4096), (4000, 4097)])
def test_range_sizes_at_the_borders_of_the_sums_shape(scene_ctx, first, n):
    """One slot, two, a workgroup's threads and one more, a segment and one more: ranges of the scene at k = 8 with no gate."""
    cfg = dict(k=8, max_dist=INF, min_pts=0, std_mul=1.0)
    m, c, st = oc.yardstick("scene", first, n, **cfg)
    out = scene_ctx.map_outliers(first, n, **cfg)
    assert out["stats"]["n"] == n == out["stats"]["n_stat"]
    _same_as_yardstick(out, m, c, st, "range %d+%d" % (first, n), cfg)


# ---- 6. removal -----------------------------------------------------------------------------------------------------------------------
def _twin_of(kept):
    from fast_limo_amd import _lib
    twin = _lib.HipCtx(0)
    twin.map_config(0.2, 2, True, 0.0)
    twin.map_add(oc.scene()[:100], stamp=0.1)
    twin.map_clear()
    if len(kept):
        twin.map_add(kept, stamp=0.5)
    return twin


def _same_map(ctx, twin, kept, what):
    assert ctx.map_size() == twin.map_size() == len(kept), what
    np.testing.assert_array_equal(ctx.map_points(), kept, err_msg=what)
    np.testing.assert_array_equal(twin.map_points(), kept, err_msg=what)
    assert ctx.grid_selfcheck()[0] == 0 and twin.grid_selfcheck()[0] == 0, what
    q = np.concatenate([oc.scene()[::7], oc.scene()[8000:8300] + F(0.05)])
    for k, gate in ((12, 3.0), (33, INF)):
        (i, s, c), (ti, ts, tc) = ctx.knn_k(q, k, gate), twin.knn_k(q, k, gate)
        np.testing.assert_array_equal(i, ti, err_msg=what)
        np.testing.assert_array_equal(bits(s), bits(ts), err_msg=what)
        np.testing.assert_array_equal(c, tc, err_msg=what)


@pytest.mark.parametrize("rng", [(0, None), (8000, 300), (8191, 3)], ids=["whole", "specks", "across-a-tile"])
def test_removal_keeps_the_rest_in_order_and_leaves_a_fresh_map(built, rng):
    first, n = rng
    cfg = dict(k=8, max_dist=INF, min_pts=0, std_mul=1.0) if n != 3 else dict(k=16, max_dist=1.0, min_pts=16, std_mul=INF)
    pts = oc.scene()
    m, c, st = oc.yardstick("scene", first, n, **cfg)
    gone = np.zeros(len(pts), bool)
    gone[first:first + len(m)] = st["mask"]
    assert 0 < gone.sum() < len(m) or n == 3
    assert gone.sum() > 0
    kept = pts[~gone]
    ctx = _ctx(pts)
    twin = _twin_of(kept)
    try:
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        removed, stats = ctx.map_remove_outliers(first, n, **cfg)
        assert removed == int(gone.sum()) == stats["outliers"]
        oc.same_stats(stats, st, "removal")
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before
        _same_map(ctx, twin, kept, "after the removal")
        # the map goes on: a later add lands in both alike, and the cleaned map is clean under the same threshold
        later = synth.box_world_map(3000, 12.0, 9)
        ctx.map_add(later, stamp=0.9); twin.map_add(later, stamp=0.9)
        assert ctx.map_size() == twin.map_size()
        _same_map(ctx, twin, ctx.map_points().copy(), "an add after the removal")
    finally:
        ctx.close(); twin.close()


def test_removing_nothing_changes_nothing_and_removing_everything_empties_the_map(built):
    pts = oc.scene()
    ctx = _ctx(pts)
    try:
        q = pts[::5]
        before = ctx.knn(q, 5)
        layout = ctx.grid_selfcheck()
        removed, stats = ctx.map_remove_outliers(k=8, max_dist=INF, min_pts=0, std_mul=INF)      # a cfg that selects nothing
        assert removed == 0 and stats["outliers"] == 0 and stats["n"] == oc.N_SCENE and stats["n_stat"] == oc.N_SCENE
        assert ctx.map_size() == oc.N_SCENE and ctx.grid_selfcheck() == layout                   # no build, no merge
        np.testing.assert_array_equal(ctx.map_points(), pts)
        for a, b in zip(before, ctx.knn(q, 5)):
            np.testing.assert_array_equal(a, b)                                                  # the very same rows, ties included
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        removed, stats = ctx.map_remove_outliers(k=4, max_dist=0.0, min_pts=1, std_mul=1.0)      # a gate nothing passes: all are `few`
        assert removed == oc.N_SCENE == stats["few"] and stats["far"] == 0 and stats["n_stat"] == 0
        assert math.isnan(stats["mu"]) and math.isnan(stats["sigma"]) and math.isnan(stats["threshold"])
        assert ctx.map_size() == 0 and len(ctx.map_points()) == 0
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before                                    # as a crop that removes everything
        i, s, c = ctx.knn_k(q[:10], 5)
        assert np.all(c == 0) and np.all(i == -1)
        out = ctx.map_outliers(k=4)                                                              # the empty map, first = n = 0
        assert out["stats"] == dict(out["stats"], n=0, n_stat=0, few=0, far=0, outliers=0) and math.isnan(out["stats"]["mu"])
        assert ctx.map_remove_outliers(k=4)[0] == 0
        ctx.map_add(pts[:500], stamp=1.5)                                                        # and it takes points again
        assert ctx.map_size() == 500 and ctx.grid_selfcheck()[0] == 0
        assert np.all(ctx.map_outliers(k=4)["cnt"] == 4)
    finally:
        ctx.close()


# ---- 7. no side effects ---------------------------------------------------------------------------------------------------------------
def test_the_predicate_changes_neither_map_nor_scan_nor_a_later_pass(built):
    from fast_limo_amd import _lib
    mp = oc.scene()
    scan = np.ascontiguousarray(synth.box_world_scan_random(4096, 12.0, 2)[:, :3])
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809

    def run(search):
        h = _ctx(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if search:
                for cfg in (dict(k=8), dict(k=33, max_dist=1.5, min_pts=2, std_mul=2.0)):
                    assert h.map_outliers(**cfg)["stats"]["outliers"] > 0
                h.set_outlier_chunk(777)
                assert h.map_outliers(5000, 3000, k=15)["stats"]["n"] == 3000
            out.append(h.match_reduce(x, mcfg))
            return out, h.map_points().copy(), h.scan_get().copy(), h.grid_selfcheck()
        finally:
            h.close()

    (plain, pm, ps, pl), (searched, sm, ss, sl) = run(False), run(True)
    assert pm.tobytes() == sm.tobytes() == mp.tobytes() and ps.tobytes() == ss.tobytes() and pl == sl
    for a, b in zip(plain, searched):
        assert a[2] == b[2] > 1000 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 8. tiny maps ---------------------------------------------------------------------------------------------------------------------
def test_maps_of_one_and_two_points(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_add(F([[1.0, 2.0, 3.0]]), stamp=0.5)
        out = ctx.map_outliers(k=8)                                  # one point: no neighbour, T empty, nothing selected
        s = out["stats"]
        assert out["cnt"].tolist() == [0] and math.isnan(out["mean_dist"][0]) and not out["mask"][0]
        assert (s["n"], s["n_stat"], s["few"], s["far"], s["outliers"]) == (1, 0, 0, 0, 0)
        assert math.isnan(s["mu"]) and math.isnan(s["sigma"]) and math.isnan(s["threshold"])
        out = ctx.map_outliers(k=8, min_pts=1)                       # ... unless the count rule asks for a neighbour
        assert out["mask"].tolist() == [True] and out["stats"]["few"] == 1 and out["stats"]["n_stat"] == 0
        assert ctx.map_remove_outliers(k=8)[0] == 0 and ctx.map_size() == 1
    finally:
        ctx.close()
    ctx = _lib.HipCtx(0)                                             # (two points, as every scene here, in the first add)
    try:
        ctx.map_add(F([[1.0, 2.0, 3.0], [1.0, 2.0, 7.0]]), stamp=0.5)
        assert ctx.map_size() == 2
        out = ctx.map_outliers(k=8, std_mul=0.0)                     # two points 4 m apart: equal means, sigma 0, none beyond mu
        s = out["stats"]
        assert out["cnt"].tolist() == [1, 1] and out["mean_dist"].tolist() == [4.0, 4.0] and not out["mask"].any()
        assert (s["n_stat"], s["mu"], s["sigma"], s["threshold"]) == (2, 4.0, 0.0, 4.0)
        out = ctx.map_outliers(1, 1, k=1, min_pts=1, max_dist=5.0)   # a range of one: N = 1, sigma 0
        assert (out["stats"]["n_stat"], out["stats"]["sigma"], out["stats"]["mu"]) == (1, 0.0, 4.0) and not out["mask"].any()
        out = ctx.map_outliers(k=8, max_dist=3.0, min_pts=1)
        assert out["mask"].all() and out["stats"]["few"] == 2 and math.isnan(out["stats"]["mu"])
        removed, s = ctx.map_remove_outliers(1, 1, k=8, max_dist=3.0, min_pts=1)
        assert removed == 1 and ctx.map_size() == 1
        np.testing.assert_array_equal(ctx.map_points(), F([[1.0, 2.0, 3.0]]))
    finally:
        ctx.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_and_map_are_untouched(scene_ctx):
    from fast_limo_amd import _lib
    L, h = scene_ctx._L, scene_ctx._h
    n = oc.N_SCENE
    layout = scene_ctx.grid_selfcheck()
    K = lambda **kw: _lib.outlier_cfg(**dict(dict(k=8, max_dist=INF, min_pts=0, std_mul=1.0), **kw))
    cases = [("null cfg", None, 0, n, ERR_INVALID), ("range beyond the map", K(), 0, n + 1, ERR_INVALID), ("first beyond the map", K(), n + 1, 0, ERR_INVALID),
             ("first + n wraps", K(), 2, 2 ** 64 - 1, ERR_INVALID), ("nan gate", K(max_dist=np.nan), 0, n, ERR_INVALID),
             ("negative gate", K(max_dist=-1.0), 0, n, ERR_INVALID), ("nan std_mul", K(std_mul=np.nan), 0, n, ERR_INVALID),
             ("negative std_mul", K(std_mul=-0.5), 0, n, ERR_INVALID), ("min_pts -1", K(min_pts=-1), 0, n, ERR_INVALID),
             ("min_pts k + 1", K(min_pts=9), 0, n, ERR_INVALID), ("k 0", K(k=0), 0, n, ERR_UNSUPPORTED), ("k 64", K(k=64, min_pts=3), 0, n, ERR_UNSUPPORTED),
             ("k -3", K(k=-3), 0, n, ERR_UNSUPPORTED), ("nan gate, n 0", K(max_dist=np.nan), 0, 0, ERR_INVALID), ("k 64, n 0", K(k=64), 5, 0, ERR_UNSUPPORTED)]
    for what, k, first, cnt_n, want in cases:
        kp = None if k is None else C.byref(k)
        mask, mean, cnt = np.full(n + 1, 7, np.uint8), np.full(n + 1, 7.0), np.full(n + 1, 7, np.int32)
        st = _lib.OutlierStats(n=9, n_stat=9, mu=3.0, sigma=3.0, threshold=3.0, few=9, far=9, outliers=9)
        removed = C.c_size_t(5)
        assert L.flimo_map_outliers(h, first, cnt_n, kp, mask.ctypes.data, mean.ctypes.data, cnt.ctypes.data, C.byref(st)) == want, what
        assert L.flimo_map_remove_outliers(h, first, cnt_n, kp, C.byref(removed), C.byref(st)) == want, what
        assert np.all(mask == 7) and np.all(mean == 7.0) and np.all(cnt == 7) and removed.value == 5, what
        assert st.as_dict() == dict(n=9, n_stat=9, mu=3.0, sigma=3.0, threshold=3.0, few=9, far=9, outliers=9), what
    assert scene_ctx.map_size() == n and scene_ctx.grid_selfcheck() == layout
    np.testing.assert_array_equal(scene_ctx.map_points(), oc.scene())
    # every output may be NULL
    k = K()
    assert L.flimo_map_outliers(h, 0, n, C.byref(k), None, None, None, None) == 0
    st = _lib.OutlierStats()
    assert L.flimo_map_outliers(h, 0, n, C.byref(k), None, None, None, C.byref(st)) == 0
    assert st.as_dict() == scene_ctx.map_outliers(k=8)["stats"]
    with pytest.raises(ValueError):
        scene_ctx.map_outliers(want=("mask", "normals"), k=8)


# ---- 10. the Localizer's forms --------------------------------------------------------------------------------------------------------
def test_the_localizer_forms_equal_the_contexts(built):
    from fast_limo_amd import api
    cfg = dict(k=16, max_dist=1.0, min_pts=3, std_mul=1.0)
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        out = loc.map_outliers(**cfg)                                # no map yet: an empty one's answer
        assert len(out["mask"]) == 0 and out["stats"]["n"] == 0 and math.isnan(out["stats"]["mu"])
        assert loc.map_remove_outliers(**cfg)[0] == 0
        with pytest.raises(api.FlimoError):
            loc.map_outliers(0, 5, **cfg)
        loc.map_add(oc.scene())
        n = loc.map_size()
        pts = loc.hip.map_points().copy()
        a, b = loc.map_outliers(**cfg), loc.hip.map_outliers(**cfg)
        assert a["stats"] == b["stats"] and a["stats"]["n"] == n and a["stats"]["outliers"] > 0
        for key in ("mask", "cnt"):
            np.testing.assert_array_equal(a[key], b[key])
        assert _dbits(a["mean_dist"]).tobytes() == _dbits(b["mean_dist"]).tobytes()
        a, b = loc.map_outliers(n - 300, 200, want=("mask",), **cfg), loc.hip.map_outliers(n - 300, 200, want=("mask",), **cfg)
        assert sorted(a) == ["mask", "stats"] and a["stats"] == b["stats"]
        np.testing.assert_array_equal(a["mask"], b["mask"])
        with pytest.raises(api.FlimoError):
            loc.map_outliers(0, n + 1, **cfg)
        whole = loc.hip.map_outliers(**cfg)
        removed, stats = loc.map_remove_outliers(**cfg)
        assert removed == whole["stats"]["outliers"] == stats["outliers"] and stats == whole["stats"]
        assert loc.map_size() == n - removed
        np.testing.assert_array_equal(loc.hip.map_points(), pts[~whole["mask"]])
        assert loc.hip.grid_selfcheck()[0] == 0
    finally:
        loc.close()
