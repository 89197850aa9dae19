"""GPU suite: Euclidean clusters of the stored points -- flimo_map_clusters labels every stored point with the smallest insertion
index of its connected component under "sqdist3 < tol * tol", flimo_map_remove_clusters forgets the points of selected components in
the crop's one ordered pass.  The yardstick is the definition restated in numpy and a plain union-find (tests/clusters_common.py).
The predicate is float32 arithmetic that numpy reproduces bit for bit and every output is an integer with one correct value, so
label, size, mask and every field of stats are compared with NO tolerance, no pair left out.  After a removal the map is clear() +
initialize(kept), as after a crop: that part is checked against a twin context."""
import ctypes as C
import itertools

import numpy as np
import pytest

import clusters_common as cc
from common import CAPS
from radius_common import bits

pytestmark = pytest.mark.gpu

ERR_INVALID = -2
F = np.float32
INF = float("inf")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_clusters", "flimo_map_remove_clusters", "flimo_set_cluster_chunk"):
        getattr(L, name)
    for name in ("flimo_loc_map_clusters", "flimo_loc_map_remove_clusters"):
        getattr(H, name)


def _ctx(batches, cell=0.0, downsample=True):
    """One batch: the first add neither drops points nor merges duplicates.  Several: the stored points are what the context says."""
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, downsample, cell)
    for k, b in enumerate(batches):
        ctx.map_add(b, stamp=0.5 + k)
    return ctx


def _one(pts, cell=0.0):
    ctx = _ctx([pts], cell)
    assert ctx.map_size() == len(pts)
    return ctx


def _sig(out):
    s = out["stats"]
    return tuple(out[k].tobytes() for k in ("label", "size", "mask")) + tuple(s[k] for k in ("n", "clusters", "largest", "sel_clusters", "sel_points"))


@pytest.fixture(scope="module")
def std(built):
    """The standard scene in three batches (insertion order and cell order differ), its stored points, and the whole map's labels
    per tol, computed once."""
    pts = cc.scene()
    ctx = _ctx([pts[:2500], pts[2500:4100], pts[4100:]], downsample=False)
    stored = ctx.map_points().copy()
    assert 4000 <= len(stored) <= 8000
    labels = {tol: cc.labels(stored, tol) for tol in cc.SCENE_TOLS}
    yield dict(ctx=ctx, pts=stored, labels=labels)
    ctx.close()


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_small_maps_at_the_edges_of_groups_and_blocks(built, n):
    pts = cc.small(n)
    ctx = _one(pts)
    try:
        for cfg in (dict(tol=0.5), dict(tol=0.5, min_size=2, max_size=5), dict(tol=0.0), dict(tol=50.0, min_size=n, max_size=n)):
            want = cc.restate(pts, **cfg)
            got = ctx.map_clusters(**cfg)
            print(n, cfg, got["stats"])
            cc.same(got, want, "n %d %s" % (n, cfg))
    finally:
        ctx.close()


@pytest.mark.parametrize("tol", cc.SCENE_TOLS)
def test_the_standard_scene_equals_the_restatement(std, tol):
    ctx, lab = std["ctx"], std["labels"][tol]
    for sel in (dict(min_size=1, max_size=0), dict(min_size=2, max_size=59), dict(min_size=60, max_size=0), dict(min_size=0, max_size=1)):
        want = cc.finish(lab, **sel)
        got = ctx.map_clusters(tol=tol, **sel)
        print("tol", tol, sel, got["stats"], "plan", cc.plan(ctx.map_index_layout(), tol))
        cc.same(got, want, "tol %g %s" % (tol, sel))
    from fast_limo_amd import api
    lists = api.cluster_lists(got["label"], min_size=2)
    assert len(lists) == int((np.bincount(lab)[np.unique(lab)] >= 2).sum()) and len(lists[0]) == want["stats"]["largest"]


def test_the_threshold_is_strict_on_the_device(built):
    for pts, tol, clusters in ((cc.pair_at(0.5), 0.5, 2), (cc.pair_at(cc.below(0.5)), 0.5, 1), (cc.lattice(), 1.0, 2048),
                               (cc.lattice(), float(np.nextafter(F(1), F(2))), 1)):
        ctx = _one(pts)
        try:
            got = ctx.map_clusters(tol=tol)
            cc.same(got, cc.restate(pts, tol=tol), "threshold")
            assert got["stats"]["clusters"] == clusters and got["stats"]["largest"] == len(pts) // clusters
        finally:
            ctx.close()


def test_two_chains_in_random_order_are_two_clusters(built):
    """5 000 points along a helix spaced 0.8 tol, a second helix passing it at 1.5 tol, inserted in a seeded random order: hooking
    from both sides, long paths, retried exchanges.  One cluster each: labels 0 and 1 (the chains' first points), sizes 5 000."""
    pts, which = cc.chains()
    ctx = _one(pts)
    try:
        for chunk in (0, 64):
            ctx.set_cluster_chunk(chunk)
            got = ctx.map_clusters(tol=0.25)
            assert got["stats"] == dict(n=10000, clusters=2, largest=5000, sel_clusters=2, sel_points=10000)
            np.testing.assert_array_equal(got["label"], which)
            assert np.all(got["size"] == 5000)
        cc.same(got, cc.restate(pts, tol=0.25), "chains")
    finally:
        ctx.close()


def test_three_hundred_duplicates_among_others(built):
    pts = cc.duplicates()
    ctx = _one(pts)
    try:
        for tol in (0.0, 1e-3, 0.5):
            got = ctx.map_clusters(tol=tol, min_size=300, max_size=0)
            cc.same(got, cc.restate(pts, tol=tol, min_size=300, max_size=0), "duplicates tol %g" % tol)
        assert got["stats"]["largest"] >= 300
        got = ctx.map_clusters(tol=0.0)
        assert got["stats"]["clusters"] == 700 and np.array_equal(got["label"], np.arange(700))
        got = ctx.map_clusters(tol=1e-3)
        assert np.all(got["label"][200:500] == 200) and np.all(got["size"][200:500] == 300)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [("scene", 0.5, 0.3, "8"), ("scene", 0.5, 0.9, "16"), ("scene", 0.5, 1.3, "64"), ("scene", 0.125, 0.3, "64"),
                                  ("sparse", 0.5, 20.0, "tiles")], ids=lambda c: "%s-cell%g-tol%g-%s" % c)
def test_every_lane_plan(built, case):
    which, cell, tol, plan = case
    pts = cc.scene() if which == "scene" else cc.sparse()
    ctx = _one(pts, cell)
    try:
        assert cc.plan(ctx.map_index_layout(), tol) == plan
        want = cc.restate(pts, tol=tol, min_size=2, max_size=0)
        got = ctx.map_clusters(tol=tol, min_size=2, max_size=0)
        print(case, got["stats"])
        cc.same(got, want, str(case))
        if which == "sparse":
            assert 10 < got["stats"]["clusters"] < 60                      # several clusters, not one
    finally:
        ctx.close()


# ---- 2. invariance --------------------------------------------------------------------------------------------------------------------
def test_no_byte_moves_with_chunk_cell_repetition_an_earlier_call_or_another_context(std):
    ctx, pts = std["ctx"], std["pts"]
    cfgs = [dict(tol=tol, min_size=2, max_size=40) for tol in cc.SCENE_TOLS]
    base = [_sig(ctx.map_clusters(**cfg)) for cfg in cfgs]
    for cfg, b in zip(cfgs, base):
        assert b == _sig(cc.finish(std["labels"][cfg["tol"]], min_size=2, max_size=40))
    assert [_sig(ctx.map_clusters(**cfg)) for cfg in cfgs] == base          # a second call
    ctx.set_cluster_chunk(64)
    try:
        assert [_sig(ctx.map_clusters(**cfg)) for cfg in cfgs] == base
    finally:
        ctx.set_cluster_chunk(0)
    ctx.map_clusters(tol=3.0)                                              # a larger call before
    assert [_sig(ctx.map_clusters(**cfg)) for cfg in cfgs] == base
    for cell in (0.25, 1.0):                                               # two cell sizes, each a second context, one batch
        other = _one(pts, cell)
        try:
            assert [_sig(other.map_clusters(**cfg)) for cfg in cfgs] == base, cell
        finally:
            other.close()


def test_a_range_is_the_slice_of_the_whole_map(std):
    ctx, N = std["ctx"], len(std["pts"])
    tol = cc.SCENE_TOLS[1]
    sel = dict(min_size=2, max_size=60)
    whole = ctx.map_clusters(tol=tol, **sel)
    for first, n in ((0, N), (0, 1), (0, 777), (N // 2, 1000), (N - 1, 1), (N, 0), (17, 0)):
        got = ctx.map_clusters(first, n, tol=tol, **sel)
        want = cc.finish(std["labels"][tol], first, n, **sel)
        cc.same(got, want, "range %d+%d" % (first, n))
        for key in ("label", "size", "mask"):
            np.testing.assert_array_equal(got[key], whole[key][first:first + n])
        assert got["stats"]["n"] == n and got["stats"]["clusters"] == whole["stats"]["clusters"]


def test_every_combination_of_null_outputs(std):
    from fast_limo_amd import _lib
    ctx, N = std["ctx"], len(std["pts"])
    L, h = ctx._L, ctx._h
    first, n = 100, N - 300
    k = _lib.cluster_cfg(tol=cc.SCENE_TOLS[1], min_size=2, max_size=60)
    want = cc.finish(std["labels"][cc.SCENE_TOLS[1]], first, n, min_size=2, max_size=60)
    for wl, ws, wm, wst in itertools.product((False, True), repeat=4):
        label, size, mask = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8)
        st = _lib.ClusterStats()
        rc = L.flimo_map_clusters(h, first, n, C.byref(k), label.ctypes.data if wl else None, size.ctypes.data if ws else None,
                                  mask.ctypes.data if wm else None, C.byref(st) if wst else None)
        assert rc == 0
        if wl:
            np.testing.assert_array_equal(label, want["label"])
        if ws:
            np.testing.assert_array_equal(size, want["size"])
        if wm:
            np.testing.assert_array_equal(mask.astype(bool), want["mask"])
        if wst:
            assert st.as_dict() == want["stats"]
    assert sorted(ctx.map_clusters(want=("size",), tol=0.1)) == ["size", "stats"]
    with pytest.raises(ValueError):
        ctx.map_clusters(want=("label", "normals"), tol=0.1)


# ---- 3. no side effects ---------------------------------------------------------------------------------------------------------------
def test_the_call_changes_neither_map_nor_scan_nor_a_later_pass(built):
    from fast_limo_amd import _lib, synth
    import outliers_common as oc
    mp = oc.scene()
    scan = np.ascontiguousarray(synth.box_world_scan_random(4096, 12.0, 2)[:, :3])
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    q = mp[::9]

    def run(search):
        h = _one(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if search:
                for cfg in (dict(tol=0.3), dict(tol=1.0, min_size=2, max_size=50)):
                    assert h.map_clusters(**cfg)["stats"]["clusters"] > 1
                h.set_cluster_chunk(777)
                assert h.map_clusters(5000, 3000, tol=0.5)["stats"]["n"] == 3000
            out.append(h.match_reduce(x, mcfg))
            return out, h.map_points().copy(), h.scan_get().copy(), h.grid_selfcheck(), h.knn_k(q, 12, 3.0)
        finally:
            h.close()

    (plain, pm, ps, pl, pk), (searched, sm, ss, sl, sk) = run(False), run(True)
    assert pm.tobytes() == sm.tobytes() == mp.tobytes() and ps.tobytes() == ss.tobytes() and pl == sl
    for a, b in zip(pk, sk):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(plain, searched):
        assert a[2] == b[2] > 1000 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 4. removal -----------------------------------------------------------------------------------------------------------------------
def _twin_of(kept):
    twin = _ctx([cc.scene()[:100]])
    twin.map_clear()
    if len(kept):
        twin.map_add(kept, stamp=0.5)
    return twin


def _same_map(ctx, twin, kept, what):
    from fast_limo_amd import _lib
    assert ctx.map_size() == twin.map_size() == len(kept), what
    np.testing.assert_array_equal(ctx.map_points(), kept, err_msg=what)
    np.testing.assert_array_equal(twin.map_points(), kept, err_msg=what)
    assert ctx.grid_selfcheck()[0] == 0 and twin.grid_selfcheck()[0] == 0, what
    q = np.concatenate([kept[::7], kept[::11] + F(0.03)])
    for k, gate in ((12, 3.0), (33, INF)):
        (i, s, c), (ti, ts, tc) = ctx.knn_k(q, k, gate), twin.knn_k(q, k, gate)
        np.testing.assert_array_equal(i, ti, err_msg=what)
        np.testing.assert_array_equal(bits(s), bits(ts), err_msg=what)
        np.testing.assert_array_equal(c, tc, err_msg=what)
    # a registration pass, bit for bit
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    scan = np.ascontiguousarray(kept[::3] + F(0.02))
    ctx.scan_set(scan); twin.scan_set(scan)
    a, b = ctx.match_reduce(x, mcfg), twin.match_reduce(x, mcfg)
    print(what, "matches", a[2])
    assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), what


@pytest.mark.parametrize("rng", [(0, None), (1000, 2000)], ids=["whole", "a-range-that-cuts-components"])
def test_removal_keeps_the_rest_in_order_and_leaves_a_fresh_map(built, rng):
    first, n = rng
    pts = cc.scene()
    tol, sel = cc.SCENE_TOLS[1], dict(min_size=1, max_size=59)
    want = cc.restate(pts, first, n, tol=tol, **sel)
    gone = np.zeros(len(pts), bool)
    gone[first:first + len(want["mask"])] = want["mask"]
    assert 0 < gone.sum() < len(pts)
    if n is not None:                                                      # a selected component with members on both sides of the range's ends
        lab = cc.labels(pts, tol)
        cut = np.intersect1d(lab[gone], lab[~gone & cc.finish(lab, **sel)["mask"]])
        assert len(cut) > 10
    kept = pts[~gone]
    ctx, twin = _one(pts), _twin_of(kept)
    try:
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        removed, stats = ctx.map_remove_clusters(first, n, tol=tol, **sel)
        assert removed == int(gone.sum()) == stats["sel_points"] and stats == want["stats"]
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before
        _same_map(ctx, twin, kept, "after the removal")
        if n is None:                                                      # max_size was below every kept component's size: nothing left to select
            layout = ctx.grid_selfcheck()
            removed, stats = ctx.map_remove_clusters(tol=tol, **sel)
            assert removed == 0 and stats["sel_points"] == 0 and stats["sel_clusters"] == 0 and stats["n"] == len(kept)
            assert stats["clusters"] == want["stats"]["clusters"] - want["stats"]["sel_clusters"] and ctx.grid_selfcheck() == layout
        later = cc.small(257) + F(20.0)                                    # the map goes on: a later add lands in both alike
        ctx.map_add(later, stamp=0.9); twin.map_add(later, stamp=0.9)
        assert ctx.map_size() == twin.map_size()
        _same_map(ctx, twin, ctx.map_points().copy(), "an add after the removal")
    finally:
        ctx.close(); twin.close()


def test_removing_nothing_changes_nothing_and_removing_everything_empties_the_map(built):
    pts = cc.scene()
    N = len(pts)
    ctx = _one(pts)
    try:
        q = pts[::5]
        before = ctx.knn(q, 5)
        layout = ctx.grid_selfcheck()
        removed, stats = ctx.map_remove_clusters(tol=0.105, min_size=N + 1, max_size=0)         # a cfg that selects nothing
        assert removed == 0 and stats["sel_points"] == 0 and stats["sel_clusters"] == 0 and stats["n"] == N and stats["clusters"] > 1
        assert ctx.map_size() == N and ctx.grid_selfcheck() == layout                          # no build, no merge
        np.testing.assert_array_equal(ctx.map_points(), pts)
        for a, b in zip(before, ctx.knn(q, 5)):
            np.testing.assert_array_equal(a, b)
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        removed, stats = ctx.map_remove_clusters(tol=0.105, min_size=0, max_size=0)             # every component is selected
        assert removed == N == stats["sel_points"] and stats["sel_clusters"] == stats["clusters"]
        assert ctx.map_size() == 0 and len(ctx.map_points()) == 0
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before                                  # as a crop that removes everything
        i, s, c = ctx.knn_k(q[:10], 5)
        assert np.all(c == 0) and np.all(i == -1)
        out = ctx.map_clusters(tol=0.5)                                                        # the empty map, first = n = 0
        assert len(out["label"]) == 0 and out["stats"] == dict(n=0, clusters=0, largest=0, sel_clusters=0, sel_points=0)
        assert ctx.map_remove_clusters(tol=0.5) == (0, out["stats"])
        ctx.map_add(pts[:500], stamp=1.5)                                                      # and it takes points again
        assert ctx.map_size() == 500 and ctx.grid_selfcheck()[0] == 0
        cc.same(ctx.map_clusters(tol=0.2), cc.restate(pts[:500], tol=0.2), "after the refill")
    finally:
        ctx.close()


def test_after_a_carve_the_removal_is_the_restatements(built):
    """The scene of tests/test_gpu_carve.py's departed object, carved with the standard cfg, then remove_clusters(min_size = 1,
    max_size = m - 1) at CARVE_TOL = 0.2, m = M_CARVE = 8.  tests/test_clusters_host.py shows on the restatement that no tol and m
    separate the residue from this sparse structure (the residue hangs on the floor); what is asserted here is what the definition
    gives on the carved map, exactly: 31 residue and 7 810 structure points go, every one from a component of fewer than 8."""
    import carve_common as cv
    static, ghost, scan, x26, sensor = cv.standard_scene()
    kept, is_ghost = cc.carve_residue_scene()
    ctx = _one(np.concatenate([static, ghost]).astype(F))
    try:
        ctx.scan_set(scan)
        assert ctx.map_carve(x26, sensor, **cv.STD_CFG) == 316
        np.testing.assert_array_equal(ctx.map_points(), kept)
        want = cc.restate(kept, tol=cc.CARVE_TOL, min_size=1, max_size=cc.M_CARVE - 1)
        cc.same(ctx.map_clusters(tol=cc.CARVE_TOL, min_size=1, max_size=cc.M_CARVE - 1), want, "after the carve")
        removed, stats = ctx.map_remove_clusters(tol=cc.CARVE_TOL, min_size=1, max_size=cc.M_CARVE - 1)
        assert removed == 31 + 7810 == stats["sel_points"] and stats == want["stats"]
        assert int(want["mask"][is_ghost].sum()) == 31
        np.testing.assert_array_equal(ctx.map_points(), kept[~want["mask"]])
        left = ctx.map_clusters(tol=cc.CARVE_TOL)
        assert left["size"].min() >= cc.M_CARVE and ctx.grid_selfcheck()[0] == 0
    finally:
        ctx.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_and_map_are_untouched(std):
    from fast_limo_amd import _lib
    ctx, pts = std["ctx"], std["pts"]
    L, h = ctx._L, ctx._h
    n = len(pts)
    layout = ctx.grid_selfcheck()
    K = lambda **kw: _lib.cluster_cfg(**dict(dict(tol=0.5, min_size=1, max_size=0), **kw))
    cases = [("null cfg", None, 0, n), ("range beyond the map", K(), 0, n + 1), ("first beyond the map", K(), n + 1, 0),
             ("first + n wraps", K(), 2, 2 ** 64 - 1), ("nan tol", K(tol=np.nan), 0, n), ("negative tol", K(tol=-0.5), 0, n),
             ("infinite tol", K(tol=INF), 0, n), ("min_size -1", K(min_size=-1), 0, n), ("max_size -1", K(max_size=-1), 0, n),
             ("max_size below min_size", K(min_size=5, max_size=4), 0, n), ("nan tol, n 0", K(tol=np.nan), 0, 0),
             ("max_size below min_size, n 0", K(min_size=3, max_size=1), 5, 0)]
    for what, k, first, cnt_n in cases:
        kp = None if k is None else C.byref(k)
        label, size, mask = np.full(n + 1, 7, np.int32), np.full(n + 1, 7, np.int32), np.full(n + 1, 7, np.uint8)
        st = _lib.ClusterStats(n=9, clusters=9, largest=9, sel_clusters=9, sel_points=9)
        removed = C.c_size_t(5)
        assert L.flimo_map_clusters(h, first, cnt_n, kp, label.ctypes.data, size.ctypes.data, mask.ctypes.data, C.byref(st)) == ERR_INVALID, what
        assert L.flimo_map_remove_clusters(h, first, cnt_n, kp, C.byref(removed), C.byref(st)) == ERR_INVALID, what
        assert np.all(label == 7) and np.all(size == 7) and np.all(mask == 7) and removed.value == 5, what
        assert st.as_dict() == dict(n=9, clusters=9, largest=9, sel_clusters=9, sel_points=9), what
    assert ctx.map_size() == n and ctx.grid_selfcheck() == layout
    np.testing.assert_array_equal(ctx.map_points(), pts)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_clusters(tol=-1.0)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_remove_clusters(0, n + 1, tol=0.5)
    # equal bounds are a valid window; n = 0 fills the whole map's fields
    out = ctx.map_clusters(n, 0, tol=cc.SCENE_TOLS[1], min_size=3, max_size=3)
    want = cc.finish(std["labels"][cc.SCENE_TOLS[1]], n, 0, min_size=3, max_size=3)
    assert out["stats"] == want["stats"] and out["stats"]["n"] == 0 and out["stats"]["sel_points"] == 0 and out["stats"]["clusters"] > 0


# ---- 6. the Localizer's forms ---------------------------------------------------------------------------------------------------------
def test_the_localizer_forms_equal_the_contexts(built):
    from fast_limo_amd import api
    cfg = dict(tol=0.105, min_size=1, max_size=59)
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        out = loc.map_clusters(**cfg)                                # no map yet: an empty one's answer
        assert len(out["label"]) == 0 and out["stats"] == dict(n=0, clusters=0, largest=0, sel_clusters=0, sel_points=0)
        assert loc.map_remove_clusters(**cfg)[0] == 0
        with pytest.raises(api.FlimoError):
            loc.map_clusters(0, 5, **cfg)
        with pytest.raises(api.FlimoError):
            loc.map_clusters(tol=-1.0)
        loc.map_add(cc.scene())
        n = loc.map_size()
        pts = loc.hip.map_points().copy()
        a, b = loc.map_clusters(**cfg), loc.hip.map_clusters(**cfg)
        assert _sig(a) == _sig(b) and a["stats"]["n"] == n
        cc.same(a, cc.restate(pts, **cfg), "localizer")
        a, b = loc.map_clusters(n - 300, 200, want=("mask",), **cfg), loc.hip.map_clusters(n - 300, 200, want=("mask",), **cfg)
        assert sorted(a) == ["mask", "stats"] and a["stats"] == b["stats"]
        np.testing.assert_array_equal(a["mask"], b["mask"])
        whole = loc.hip.map_clusters(**cfg)
        removed, stats = loc.map_remove_clusters(**cfg)
        assert removed == whole["stats"]["sel_points"] == stats["sel_points"] > 0 and stats == whole["stats"]
        assert loc.map_size() == n - removed
        np.testing.assert_array_equal(loc.hip.map_points(), pts[~whole["mask"]])
        assert loc.hip.grid_selfcheck()[0] == 0
    finally:
        loc.close()
