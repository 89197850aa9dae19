"""Voxel statistics and thinning of the stored points on the GPU (flimo_map_voxels, flimo_map_voxel_mask, flimo_map_thin) against
the definition restated in numpy (tests/voxels_common.py): every integer with no tolerance, every float64 of centroid and cov bit
for bit.  Maps of at most 17 000 points."""
import ctypes as C
import itertools

import numpy as np
import pytest

import voxels_common as vc
from common import CAPS
from radius_common import bits

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5
F = np.float32
D = np.float64
ALL = ("ijk", "count", "first", "rep", "centroid", "cov")
PLANS = (1, 2, 3, 4, 8, 9, 11, 12)      # groups of 8, 16, 64 lanes, the many-runs path; + 8: through the sorted copy
RULES = (dict(keep=vc.KEEP_FIRST, max_pts=1), dict(keep=vc.KEEP_FIRST, max_pts=3), dict(keep=vc.KEEP_NEAREST, max_pts=1))


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_voxels", "flimo_map_voxel_mask", "flimo_map_thin", "flimo_voxel_key_host", "flimo_set_voxel_plan"):
        getattr(L, name)
    for name in ("flimo_loc_map_voxels", "flimo_loc_map_voxel_mask", "flimo_loc_map_thin"):
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


def _whole(ctx, pts, what="", first=0, n=None, **cfg):
    """Both read-only calls against the restatement; returns (got voxels, got mask, want)."""
    want = vc.restate(pts, first=first, n=n, **cfg)
    got = ctx.map_voxels(want=ALL, **cfg)
    whole = vc.restate(pts, **cfg) if (first, n) != (0, None) else want
    vc.same(got, dict(whole, stats=whole["stats"]), what + " voxels")
    gm = ctx.map_voxel_mask(first=first, n=n, **cfg)
    vc.same(gm, want, what + " mask")
    return got, gm, want


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_tiny_maps(built, n):
    pts = vc.small(n)
    ctx = _one(pts)
    try:
        for cfg in RULES:
            _whole(ctx, pts, "n %d" % n, leaf=0.25, **cfg)
        got, _, want = _whole(ctx, pts, "one voxel", leaf=64.0, keep=vc.KEEP_NEAREST)      # everything in at most 8 voxels around the origin
        assert got["nv"] <= 8 and got["count"].sum() == n
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def std(built):
    """The scene in one batch and in five, the stored points of each, computed once."""
    pts = vc.scene()
    one = _one(pts)
    cuts = [0, 900, 2500, 2600, 5000, len(pts)]
    five = _ctx([pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])], downsample=False)
    stored5 = five.map_points().copy()
    assert 4000 <= len(stored5) <= len(pts)
    yield dict(one=one, pts=pts, five=five, pts5=stored5)
    one.close(); five.close()


@pytest.mark.parametrize("leaf", vc.SCENE_LEAVES)
def test_the_scene_in_one_batch_and_in_five(std, leaf):
    for ctx, pts, what in ((std["one"], std["pts"], "one batch"), (std["five"], std["pts5"], "five batches")):
        for cfg in RULES:
            got, gm, want = _whole(ctx, pts, "%s leaf %g" % (what, leaf), leaf=leaf, **cfg)
        print(what, "leaf", leaf, "voxels", got["nv"], "largest", got["stats"]["largest"], "nearest goes", gm["stats"]["sel_points"])
        assert got["stats"]["outside"] == 0 and got["count"].sum() == len(pts)
        assert not np.signbit(got["cov"][:, [0, 3, 5]]).any()
    if np.array_equal(std["pts"], std["pts5"]):              # the same stored points: the batches moved nothing
        a, b = std["one"].map_voxels(want=ALL, leaf=leaf), std["five"].map_voxels(want=ALL, leaf=leaf)
        vc.same(a, b, "batches")


def test_voxels_of_exactly_1_to_4097_points(built):
    pts, which = vc.hand_voxels()
    ctx = _one(pts)
    try:
        for cfg in RULES:
            got, gm, want = _whole(ctx, pts, "hand", leaf=0.5, **cfg)
        assert got["count"].tolist() == list(vc.HAND_COUNTS) and got["ijk"][:, 0].tolist() == [3 * t - 15 for t in range(len(vc.HAND_COUNTS))]
        np.testing.assert_array_equal(got["ijk"][gm["voxel"], 0], which)
        assert gm["stats"]["sel_points"] == len(pts) - len(vc.HAND_COUNTS)
        for plan in PLANS:
            ctx.set_voxel_plan(plan)
            vc.same(ctx.map_voxels(want=ALL, leaf=0.5, keep=vc.KEEP_NEAREST), want, "plan %d" % plan)
        ctx.set_voxel_plan(0)
        # the sums in plain Python floats, for the voxels of 65 and 4097 points
        cen, cov, near = vc.restate_plain(pts, 0.5)
        np.testing.assert_array_equal(bits(got["centroid"]), bits(cen))
        np.testing.assert_array_equal(bits(got["cov"]), bits(cov))
        np.testing.assert_array_equal(got["rep"], near)
    finally:
        ctx.close()


def test_a_whole_map_in_one_voxel(built):
    pts = vc.one_voxel()
    ctx = _one(pts)
    try:
        got, gm, want = _whole(ctx, pts, "one voxel", leaf=4.0, keep=vc.KEEP_NEAREST)
        assert got["nv"] == 1 and got["count"].tolist() == [len(pts)] and got["stats"]["largest"] == len(pts) and got["first"].tolist() == [0]
        assert gm["mask"].sum() == len(pts) - 1 and not gm["mask"][got["rep"][0]]
        for plan in PLANS:
            ctx.set_voxel_plan(plan)
            vc.same(ctx.map_voxels(want=ALL, leaf=4.0, keep=vc.KEEP_NEAREST), want, "plan %d" % plan)
        ctx.set_voxel_plan(0)
        _whole(ctx, pts, "first 100", leaf=4.0, keep=vc.KEEP_FIRST, max_pts=100)
    finally:
        ctx.close()


def test_a_dyadic_lattice_by_hand(built):
    pts = vc.dyadic_lattice()
    ctx = _one(pts)
    try:
        got, gm, _ = _whole(ctx, pts, "dyadic", leaf=1.0, keep=vc.KEEP_NEAREST)
        assert got["ijk"].tolist() == [[0, 0, 0], [1, 0, 0]] and got["count"].tolist() == [8, 4]
        assert got["centroid"].tolist() == [[0.5, 0.5, 0.5], [1.4375, 0.4375, 0.5]]
        assert got["cov"].tolist() == [[0.0625, 0.0, 0.0, 0.0625, 0.0, 0.0625], [0.04296875, -0.01953125, 0.0, 0.04296875, 0.0, 0.0]]
        assert not np.signbit(got["cov"][0]).any()           # exact cancellation to +0.0
        assert got["rep"].tolist() == [0, 11]                # eight members equally far: the smallest index wins
        assert gm["mask"].tolist() == [False] + [True] * 10 + [False]
        for plan in PLANS:
            ctx.set_voxel_plan(plan)
            assert ctx.map_voxels(want=("rep",), leaf=1.0, keep=vc.KEEP_NEAREST)["rep"].tolist() == [0, 11]
    finally:
        ctx.close()


def test_three_hundred_exact_duplicates(built):
    pts = vc.duplicates()
    ctx = _one(pts)
    try:
        for cfg in RULES:
            got, gm, want = _whole(ctx, pts, "duplicates", leaf=0.5, **cfg)
        v = gm["voxel"][200]
        assert got["count"][v] >= 300 and np.all(gm["voxel"][200:500] == v)
        assert gm["mask"][200:500].sum() >= 299              # (KEEP_NEAREST, the last rule: at most the first of the copies stays)
    finally:
        ctx.close()


def test_a_map_ten_kilometres_away(built):
    pts = vc.far_away()
    ctx = _one(pts)
    try:
        for leaf in (0.25, 1.0):
            got, _, _ = _whole(ctx, pts, "far leaf %g" % leaf, leaf=leaf, keep=vc.KEEP_NEAREST)
            assert got["stats"]["outside"] == 0 and np.all(got["ijk"][:, 0] >= int(10000 / leaf) - 1) and np.all(got["ijk"][:, 1] < 0)
            # two passes: the covariance stays small and non-negative on the diagonal where E[xx] - E[x]^2 would have lost it
            assert np.all(got["cov"][:, [0, 3, 5]] >= 0) and got["cov"][:, [0, 3, 5]].max() <= leaf * leaf
    finally:
        ctx.close()


def test_points_outside_the_lattice(built):
    pts = vc.with_outside()
    ctx = _one(pts)
    try:
        far = np.abs(pts[:, 0]) > 1100
        for cfg in RULES:
            got, gm, want = _whole(ctx, pts, "outside", leaf=0.001, **cfg)
            assert got["stats"]["outside"] == far.sum() == 40 and np.all((gm["voxel"] == -1) == far) and not gm["mask"][far].any()
            assert got["count"].sum() == len(pts) - 40
        removed, st = ctx.map_thin(leaf=5.0, keep=vc.KEEP_FIRST, max_pts=1)      # a coarse leaf: everything inside, heavy thinning
        assert st["outside"] == 0 and removed == st["sel_points"] > 500
        ctx.map_clear(); ctx.map_add(pts, stamp=0.5)
        removed, st = ctx.map_thin(leaf=0.001, keep=vc.KEEP_NEAREST)             # the fine leaf: the outside points are never removed
        want = vc.restate(pts, leaf=0.001, keep=vc.KEEP_NEAREST)
        assert removed == want["stats"]["sel_points"] and st == want["stats"]
        kept = ctx.map_points()
        np.testing.assert_array_equal(kept, pts[~want["mask"]])
        assert (np.abs(kept[:, 0]) > 1100).sum() == 40
    finally:
        ctx.close()


# ---- 2. invariance ----------------------------------------------------------------------------------------------------------------------
def test_no_bit_moves_with_the_plan_the_cell_size_or_what_came_before(std):
    pts = std["pts"]
    want = vc.restate(pts, leaf=0.25, keep=vc.KEEP_NEAREST)
    ctx = std["one"]
    for plan in PLANS:
        ctx.set_voxel_plan(plan)
        vc.same(ctx.map_voxels(want=ALL, leaf=0.25, keep=vc.KEEP_NEAREST), want, "plan %d" % plan)
        vc.same(ctx.map_voxel_mask(leaf=0.25, keep=vc.KEEP_NEAREST), want, "plan %d mask" % plan)
    ctx.set_voxel_plan(0)
    for bad in (-1, 5, 7, 13, 16):
        with pytest.raises(Exception, match="invalid"):
            ctx.set_voxel_plan(bad)
    for cell in (0.3, 0.8, 2.5):
        other = _one(pts, cell)
        try:
            other.map_voxels(want=ALL, leaf=1.0)             # a larger call made before
            other.map_voxel_mask(leaf=0.1, keep=vc.KEEP_NEAREST)
            vc.same(other.map_voxels(want=ALL, leaf=0.25, keep=vc.KEEP_NEAREST), want, "cell %g" % cell)
        finally:
            other.close()


def test_reversing_the_insertion_order(std):
    pts = std["pts"]
    rev = np.ascontiguousarray(pts[::-1])
    ctx = _one(rev)
    try:
        a = std["one"].map_voxels(want=ALL, leaf=0.25)
        got, _, want = _whole(ctx, rev, "reversed", leaf=0.25, keep=vc.KEEP_NEAREST)
        np.testing.assert_array_equal(got["ijk"], a["ijk"])
        np.testing.assert_array_equal(got["count"], a["count"])
        # (the centroid's bits are the restatement's for the new order -- _whole above; a dozen widened float32 of one size add
        #  exactly in float64, so here they are also the old order's, and the covariance's products are not exact: only close)
        np.testing.assert_array_equal(bits(got["centroid"]), bits(a["centroid"]))
        assert np.abs(got["cov"] - a["cov"]).max() < 1e-12
        g = vc.group(pts, 0.25)                              # the oldest member of the new order is the youngest of the old
        np.testing.assert_array_equal(got["first"], len(pts) - 1 - g["order"][g["start"] + g["count"] - 1])
    finally:
        ctx.close()


def test_range_forms(std):
    ctx, pts = std["one"], std["pts"]
    N = len(pts)
    for first, n in ((0, 0), (0, 1), (1000, 3000), (N - 257, 257), (N, 0)):
        for cfg in RULES:
            want = vc.restate(pts, first=first, n=n, leaf=0.25, **cfg)
            vc.same(ctx.map_voxel_mask(first=first, n=n, leaf=0.25, **cfg), want, "range %d + %d" % (first, n))
            assert want["stats"]["voxels"] > 300            # the voxels of the whole map, whatever the range
    # KEEP_FIRST over a range of late points drops exactly those beyond rank m
    m, first = 2, 4000
    got = ctx.map_voxel_mask(first=first, leaf=0.25, keep=vc.KEEP_FIRST, max_pts=m)
    whole = ctx.map_voxel_mask(leaf=0.25, keep=vc.KEEP_FIRST, max_pts=m)
    older = np.array([np.sum(whole["voxel"][:i] == whole["voxel"][i]) for i in range(first, N)])
    np.testing.assert_array_equal(got["mask"], older >= m)
    assert 0 < got["mask"].sum() < N - first


def test_cap_and_every_combination_of_outputs(std):
    from fast_limo_amd import _lib
    ctx, pts = std["one"], std["pts"]
    L, h = ctx._L, ctx._h
    cfg = dict(leaf=0.25, keep=vc.KEEP_NEAREST)
    want = vc.restate(pts, **cfg)
    nv = want["nv"]
    k = _lib.voxel_cfg(**cfg)
    for names in itertools.chain.from_iterable(itertools.combinations(ALL, r) for r in range(len(ALL) + 1)):
        got = ctx.map_voxels(want=names, **cfg)
        assert sorted(got) == sorted(names + ("nv", "stats"))
        vc.same(got, want, "outputs %s" % (names,))
    for keep in (vc.KEEP_FIRST, vc.KEEP_NEAREST):            # no moments asked for, rep alone
        got = ctx.map_voxels(want=("rep",), leaf=0.25, keep=keep)
        vc.same(got, vc.restate(pts, leaf=0.25, keep=keep), "rep alone")
    for names in ((), ("voxel",), ("mask",), ("voxel", "mask")):
        vc.same(ctx.map_voxel_mask(want=names, **cfg), want, "mask outputs %s" % (names,))
    # everything NULL: the count alone; and nothing at all
    got_nv = C.c_size_t(0)
    assert L.flimo_map_voxels(h, C.byref(k), 0, C.byref(got_nv), None, None, None, None, None, None, None) == 0 and got_nv.value == nv
    assert L.flimo_map_voxels(h, C.byref(k), 0, None, None, None, None, None, None, None, None) == 0
    assert L.flimo_map_voxel_mask(h, 0, len(pts), C.byref(k), None, None, None) == 0
    # cap one below, at and above nv
    for cap, rc in ((nv - 1, ERR_TOO_LARGE), (nv, 0), (nv + 1, 0)):
        count, cen = np.full(nv + 2, 7, np.int32), np.full((nv + 2, 3), 7.0)
        got_nv = C.c_size_t(0)
        st = _lib.VoxelStats(7, 7, 7, 7, 7)
        assert L.flimo_map_voxels(h, C.byref(k), cap, C.byref(got_nv), None, count.ctypes.data, None, None, cen.ctypes.data, None, C.byref(st)) == rc
        assert got_nv.value == nv                           # always written
        if rc:
            assert np.all(count == 7) and np.all(cen == 7) and st.n == 7
        else:
            np.testing.assert_array_equal(count[:nv], want["count"])
            np.testing.assert_array_equal(bits(cen[:nv]), bits(want["centroid"]))
            assert np.all(count[nv:] == 7) and np.all(cen[nv:] == 7) and st.as_dict() == want["stats"]


def test_against_the_scans_voxel_filter(std):
    """The same cloud as a scan through flimo_scan_voxel_filter: the same voxels in the same order; its centroid is a float32
    running sum, so each component differs by at most (c + 1) * 2^-24 * max |coordinate|."""
    ctx, pts = std["one"], std["pts"]
    for leaf in (0.25, 1.0):
        got = ctx.map_voxels(want=("count", "centroid"), leaf=leaf)
        ctx.scan_set(pts)
        n = ctx.scan_voxel_filter(leaf)
        cloud = ctx.scan_get()
        assert n == got["nv"] == len(cloud)
        bound = (got["count"] + 1.0) * 2.0 ** -24 * float(np.abs(pts).max())
        err = np.abs(cloud.astype(D) - got["centroid"]).max(axis=1)
        print("leaf", leaf, "voxels", n, "largest difference / bound", float((err / bound).max()))
        assert np.all(err <= bound)


# ---- 3. thinning ----------------------------------------------------------------------------------------------------------------------
def _twin_of(kept):
    twin = _ctx([vc.scene()[:100]])
    twin.map_clear()
    if len(kept):
        twin.map_add(kept, stamp=0.5)
    return twin


def _same_map(ctx, twin, kept, what):
    from fast_limo_amd import _lib, synth
    assert ctx.map_size() == twin.map_size() == len(kept), what
    np.testing.assert_array_equal(ctx.map_points(), kept, err_msg=what)
    np.testing.assert_array_equal(twin.map_points(), kept, err_msg=what)
    assert ctx.grid_selfcheck()[0] == 0 and twin.grid_selfcheck()[0] == 0, what
    q = np.concatenate([kept[:: max(len(kept) // 100, 1)][:100], kept[:: max(len(kept) // 100, 1)][:100] + F(0.03)])
    (i, s, c), (ti, ts, tc) = ctx.knn_k(q, 12, 3.0), twin.knn_k(q, 12, 3.0)
    np.testing.assert_array_equal(i, ti, err_msg=what)
    np.testing.assert_array_equal(bits(s), bits(ts), err_msg=what)
    np.testing.assert_array_equal(c, tc, err_msg=what)
    for a, b in zip(ctx.radius_search(q, 0.4, sorted=True), twin.radius_search(q, 0.4, sorted=True)):
        assert a.tobytes() == b.tobytes(), what
    scan = np.ascontiguousarray(synth.box_world_scan_random(2048, 6.0, 2)[:, :3])
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    ctx.scan_set(scan); twin.scan_set(scan)
    for a, b in zip(ctx.match_reduce(x, mcfg), twin.match_reduce(x, mcfg)):      # one registration pass
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), what
    a, b = ctx.map_voxels(want=ALL, leaf=0.5), twin.map_voxels(want=ALL, leaf=0.5)
    vc.same(a, b, what)


@pytest.mark.parametrize("case", [(0, None, RULES[0]), (0, None, RULES[1]), (0, None, RULES[2]), (3000, 2500, RULES[0]), (3000, 2500, RULES[2])],
                         ids=["first-1", "first-3", "nearest", "range-first-1", "range-nearest"])
def test_thinning_keeps_the_rest_in_order_and_leaves_a_fresh_map(built, case):
    first, n, cfg = case
    pts = vc.scene()
    want = vc.restate(pts, first=first, n=n, leaf=0.25, **cfg)
    gone = np.zeros(len(pts), bool)
    gone[first:first + len(want["mask"])] = want["mask"]
    kept = pts[~gone]
    ctx, twin = _one(pts), _twin_of(kept)
    try:
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        removed, st = ctx.map_thin(first=first, n=n, leaf=0.25, **cfg)
        assert removed == st["sel_points"] == int(gone.sum()) > 100 and st == want["stats"]
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before
        _same_map(ctx, twin, kept, "after the thinning")
        after = ctx.map_voxels(want=("count",), leaf=0.25, **cfg)
        if n is None:
            assert after["nv"] == want["nv"] and after["stats"]["largest"] <= cfg["max_pts"]
            assert after["stats"]["sel_points"] == 0
        if n is None:                                        # a second thinning removes nothing and changes nothing
            layout = ctx.grid_selfcheck()
            assert ctx.map_thin(leaf=0.25, **cfg)[0] == 0 and ctx.grid_selfcheck() == layout
            np.testing.assert_array_equal(ctx.map_points(), kept)
            later = vc.small(257) + F(20.0)                  # the map goes on: a later add lands in both alike
            ctx.map_add(later, stamp=0.9); twin.map_add(later, stamp=0.9)
            _same_map(ctx, twin, ctx.map_points().copy(), "an add after the thinning")
        else:                                                # (the range's indices are renumbered: thin the whole map, then again)
            ctx.map_thin(leaf=0.25, **cfg)
            assert ctx.map_thin(leaf=0.25, **cfg)[0] == 0
    finally:
        ctx.close(); twin.close()


def test_the_read_only_calls_change_neither_map_nor_scan_nor_a_later_pass(built):
    from fast_limo_amd import _lib, synth
    import outliers_common as oc
    mp = oc.scene()
    scan = np.ascontiguousarray(synth.box_world_scan_random(4096, 12.0, 2)[:, :3])
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    q = mp[::9]

    def run(voxels):
        h = _one(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if voxels:
                assert h.map_voxels(want=ALL, leaf=0.3, keep=vc.KEEP_NEAREST)["nv"] > 100
                h.set_voxel_plan(12)
                assert h.map_voxel_mask(leaf=1.0, keep=vc.KEEP_NEAREST)["stats"]["sel_points"] > 0
                removed, st = h.map_thin(first=0, n=0, leaf=0.3)      # an empty range: the whole map's figures, nothing selected
                assert removed == 0 and st["n"] == st["sel_points"] == 0 and st["voxels"] > 100
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


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_and_map_are_untouched(std):
    from fast_limo_amd import _lib
    ctx, pts = std["one"], std["pts"]
    L, h = ctx._L, ctx._h
    n = len(pts)
    layout = ctx.grid_selfcheck()
    K = lambda **kw: _lib.voxel_cfg(**vc.cfg_of(**kw))
    cases = [("null cfg", None, 0, n)] + [(str(bad), K(**bad), 0, n) for bad in vc.BAD_CFGS] + \
            [("range beyond the map", K(), 0, n + 1), ("first beyond the map", K(), n + 1, 0), ("first + n wraps", K(), 2, 2 ** 64 - 1),
             ("nan leaf, n 0", K(leaf=float("nan")), 0, 0)]
    for what, k, first, cnt_n in cases:
        kp = None if k is None else C.byref(k)
        voxel, mask, removed = np.full(n + 1, 7, np.int32), np.full(n + 1, 7, np.uint8), C.c_size_t(5)
        st = _lib.VoxelStats(7, 7, 7, 7, 7)
        assert L.flimo_map_voxel_mask(h, first, cnt_n, kp, voxel.ctypes.data, mask.ctypes.data, C.byref(st)) == ERR_INVALID, what
        assert L.flimo_map_thin(h, first, cnt_n, kp, C.byref(removed), C.byref(st)) == ERR_INVALID, what
        assert np.all(voxel == 7) and np.all(mask == 7) and removed.value == 5 and st.voxels == 7, what
        if first == 0 and cnt_n == n:
            count, cen, nv = np.full(n, 7, np.int32), np.full((n, 3), 7.0), C.c_size_t(5)
            assert L.flimo_map_voxels(h, kp, n, C.byref(nv), None, count.ctypes.data, None, None, cen.ctypes.data, None, C.byref(st)) == ERR_INVALID, what
            assert np.all(count == 7) and np.all(cen == 7) and nv.value == 5 and st.voxels == 7, what
    assert ctx.map_size() == n and ctx.grid_selfcheck() == layout
    np.testing.assert_array_equal(ctx.map_points(), pts)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_thin(leaf=-1.0)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_voxel_mask(first=0, n=n + 1)
    vc.same(ctx.map_voxels(want=ALL, leaf=0.25), vc.restate(pts, leaf=0.25), "after the refusals")


def test_the_empty_map(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    try:
        none = dict(n=0, voxels=0, largest=0, outside=0, sel_points=0)
        got = ctx.map_voxels(want=ALL, leaf=0.25)
        assert got["nv"] == 0 and got["stats"] == none and all(len(got[k]) == 0 for k in ALL)
        assert ctx.map_voxel_mask(leaf=0.25)["stats"] == none and ctx.map_thin(leaf=0.25) == (0, none)
        with pytest.raises(_lib.FlimoError, match="invalid"):
            ctx.map_voxel_mask(first=0, n=1, leaf=0.25)
    finally:
        ctx.close()


# ---- 5. the Localizer's forms ---------------------------------------------------------------------------------------------------------
def test_the_localizer_forms_equal_the_contexts(built):
    from fast_limo_amd import api
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        none = dict(n=0, voxels=0, largest=0, outside=0, sel_points=0)
        assert loc.map_voxels(leaf=0.5)["nv"] == 0 and loc.map_voxel_mask(leaf=0.5)["stats"] == none and loc.map_thin(leaf=0.5) == (0, none)
        assert loc.voxel_cloud(0.5).shape == (0, 3)
        with pytest.raises(api.FlimoError):
            loc.map_voxel_mask(first=0, n=5, leaf=0.5)
        with pytest.raises(api.FlimoError):
            loc.map_voxels(leaf=0.0)
        loc.map_add(vc.scene())
        n = loc.map_size()
        pts = loc.hip.map_points().copy()
        cfg = dict(leaf=0.25, keep=vc.KEEP_NEAREST)
        want = vc.restate(pts, **cfg)
        a, b = loc.map_voxels(want=ALL, **cfg), loc.hip.map_voxels(want=ALL, **cfg)
        vc.same(a, b, "localizer"); vc.same(a, want, "localizer")
        vc.same(loc.map_voxel_mask(**cfg), want, "localizer mask")
        cloud = loc.voxel_cloud(0.25)
        assert cloud.dtype == F and cloud.shape == (want["nv"], 3)
        np.testing.assert_array_equal(cloud, want["centroid"].astype(F))
        removed, st = loc.map_thin(**cfg)
        assert removed == want["stats"]["sel_points"] == st["sel_points"] and loc.map_size() == n - removed == want["nv"]
        np.testing.assert_array_equal(loc.hip.map_points(), pts[~want["mask"]])
        assert loc.hip.grid_selfcheck()[0] == 0
    finally:
        loc.close()
