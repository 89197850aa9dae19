"""GPU suite: smooth-surface regions of the stored points -- flimo_map_regions labels every stored point with the smallest insertion
index among the smooth points of its region (neighbours closer than tol whose normals agree), flimo_map_region_list lists the selected
regions with float64 centroid and covariance in the voxels' summation shape, flimo_map_remove_regions forgets the points of selected
regions in the crop's one ordered pass.  The yardstick is the definition restated in numpy (tests/regions_common.py), fed with the
SAME context's normals_range output: the predicates are float32 arithmetic that numpy reproduces bit for bit and every integer has
one correct value given the normals, so label, size, mask, stats and the listing's integers are compared with NO tolerance, centroid
and cov bit for bit.  After a removal the map is clear() + initialize(kept), as after a crop: checked against a twin context."""
import ctypes as C
import itertools

import numpy as np
import pytest

import clusters_common as cc
import regions_common as rc
from common import CAPS
from radius_common import bits

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_TOO_LARGE = -2, -6, -5
F = np.float32
INF = float("inf")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_regions", "flimo_map_region_list", "flimo_map_remove_regions", "flimo_set_region_chunk", "flimo_region_joined_host"):
        getattr(L, name)
    for name in ("flimo_loc_map_regions", "flimo_loc_map_region_list", "flimo_loc_map_remove_regions"):
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


def _normals(ctx, **cfg):
    """The context's own normals of the whole map: the restatement's input."""
    k = rc.cfg_of(**cfg)
    n = ctx.map_size()
    return ctx.normals_range(0, n, k["normal_k"], k["normal_max_dist"], k["normal_min_pts"], want=())["normal"] if n else np.zeros((0, 4), F)


def _want(ctx, pts, first=0, n=None, **cfg):
    return rc.restate(pts, _normals(ctx, **cfg), first, n, **cfg)


def _sig(out):
    return tuple(out[k].tobytes() for k in ("label", "size", "mask")) + tuple(out["stats"][k] for k in rc.STATS)


def _lsig(out):
    return tuple(out[k].tobytes() for k in ("label", "count", "first", "centroid", "cov")) + (out["nr"],) + tuple(out["stats"][k] for k in rc.STATS)


ALL5 = ("label", "count", "first", "centroid", "cov")


@pytest.fixture(scope="module")
def std(built):
    """The standard scene in three batches (insertion order and cell order differ), its stored points, the context's normals at both
    neighbourhood sizes and the whole map's labels per setting, computed once."""
    pts = rc.scene()
    ctx = _ctx([pts[:2500], pts[2500:4100], pts[4100:]], downsample=False)
    stored = ctx.map_points().copy()
    np.testing.assert_array_equal(stored, pts)
    nrm = {k: _normals(ctx, normal_k=k) for k in (16, 10)}
    labels = [rc.labels(stored, nrm[s["normal_k"]], **rc.cfg_of(**s)) for s in rc.SETTINGS]
    yield dict(ctx=ctx, pts=stored, nrm=nrm, labels=labels)
    ctx.close()


def _fin(std, which, first=0, n=None, **sel):
    s = rc.SETTINGS[which]
    out = rc.finish(std["labels"][which], std["nrm"][s["normal_k"]], s["max_curv"], first, n, **sel)
    out.pop("sel_all")
    return out


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257])
def test_small_maps_at_the_edges_of_groups_and_blocks(built, n):
    pts = cc.small(n)
    ctx = _one(pts)
    try:
        for cfg in (dict(tol=0.5, normal_k=8, min_cos=0.5, max_curv=0.2, border=1), dict(tol=0.5, normal_k=8, min_cos=0.5, max_curv=0.2, border=0),
                    dict(tol=0.5, normal_k=5, min_cos=0.0, max_curv=INF, border=1, min_size=2, max_size=5), dict(tol=0.0, normal_k=8, max_curv=0.3),
                    dict(tol=50.0, normal_k=8, min_cos=0.0, max_curv=0.1, border=1, min_size=n, max_size=n)):
            want = _want(ctx, pts, **cfg)
            got = ctx.map_regions(**cfg)
            print(n, cfg, got["stats"])
            rc.same(got, want, "n %d %s" % (n, cfg))
            nrm = _normals(ctx, **cfg)
            rc.same_listing(ctx.map_region_list(want=ALL5, **cfg), rc.listing(pts, rc.labels(pts, nrm, **rc.cfg_of(**cfg)), nrm, **rc.cfg_of(**cfg)),
                            "list n %d %s" % (n, cfg))
    finally:
        ctx.close()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["k16-border0", "k16-border1", "k10-border1"])
def test_the_standard_scene_equals_the_restatement(std, which):
    ctx, s = std["ctx"], rc.SETTINGS[which]
    for sel in (dict(min_size=1, max_size=0), dict(min_size=100, max_size=0), dict(min_size=2, max_size=1500), dict(min_size=0, max_size=1)):
        want = _fin(std, which, **sel)
        got = ctx.map_regions(**s, **sel)
        print(s, sel, got["stats"], "plan", cc.plan(ctx.map_index_layout(), s["tol"]))
        rc.same(got, want, "%s %s" % (s, sel))
        li = rc.listing(std["pts"], std["labels"][which], std["nrm"][s["normal_k"]], s["max_curv"], **sel)
        rc.same_listing(ctx.map_region_list(want=ALL5, **s, **sel), li, "list %s %s" % (s, sel))
    assert got["stats"]["regions"] >= 4 and got["stats"]["unassigned"] > 0


def test_the_scene_is_recovered(std):
    """Setting 1 without the border: exactly four regions of at least 100 points, each with at least 99 % of its members on one
    surface, at least 4 500 of the 5 060 points in them (the restatement with numpy normals: 100 % and 4 748; the margin covers the
    device's eigenvectors differing from numpy's in rounding); flimo_map_clusters at the same tol: one component."""
    ctx, s = std["ctx"], rc.SETTINGS[0]
    got = ctx.map_regions(**s)
    big, purity, inside = rc.recovery(got["label"], rc.scene_surface())
    print("regions", [(int(r), int((got["label"] == r).sum())) for r in big], "purity", purity, "inside", inside, got["stats"])
    assert len(big) == 4 and min(purity) >= 0.99 and inside >= 4500
    surf = rc.scene_surface()
    assert sorted(int(np.bincount(surf[got["label"] == r], minlength=3).argmax()) for r in big) == [0, 0, 1, 2]      # floor twice: the disc
    assert ctx.map_clusters(tol=s["tol"])["stats"]["clusters"] == 1
    from fast_limo_amd import api
    li = ctx.map_region_list(min_size=100, **s)
    planes = api.region_planes(li)
    flat = [r for r in range(li["nr"]) if surf[li["label"][r]] != 2]
    assert len(flat) == 3 and np.all(planes["rms"][flat] < 0.02)          # the jitter is 1 cm
    for r in flat:
        axis = 0 if surf[li["label"][r]] == 1 else 2
        assert abs(planes["normal"][r][axis]) > 0.999 and abs(planes["d"][r]) < 0.05


def test_degenerate_settings(std):
    ctx, pts = std["ctx"], std["pts"]
    open_cfg = dict(tol=0.15, normal_k=16, min_cos=0.0, max_curv=INF, border=0)
    assert rc.has_normal(std["nrm"][16]).all()
    got, cl = ctx.map_regions(**open_cfg), ctx.map_clusters(tol=0.15)
    np.testing.assert_array_equal(got["label"], cl["label"])              # the Euclidean clusters of the points that have a normal
    np.testing.assert_array_equal(got["size"], cl["size"])
    assert got["stats"]["regions"] == cl["stats"]["clusters"] and got["stats"]["smooth"] == len(pts) and got["stats"]["unassigned"] == 0
    for tol in (0.06, 0.105):                                             # thousands of single points; the surfaces half joined
        got, cl = ctx.map_regions(**dict(open_cfg, tol=tol)), ctx.map_clusters(tol=tol)
        np.testing.assert_array_equal(got["label"], cl["label"])
        np.testing.assert_array_equal(got["size"], cl["size"])
    zero = dict(tol=0.0, normal_k=16, max_curv=0.05, border=1)
    got = ctx.map_regions(**zero)
    sm = rc.smooth(std["nrm"][16], 0.05)
    np.testing.assert_array_equal(got["label"], np.where(sm, np.arange(len(pts)), -1))
    np.testing.assert_array_equal(got["size"], sm.astype(np.int32))
    assert got["stats"] == dict(n=len(pts), smooth=int(sm.sum()), regions=int(sm.sum()), largest=1, sel_regions=int(sm.sum()),
                                unassigned=int((~sm).sum()), sel_points=int(sm.sum()))
    rc.same(got, _want(ctx, pts, **zero), "tol 0")
    # ... and the listing of thousands of one-point regions: more than the wrapper's first call has room for
    li = ctx.map_region_list(want=ALL5, **zero)
    rc.same_listing(li, rc.listing(pts, np.where(sm, np.arange(len(pts)), -1), std["nrm"][16], 0.05), "tol 0 list")
    assert li["nr"] == int(sm.sum()) > 1024 and np.all(li["count"] == 1) and np.all(li["cov"] == 0.0)
    np.testing.assert_array_equal(li["centroid"], pts[sm].astype(np.float64))


@pytest.mark.parametrize("k", [9, 16])
def test_a_tie_between_two_regions_goes_to_the_smaller_index(built, k):
    cfg = dict(rc.TIE_CFG, normal_k=k)
    seen = []
    for swap in (False, True):
        pts = rc.tie_case(swap)
        ctx = _one(pts)
        try:
            nrm = _normals(ctx, **cfg)
            # the premises, from the context's normals
            sm = rc.smooth(nrm, cfg["max_curv"])
            print(k, swap, "middle", nrm[128], "patches' curvature up to", float(np.abs(nrm[:128, 3]).max()))
            assert sm[:128].all() and not sm[128] and rc.has_normal(nrm)[128]
            d = cc.sqdist_block(pts, 128, 129)[0]
            near = np.argsort((rc.bits32(d).astype(np.uint64) << np.uint64(32)) | np.arange(129, dtype=np.uint64))[:3]
            assert near[0] == 128 and rc.bits32(d)[near[1]] == rc.bits32(d)[near[2]] and near[1] < 64 <= near[2]
            got = ctx.map_regions(**cfg)
            assert got["label"][near[1]] == 0 and got["label"][near[2]] == 64          # the candidates lie in different regions
            assert got["label"][128] == 0 and got["size"][128] == 65 and got["size"][64] == 64
            rc.same(got, _want(ctx, pts, **cfg), "tie")
            seen.append(float(pts[got["label"][128], 2]))
            assert ctx.map_regions(**dict(cfg, border=0))["label"][128] == -1
        finally:
            ctx.close()
    assert seen == [0.0, 1.0]                                             # swapping the patches moves it to the other patch


def test_points_without_a_normal_are_unassigned(built):
    pts = rc.gated_scene()
    ctx = _one(pts)
    try:
        cfg = dict(tol=0.15, normal_k=16, normal_max_dist=0.5, min_size=0)
        nrm = _normals(ctx, **cfg)
        lone = np.flatnonzero(~rc.has_normal(nrm))
        assert lone.tolist() == [2000, 2001, 5062, 5063, 5064]
        got = ctx.map_regions(**cfg)
        assert np.all(got["label"][lone] == -1) and np.all(got["size"][lone] == 0) and not got["mask"][lone].any()
        rc.same(got, _want(ctx, pts, **cfg), "gate")
        # a gate no neighbourhood fits in: nothing has a normal, nothing is assigned, nothing is removed
        none = ctx.map_regions(tol=0.15, normal_k=16, normal_max_dist=0.01, min_size=0)
        assert none["stats"] == dict(n=len(pts), smooth=0, regions=0, largest=0, sel_regions=0, unassigned=len(pts), sel_points=0)
        assert np.all(none["label"] == -1) and not none["mask"].any()
        assert ctx.map_remove_regions(tol=0.15, normal_k=16, normal_max_dist=0.01, min_size=0)[0] == 0 and ctx.map_size() == len(pts)
        assert ctx.map_region_list(tol=0.15, normal_k=16, normal_max_dist=0.01, min_size=0)["nr"] == 0
    finally:
        ctx.close()


def test_duplicates_and_a_map_ten_kilometres_away(built):
    pts = cc.duplicates()
    ctx = _one(pts)
    try:
        for cfg in (dict(tol=0.5, normal_k=16, min_cos=0.3, max_curv=0.2), dict(tol=1e-3, normal_k=16, min_cos=0.0, max_curv=INF),
                    dict(tol=0.0, normal_k=64, min_cos=0.0, max_curv=INF)):
            rc.same(ctx.map_regions(**cfg), _want(ctx, pts, **cfg), "duplicates %s" % cfg)
    finally:
        ctx.close()
    pts = rc.moved(rc.scene())
    ctx = _one(pts)
    try:
        for s in rc.SETTINGS[1:2]:
            got = ctx.map_regions(**s)
            rc.same(got, _want(ctx, pts, **s), "10 km %s" % s)
            nrm = _normals(ctx, **s)
            rc.same_listing(ctx.map_region_list(want=ALL5, min_size=50, **s),
                            rc.listing(pts, rc.labels(pts, nrm, **rc.cfg_of(**s)), nrm, s["max_curv"], min_size=50), "10 km list")
        assert got["stats"]["regions"] >= 3
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [("scene", 0.5, 0.3, "8"), ("scene", 0.5, 0.9, "16"), ("scene", 0.5, 1.3, "64"), ("scene", 0.125, 0.3, "64"),
                                  ("sparse", 0.5, 20.0, "tiles"), ("sparse", 0.5, 150.0, "tiles")], ids=lambda c: "%s-cell%g-tol%g-%s" % c)
def test_every_lane_plan(built, case):
    which, cell, tol, plan = case
    pts = rc.scene() if which == "scene" else cc.sparse()
    ctx = _one(pts, cell)
    try:
        assert cc.plan(ctx.map_index_layout(), tol) == plan
        cfg = dict(tol=tol, normal_k=10, min_cos=rc.COS20, max_curv=0.03, border=1, min_size=2) if which == "scene" else \
            dict(tol=tol, normal_k=5, min_cos=0.2 if tol < 100 else 0.5, max_curv=0.15 if tol < 100 else 0.1, border=1, min_size=2)
        want = _want(ctx, pts, **cfg)
        got = ctx.map_regions(**cfg)
        print(case, got["stats"])
        rc.same(got, want, str(case))
        assert got["stats"]["regions"] > 1 and got["stats"]["smooth"] < len(pts)
        if case[:3] != ("sparse", 0.5, 20.0):      # (there the five points of a group share one neighbourhood and no other group is near)
            assert got["stats"]["unassigned"] < len(pts) - got["stats"]["smooth"]      # the border attached some
        without = ctx.map_regions(**dict(cfg, border=0))
        sm = without["label"] >= 0                                                 # the border moves no smooth point's label
        np.testing.assert_array_equal(without["label"][sm], got["label"][sm])
        assert without["stats"]["unassigned"] == len(pts) - got["stats"]["smooth"]
    finally:
        ctx.close()


# ---- 2. invariance --------------------------------------------------------------------------------------------------------------------
def test_no_byte_moves_with_chunks_cell_batches_repetition_or_an_earlier_call(std):
    ctx, pts = std["ctx"], std["pts"]
    cfgs = [dict(s, min_size=50, max_size=1700) for s in rc.SETTINGS]
    run = lambda c: [_sig(c.map_regions(**cfg)) for cfg in cfgs] + [_lsig(c.map_region_list(want=ALL5, **cfg)) for cfg in cfgs]
    base = run(ctx)
    for which, b in enumerate(base[:3]):
        assert b == _sig(_fin(std, which, min_size=50, max_size=1700))
    assert run(ctx) == base                                               # a second call
    for chunk in (1, 7, 1000):
        ctx.set_region_chunk(chunk)
        try:
            assert run(ctx) == base, chunk
        finally:
            ctx.set_region_chunk(0)
    ctx.set_normals_chunk(999)                                            # a normals chunk smaller than the map
    try:
        assert run(ctx) == base
    finally:
        ctx.set_normals_chunk(0)
    for plan in (1, 2, 3, 4):                                             # the listing's moments under every forced lane plan
        ctx.set_voxel_plan(plan)
        try:
            assert run(ctx)[3:] == base[3:], plan
        finally:
            ctx.set_voxel_plan(0)
    ctx.map_regions(tol=1.0, normal_k=32, min_cos=0.0, max_curv=INF)      # a larger call before
    assert run(ctx) == base
    for cell in (0.25, 1.0):                                              # two cell sizes, each a second context, one batch
        other = _one(pts, cell)
        try:
            assert run(other) == base, cell
        finally:
            other.close()
    five = _ctx(np.array_split(pts, 5), downsample=False)                 # one batch against five
    try:
        np.testing.assert_array_equal(five.map_points(), pts)
        assert run(five) == base
    finally:
        five.close()


def test_a_range_is_the_slice_of_the_whole_map(std):
    ctx, N = std["ctx"], len(std["pts"])
    s, sel = rc.SETTINGS[1], dict(min_size=200, max_size=1700)
    whole = ctx.map_regions(**s, **sel)
    for first, n in ((0, N), (0, 1), (0, 777), (N // 2, 1000), (N - 1, 1), (N, 0), (17, 0)):      # ranges that cut every large region
        got = ctx.map_regions(first, n, **s, **sel)
        rc.same(got, _fin(std, 1, first, n, **sel), "range %d+%d" % (first, n))
        for key in ("label", "size", "mask"):
            np.testing.assert_array_equal(got[key], whole[key][first:first + n])
        assert got["stats"]["n"] == n and got["stats"]["regions"] == whole["stats"]["regions"]


def test_every_combination_of_null_outputs(std):
    from fast_limo_amd import _lib
    ctx, N = std["ctx"], len(std["pts"])
    L, h = ctx._L, ctx._h
    first, n = 100, N - 300
    s, sel = rc.SETTINGS[1], dict(min_size=200, max_size=1700)
    k = _lib.region_cfg(**s, **sel)
    want = _fin(std, 1, first, n, **sel)
    for wl, ws, wm, wst in itertools.product((False, True), repeat=4):
        label, size, mask = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8)
        st = _lib.RegionStats()
        rc_ = L.flimo_map_regions(h, first, n, C.byref(k), label.ctypes.data if wl else None, size.ctypes.data if ws else None,
                                  mask.ctypes.data if wm else None, C.byref(st) if wst else None)
        assert rc_ == 0
        if wl:
            np.testing.assert_array_equal(label, want["label"])
        if ws:
            np.testing.assert_array_equal(size, want["size"])
        if wm:
            np.testing.assert_array_equal(mask.astype(bool), want["mask"])
        if wst:
            assert st.as_dict() == want["stats"]
    li = rc.listing(std["pts"], std["labels"][1], std["nrm"][16], s["max_curv"], **sel)
    for r in range(6):
        for names in itertools.combinations(ALL5, r):
            got = ctx.map_region_list(want=names, **s, **sel)
            assert sorted(got) == sorted(names + ("nr", "stats"))
            rc.same_listing(got, li, str(names))
    assert sorted(ctx.map_regions(want=("size",), tol=0.1)) == ["size", "stats"]
    with pytest.raises(ValueError):
        ctx.map_regions(want=("label", "normals"), tol=0.1)
    with pytest.raises(ValueError):
        ctx.map_region_list(want=("rep",), tol=0.1)


# ---- 3. the listing -------------------------------------------------------------------------------------------------------------------
def test_cap_one_below_at_and_above_the_number_of_regions(std):
    from fast_limo_amd import _lib
    ctx = std["ctx"]
    L, h = ctx._L, ctx._h
    s, sel = rc.SETTINGS[1], dict(min_size=100, max_size=0)
    li = rc.listing(std["pts"], std["labels"][1], std["nrm"][16], s["max_curv"], **sel)
    m = li["nr"]
    assert m == 4
    k = _lib.region_cfg(**s, **sel)
    for cap in (m - 1, 0, m, m + 1, 5060):
        label, count, first = (np.full(cap + 2, -7, np.int32) for _ in range(3))
        cen, cov = np.full((cap + 2, 3), -7.0), np.full((cap + 2, 6), -7.0)
        nr, st = C.c_size_t(99), _lib.RegionStats(*([9] * 7))
        rc_ = L.flimo_map_region_list(h, C.byref(k), cap, C.byref(nr), label.ctypes.data, count.ctypes.data, first.ctypes.data, cen.ctypes.data,
                                      cov.ctypes.data, C.byref(st))
        assert nr.value == m
        if cap < m:
            assert rc_ == ERR_TOO_LARGE and st.as_dict() == dict.fromkeys(rc.STATS, 9)
            assert np.all(label == -7) and np.all(count == -7) and np.all(first == -7) and np.all(cen == -7.0) and np.all(cov == -7.0)
        else:
            assert rc_ == 0
            rc.same_listing(dict(label=label[:m], count=count[:m], first=first[:m], centroid=cen[:m], cov=cov[:m], nr=int(nr.value), stats=st.as_dict()),
                            li, "cap %d" % cap)
            assert np.all(label[m:] == -7) and np.all(cen[m:] == -7.0) and np.all(cov[m:] == -7.0)
    # no arrays: the count alone, whatever the cap
    nr = C.c_size_t(99)
    assert L.flimo_map_region_list(h, C.byref(k), 0, C.byref(nr), None, None, None, None, None, None) == 0 and nr.value == m
    # nothing asked for at all: nothing to do, but the arguments are still checked
    assert L.flimo_map_region_list(h, C.byref(k), 0, None, None, None, None, None, None, None) == 0
    bad = _lib.region_cfg(**dict(s, tol=-1.0))
    assert L.flimo_map_region_list(h, C.byref(bad), 0, None, None, None, None, None, None, None) == ERR_INVALID


def test_regions_of_exactly_63_64_65_and_1025_members_and_the_whole_scene_as_one(std):
    pts, which = rc.hand_regions()
    ctx = _one(pts)
    try:
        cfg = dict(tol=0.15, normal_k=9, min_cos=0.9, max_curv=0.01, border=1)
        nrm = _normals(ctx, **cfg)
        lab = rc.labels(pts, nrm, **rc.cfg_of(**cfg))
        want = rc.listing(pts, lab, nrm, cfg["max_curv"])
        assert sorted(want["count"].tolist()) == [63, 64, 65, 1025]
        for plan in (0, 1, 2, 3, 4):
            ctx.set_voxel_plan(plan)
            got = ctx.map_region_list(want=ALL5, **cfg)
            rc.same_listing(got, want, "plan %d" % plan)
        ctx.set_voxel_plan(0)
        for r in range(4):
            assert len(np.unique(which[lab == got["label"][r]])) == 1
    finally:
        ctx.close()
    ctx, s = std["ctx"], dict(tol=0.15, normal_k=16, min_cos=0.0, max_curv=INF, border=0)
    got = ctx.map_region_list(want=ALL5, **s)
    assert got["nr"] == 1 and got["count"].tolist() == [5060] and got["label"].tolist() == [0] and got["first"].tolist() == [0]
    rc.same_listing(got, rc.listing(std["pts"], np.zeros(5060, np.int64), std["nrm"][16], INF), "one region")


# ---- 4. no side effects ---------------------------------------------------------------------------------------------------------------
def test_the_calls_change_neither_map_nor_scan_nor_a_later_pass(built):
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
                for cfg in (dict(tol=0.3), dict(tol=1.0, min_size=2, max_size=50, border=0)):
                    assert h.map_regions(**cfg)["stats"]["n"] == len(mp)
                    assert h.map_region_list(**cfg)["stats"]["n"] == len(mp)
                h.set_region_chunk(777)
                assert h.map_regions(5000, 3000, tol=0.5)["stats"]["n"] == 3000
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


# ---- 5. removal -----------------------------------------------------------------------------------------------------------------------
def _twin_of(kept):
    twin = _ctx([rc.scene()[:100]])
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


@pytest.mark.parametrize("rng", [(0, None), (1000, 2000)], ids=["whole", "a-range-that-cuts-regions"])
def test_removal_keeps_the_rest_in_order_and_leaves_a_fresh_map(built, rng):
    """The large smooth regions go (the walls and the floor of a room), what is left is the creases and whatever stood there."""
    first, n = rng
    pts = rc.scene()
    cfg = dict(rc.SETTINGS[1], min_size=1000, max_size=0)
    ctx = _one(pts)
    try:
        want = _want(ctx, pts, first, n, **cfg)
        gone = np.zeros(len(pts), bool)
        gone[first:first + len(want["mask"])] = want["mask"]
        assert 0 < gone.sum() < len(pts) and want["stats"]["sel_regions"] == 3
        kept = pts[~gone]
        twin = _twin_of(kept)
        try:
            t_before = ctx._L.flimo_map_last_time(ctx._h)
            removed, stats = ctx.map_remove_regions(first, n, **cfg)
            assert removed == int(gone.sum()) == stats["sel_points"] and stats == want["stats"]
            assert ctx._L.flimo_map_last_time(ctx._h) == t_before
            _same_map(ctx, twin, kept, "after the removal")
            if n is None:                                                  # a second removal finds no region of 1 000 points
                layout = ctx.grid_selfcheck()
                removed, stats = ctx.map_remove_regions(**cfg)
                assert removed == 0 and stats["sel_points"] == 0 and stats["sel_regions"] == 0 and stats["n"] == len(kept)
                assert ctx.grid_selfcheck() == layout
                np.testing.assert_array_equal(ctx.map_points(), kept)
            later = cc.small(257) + F(20.0)                                # the map goes on: a later add lands in both alike
            ctx.map_add(later, stamp=0.9); twin.map_add(later, stamp=0.9)
            _same_map(ctx, twin, ctx.map_points().copy(), "an add after the removal")
        finally:
            twin.close()
    finally:
        ctx.close()


def test_removing_everything_empties_the_map_and_an_empty_map_answers(built):
    pts = rc.scene()
    ctx = _one(pts)
    try:
        open_cfg = dict(tol=0.15, normal_k=16, min_cos=0.0, max_curv=INF, border=0, min_size=0)
        removed, stats = ctx.map_remove_regions(**open_cfg)
        assert removed == len(pts) == stats["sel_points"] and ctx.map_size() == 0
        none = dict.fromkeys(rc.STATS, 0)
        out = ctx.map_regions(tol=0.5)
        assert len(out["label"]) == 0 and out["stats"] == none
        assert ctx.map_remove_regions(tol=0.5) == (0, none)
        li = ctx.map_region_list(want=ALL5, tol=0.5)
        assert li["nr"] == 0 and li["stats"] == none and li["cov"].shape == (0, 6)
        ctx.map_add(pts[:500], stamp=1.5)
        rc.same(ctx.map_regions(tol=0.3), _want(ctx, pts[:500], tol=0.3), "after the refill")
    finally:
        ctx.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_and_map_are_untouched(std):
    from fast_limo_amd import _lib
    ctx, pts = std["ctx"], std["pts"]
    L, h = ctx._L, ctx._h
    n = len(pts)
    layout = ctx.grid_selfcheck()
    K = lambda **kw: _lib.region_cfg(**dict(rc.SETTINGS[1], **kw))
    cases = [("null cfg", None, 0, n, ERR_INVALID), ("range beyond the map", K(), 0, n + 1, ERR_INVALID), ("first beyond the map", K(), n + 1, 0, ERR_INVALID),
             ("first + n wraps", K(), 2, 2 ** 64 - 1, ERR_INVALID), ("nan tol", K(tol=np.nan), 0, n, ERR_INVALID),
             ("negative tol", K(tol=-0.5), 0, n, ERR_INVALID), ("infinite tol", K(tol=INF), 0, n, ERR_INVALID),
             ("nan min_cos", K(min_cos=np.nan), 0, n, ERR_INVALID), ("min_cos below 0", K(min_cos=-0.01), 0, n, ERR_INVALID),
             ("min_cos above 1", K(min_cos=1.01), 0, n, ERR_INVALID), ("nan max_curv", K(max_curv=np.nan), 0, n, ERR_INVALID),
             ("negative max_curv", K(max_curv=-0.01), 0, n, ERR_INVALID), ("nan gate", K(normal_max_dist=np.nan), 0, n, ERR_INVALID),
             ("negative gate", K(normal_max_dist=-1.0), 0, n, ERR_INVALID), ("normal_min_pts -1", K(normal_min_pts=-1), 0, n, ERR_INVALID),
             ("min_size -1", K(min_size=-1), 0, n, ERR_INVALID), ("max_size -1", K(max_size=-1), 0, n, ERR_INVALID),
             ("max_size below min_size", K(min_size=5, max_size=4), 0, n, ERR_INVALID), ("nan tol, n 0", K(tol=np.nan), 0, 0, ERR_INVALID),
             ("normal_k 0", K(normal_k=0), 0, n, ERR_UNSUPPORTED), ("normal_k 65", K(normal_k=65), 0, n, ERR_UNSUPPORTED),
             ("normal_k 65, n 0", K(normal_k=65), 5, 0, ERR_UNSUPPORTED)]
    for what, k, first, cnt_n, code in cases:
        kp = None if k is None else C.byref(k)
        label, size, mask = np.full(n + 1, 7, np.int32), np.full(n + 1, 7, np.int32), np.full(n + 1, 7, np.uint8)
        cen, cov = np.full((n + 1, 3), 7.0), np.full((n + 1, 6), 7.0)
        st = _lib.RegionStats(*([9] * 7))
        removed, nr = C.c_size_t(5), C.c_size_t(5)
        assert L.flimo_map_regions(h, first, cnt_n, kp, label.ctypes.data, size.ctypes.data, mask.ctypes.data, C.byref(st)) == code, what
        assert L.flimo_map_remove_regions(h, first, cnt_n, kp, C.byref(removed), C.byref(st)) == code, what
        if "beyond" not in what and "wraps" not in what:
            assert L.flimo_map_region_list(h, kp, n + 1, C.byref(nr), label.ctypes.data, size.ctypes.data, size.ctypes.data, cen.ctypes.data,
                                           cov.ctypes.data, C.byref(st)) == code, what
        assert np.all(label == 7) and np.all(size == 7) and np.all(mask == 7) and removed.value == 5 and nr.value == 5, what
        assert np.all(cen == 7.0) and np.all(cov == 7.0) and st.as_dict() == dict.fromkeys(rc.STATS, 9), what
    assert ctx.map_size() == n and ctx.grid_selfcheck() == layout
    np.testing.assert_array_equal(ctx.map_points(), pts)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_regions(tol=-1.0)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_remove_regions(0, n + 1, tol=0.5)
    # equal bounds are a valid window; n = 0 fills the whole map's fields
    out = ctx.map_regions(n, 0, **rc.SETTINGS[1], min_size=300, max_size=1300)
    want = _fin(std, 1, n, 0, min_size=300, max_size=1300)
    assert out["stats"] == want["stats"] and out["stats"]["n"] == 0 and out["stats"]["sel_points"] == 0 and out["stats"]["regions"] > 0


def test_the_edges_of_the_accepted_values(built):
    pts = rc.scene()[:1200]
    ctx = _one(pts)
    try:
        for kw in (dict(min_cos=0.0), dict(min_cos=1.0), dict(max_curv=0.0), dict(max_curv=INF), dict(normal_max_dist=0.0), dict(normal_k=1),
                   dict(normal_k=64), dict(normal_min_pts=0), dict(normal_min_pts=17), dict(tol=1e-30)):
            cfg = dict(dict(rc.SETTINGS[1], tol=0.3), **kw)
            got = ctx.map_regions(**cfg)
            print(kw, got["stats"])
            rc.same(got, _want(ctx, pts, **cfg), str(kw))
    finally:
        ctx.close()


# ---- 7. the Localizer's forms ---------------------------------------------------------------------------------------------------------
def test_the_localizer_forms_equal_the_contexts(built):
    from fast_limo_amd import api
    cfg = dict(rc.SETTINGS[1], min_size=1000, max_size=0)
    none = dict.fromkeys(rc.STATS, 0)
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        out = loc.map_regions(**cfg)                                 # no map yet: an empty one's answer
        assert len(out["label"]) == 0 and out["stats"] == none
        assert loc.map_remove_regions(**cfg) == (0, none)
        li = loc.map_region_list(**cfg)
        assert li["nr"] == 0 and li["stats"] == none
        with pytest.raises(api.FlimoError):
            loc.map_regions(0, 5, **cfg)
        with pytest.raises(api.FlimoError):
            loc.map_regions(tol=-1.0)
        with pytest.raises(api.FlimoError):
            loc.map_region_list(normal_k=0)
        loc.map_add(rc.scene())
        n = loc.map_size()
        pts = loc.hip.map_points().copy()
        a, b = loc.map_regions(**cfg), loc.hip.map_regions(**cfg)
        assert _sig(a) == _sig(b) and a["stats"]["n"] == n
        rc.same(a, _want(loc.hip, pts, **cfg), "localizer")
        assert _lsig(loc.map_region_list(want=ALL5, **cfg)) == _lsig(loc.hip.map_region_list(want=ALL5, **cfg))
        a, b = loc.map_regions(n - 300, 200, want=("mask",), **cfg), loc.hip.map_regions(n - 300, 200, want=("mask",), **cfg)
        assert sorted(a) == ["mask", "stats"] and a["stats"] == b["stats"]
        np.testing.assert_array_equal(a["mask"], b["mask"])
        whole = loc.hip.map_regions(**cfg)
        removed, stats = loc.map_remove_regions(**cfg)
        assert removed == whole["stats"]["sel_points"] == stats["sel_points"] > 0 and stats == whole["stats"]
        assert loc.map_size() == n - removed
        np.testing.assert_array_equal(loc.hip.map_points(), pts[~whole["mask"]])
        assert loc.hip.grid_selfcheck()[0] == 0
        # what the large smooth regions leave behind is what the clusters then see
        left = loc.map_clusters(tol=0.15, min_size=10)
        print("left", loc.map_size(), left["stats"])
        assert left["stats"]["clusters"] > 1
    finally:
        loc.close()
