"""RANSAC planes of the stored points on the GPU (flimo_map_planes, flimo_map_plane_mask, flimo_map_remove_plane) against the
definition restated in numpy (tests/planes_common.py): status, inliers, mask and count with no tolerance, plane and sum_sq bit for
bit.  Maps of at most 25 000 points, at most 1 024 hypotheses a call."""
import ctypes as C

import numpy as np
import pytest

import planes_common as pc
from common import CAPS
from radius_common import bits

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5
F = np.float32
D = np.float64
INF = float("inf")
G, W = pc.SHIPPED_G, pc.SHIPPED_W


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_planes", "flimo_map_plane_mask", "flimo_map_remove_plane", "flimo_set_plane_chunk", "flimo_plane_solve_host"):
        getattr(L, name)
    for name in ("flimo_loc_map_planes", "flimo_loc_map_plane_mask", "flimo_loc_map_remove_plane"):
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


def _mixed_triplets(pts, nh, seed):
    """Random triplets (a repeated index now and then) with the hand-made ones in front."""
    hand = np.array([t for _, t, _ in pc.hand_triplets(pts)], np.int32)
    return np.concatenate([hand, pc.random_triplets(len(pts), nh - len(hand), seed)]).astype(np.int32)


@pytest.fixture(scope="module")
def std(built):
    """The standard scene in three batches, its stored points, 400 mixed hypotheses and their restatement under the recovery's
    cfg, computed once."""
    pts = pc.scene()
    ctx = _ctx([pts[:2500], pts[2500:4100], pts[4100:]], downsample=False)
    stored = ctx.map_points().copy()
    assert 4000 <= len(stored) <= 8000
    tri = _mixed_triplets(stored, 400, 1)
    want = pc.restate(stored, tri, **pc.REC_CFG)
    yield dict(ctx=ctx, pts=stored, tri=tri, want=want)
    ctx.close()


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
def test_the_standard_scene_equals_the_restatement(std):
    ctx, pts, tri, want = std["ctx"], std["pts"], std["tri"], std["want"]
    got = ctx.map_planes(tri, **pc.REC_CFG)
    for (name, _, st), g in zip(pc.hand_triplets(pts), got["status"]):
        assert g == st, name
    assert {pc.OK, pc.DEGENERATE, pc.REJECTED} == set(got["status"].tolist())
    print("OK", int((got["status"] == pc.OK).sum()), "of", len(tri), "most inliers", int(got["inliers"].max()))
    pc.same(got, want, "recovery cfg")
    assert np.all(got["inliers"][got["status"] == pc.OK] >= 3)                    # the sample's own points count
    assert not np.signbit(got["sum_sq"]).any() and np.all(got["sum_sq"][got["status"] != pc.OK] == 0)
    # no constraint at all, a wide gate: every triplet of distinct points survives
    sub = tri[:120]
    loose = dict(dist=0.2)
    pc.same(ctx.map_planes(sub, **loose), pc.restate(pts, sub, **loose), "defaults")
    # the plane is optional
    bare = ctx.map_planes(tri, want=(), **pc.REC_CFG)
    assert sorted(bare) == ["inliers", "status", "sum_sq"]
    pc.same(bare, want, "no plane")


@pytest.mark.parametrize("n", [3, 4, 255, 256, 257, 8191, 8192, 8193, 2 * 8192 + 1])
def test_sizes_around_the_thread_stride_and_the_slab(built, n):
    pts = pc.cloud(n, seed=1)
    ctx = _one(pts)
    try:
        tri = pc.random_triplets(n, 24, n)
        tri[0] = (0, 1, 2)
        tri[1] = (n - 1, 0, n // 2)                                                # the last point anchors one
        cfg = dict(dist=0.05, min_sin=0.05)
        got, want = ctx.map_planes(tri, **cfg), pc.restate(pts, tri, **cfg)
        pc.same(got, want, "n %d" % n)
        assert (got["status"] == pc.OK).sum() >= (1 if n <= 4 else 8)
        wide = dict(dist=INF)                                                      # every point of every slab counts
        got = ctx.map_planes(tri, **wide)
        pc.same(got, pc.restate(pts, tri, **wide), "n %d, no gate" % n)
        assert np.all(got["inliers"][got["status"] == pc.OK] == n)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def mid(built):
    pts = pc.cloud(9001, seed=2)
    ctx = _one(pts)
    yield dict(ctx=ctx, pts=pts)
    ctx.close()


@pytest.mark.parametrize("nh", sorted({1, G - 1, G, G + 1, 2 * G + 1, G * W - 1, G * W, G * W + 1, 2 * G * W + 1, 7, 8, 9}))
def test_hypotheses_around_the_group_and_the_walk(mid, nh):
    ctx, pts = mid["ctx"], mid["pts"]
    tri = pc.random_triplets(len(pts), nh, 50 + nh)
    tri[:, 1] = (tri[:, 0] + 1 + tri[:, 1] % 100) % len(pts)                       # distinct indices: every hypothesis survives
    tri[:, 2] = (tri[:, 0] + 200 + tri[:, 2] % 100) % len(pts)
    got = ctx.map_planes(tri, dist=0.04)
    assert np.all(got["status"] == pc.OK)
    pc.same(got, pc.restate(pts, tri, dist=0.04), "nh %d" % nh)


def test_nothing_to_count_and_exactly_one_survivor(mid):
    ctx, pts = mid["ctx"], mid["pts"]
    tri = pc.random_triplets(len(pts), 40, 3)
    none = ctx.map_planes(tri, dist=0.05, min_edge=100.0)                          # no edge is that long: all DEGENERATE
    assert np.all(none["status"] == pc.DEGENERATE) and not none["inliers"].any() and np.all(pc.bits(none["sum_sq"]) == 0)
    assert np.all(np.isnan(none["plane"]))
    pc.same(none, pc.restate(pts, tri, dist=0.05, min_edge=100.0), "none")
    for where in (0, 17, 39):
        one = np.tile(np.array([[5, 5, 9]], np.int32), (40, 1))                    # a repeated index everywhere ...
        one[where] = (10, 500, 4000)                                               # ... but here
        got = ctx.map_planes(one, dist=0.05)
        assert (got["status"] == pc.OK).sum() == 1 and got["status"][where] == pc.OK and got["inliers"][where] >= 3
        pc.same(got, pc.restate(pts, one, dist=0.05), "one survivor at %d" % where)


# ---- 2. no bit moves ------------------------------------------------------------------------------------------------------------------
def test_no_bit_moves_with_the_chunk_the_order_or_the_company(std):
    ctx, pts, tri, want = std["ctx"], std["pts"], std["tri"][:61], std["want"]
    base = ctx.map_planes(tri, **pc.REC_CFG)
    pc.same(base, {k: v[:61] for k, v in want.items()}, "base")
    try:
        for chunk in (1, 3, 7):
            ctx.set_plane_chunk(chunk)
            pc.same_bits(ctx.map_planes(tri, **pc.REC_CFG), base, "chunk %d" % chunk)
    finally:
        ctx.set_plane_chunk(0)
    pc.same_bits(ctx.map_planes(tri, **pc.REC_CFG), base, "the default chunk again")
    rev = ctx.map_planes(tri[::-1], **pc.REC_CFG)
    pc.same_bits({k: v[::-1] for k, v in rev.items()}, base, "reversed")
    ok = np.flatnonzero(base["status"] == pc.OK)
    j = int(ok[len(ok) // 2])
    alone = ctx.map_planes(tri[j:j + 1], **pc.REC_CFG)
    pc.same_bits(alone, {k: v[j:j + 1] for k, v in base.items()}, "alone")
    crowd = np.concatenate([pc.random_triplets(len(pts), 613, 9), tri[j:j + 1], pc.random_triplets(len(pts), 387, 10)])
    among = ctx.map_planes(crowd, **pc.REC_CFG)
    pc.same_bits({k: v[613:614] for k, v in among.items()}, alone, "among 1 000 others")
    full = ctx.map_planes(std["tri"], **pc.REC_CFG)                                # nh moves nothing either
    pc.same_bits({k: v[:61] for k, v in full.items()}, base, "the first 61 of 400")


def test_no_bit_moves_with_the_cell_size_or_the_batches(std):
    pts, tri = std["pts"], std["tri"][:80]
    base = std["ctx"].map_planes(tri, **pc.REC_CFG)
    cuts = [0, 700, 1500, 3100, 4800, len(pts)]
    variants = [("cell %g" % cell, lambda cell=cell: _one(pts, cell)) for cell in (0.25, 0.5, 2.0)]
    variants.append(("five batches", lambda: _ctx([pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])], downsample=False)))
    for what, make in variants:
        ctx = make()
        try:
            stored = ctx.map_points()
            np.testing.assert_array_equal(stored, pts, err_msg=what)               # the same stored points in the same order
            pc.same_bits(ctx.map_planes(tri, **pc.REC_CFG), base, what)
        finally:
            ctx.close()


# ---- 3. the gate ----------------------------------------------------------------------------------------------------------------------
def test_the_gate_is_strict_on_a_lattice_where_t_is_exact(built):
    pts, zs = pc.lattice_layers()
    ctx = _one(pts)
    try:
        tri = np.array([[0, 1, 2], [0, 2, 1], [2, 0, 1]], np.int32)
        dist = 64 * pc.STEP
        got = ctx.map_planes(tri, dist=dist)
        np.testing.assert_array_equal(got["plane"], [[0.0, 0.0, 1.0, 0.0]] * 3)
        inside = np.abs(zs) < 64                                                   # exactly dist away stays out, one step nearer is in
        assert got["inliers"].tolist() == [int(inside.sum())] * 3 == [5 * 576] * 3
        t = (zs * pc.STEP).astype(F)
        np.testing.assert_array_equal(pc.signed_t(pts, F([0, 0, 1]), pts[0]), t)   # t IS z: exact
        pc.same(got, pc.restate(pts, tri, dist=dist), "lattice")
        assert got["sum_sq"][0] == 2 * 576 * (63 * pc.STEP) ** 2 + 2 * 576 * pc.STEP ** 2      # exact in float64 whatever the shape
        mask, count = ctx.map_plane_mask(normal=(0, 0, 1), anchor=pts[0], dist=dist)
        np.testing.assert_array_equal(mask, inside)
        assert count == inside.sum()
        for d, inl in ((float(pc.up(dist)), np.abs(zs) <= 64), (0.0, np.zeros(len(zs), bool)), (INF, np.ones(len(zs), bool))):
            got = ctx.map_planes(tri, dist=d)
            assert got["inliers"].tolist() == [int(inl.sum())] * 3, d
            pc.same(got, pc.restate(pts, tri, dist=d), "dist %r" % d)
            assert ctx.map_plane_mask(normal=(0, 0, 1), anchor=pts[0], dist=d, want_mask=False) == (None, int(inl.sum()))
    finally:
        ctx.close()


def test_a_map_ten_kilometres_away_counts_the_same(built):
    pts, _ = pc.lattice_layers()
    shift = F([10240.0, -10240.0, 10240.0])                                        # a multiple of the lattice step, and of the ulp there
    far = (pts + shift).astype(F)
    assert np.array_equal(far.astype(D) - shift.astype(D), pts.astype(D))          # nothing was rounded
    tri = np.concatenate([[[0, 1, 2]], pc.random_triplets(len(pts), 63, 4)]).astype(np.int32)
    cfg = dict(dist=0.05, min_sin=0.05)
    near_ctx, far_ctx = _one(pts), _one(far)
    try:
        a, b = near_ctx.map_planes(tri, **cfg), far_ctx.map_planes(tri, **cfg)
        pc.same(b, pc.restate(far, tri, **cfg), "far")
        assert (a["status"] == pc.OK).sum() > 40
        for key in ("status", "inliers", "sum_sq"):                                # the differences are exact: the same t, bit for bit
            assert a[key].tobytes() == b[key].tobytes(), key
        ok = a["status"] == pc.OK
        assert a["plane"][ok, :3].tobytes() == b["plane"][ok, :3].tobytes()
    finally:
        near_ctx.close(); far_ctx.close()


def test_duplicates_of_a_sample_point_all_count(built):
    base = pc.cloud(500, seed=3)
    pts = np.concatenate([base[:300], np.tile(base[7:8], (50, 1)), base[300:]]).astype(F)
    ctx = _one(pts)
    try:
        tri = np.array([[7, 100, 400], [300, 100, 400], [349, 7, 100], [7, 300, 100], [7, 310, 349]], np.int32)
        got = ctx.map_planes(tri, dist=0.02)
        pc.same(got, pc.restate(pts, tri, dist=0.02), "duplicates")
        assert got["status"].tolist() == [pc.OK, pc.OK, pc.DEGENERATE, pc.DEGENERATE, pc.DEGENERATE]      # equal points, distinct indices: q == 0
        assert np.all(got["inliers"][:2] >= 53) and got["plane"][0].tobytes() == got["plane"][1].tobytes()
    finally:
        ctx.close()


# ---- 4. the mask ----------------------------------------------------------------------------------------------------------------------
def test_the_mask_counts_the_inliers_of_every_hypothesis(std):
    ctx, pts, tri, want = std["ctx"], std["pts"], std["tri"][:48], std["want"]
    dist = pc.REC_CFG["dist"]
    ok = np.flatnonzero(want["status"][:48] == pc.OK)
    assert len(ok) >= 5
    for j in ok:
        nf, anchor = want["plane"][j, :3].astype(F), pts[tri[j, 0]]
        mask, count = ctx.map_plane_mask(normal=nf, anchor=anchor, dist=dist, side=0)
        assert count == want["inliers"][j] == mask.sum(), j
        np.testing.assert_array_equal(mask, pc.mask_restate(pts, nf, anchor, dist), err_msg=str(j))


def test_the_three_sides_and_ranges(std):
    from fast_limo_amd import _lib
    ctx, pts = std["ctx"], std["pts"]
    n = len(pts)
    nf, anchor = F([0.05, -0.02, 0.998]), F([1.0, 1.0, 0.5])
    whole = {}
    for side in (-1, 0, 1):
        mask, count = ctx.map_plane_mask(_lib.plane_sel(nf, anchor, 0.3, side))
        want = pc.mask_restate(pts, nf, anchor, 0.3, side)
        np.testing.assert_array_equal(mask, want, err_msg="side %d" % side)
        assert count == want.sum() and 0 < count < n
        whole[side] = mask
    np.testing.assert_array_equal(whole[0], whole[-1] & whole[1])
    assert np.all(whole[-1] | whole[1])
    for first, cnt in ((0, 1), (1, 255), (63, 65), (1000, 4097), (n - 1, 1), (n, 0), (17, 0)):
        mask, count = ctx.map_plane_mask(first=first, n=cnt, normal=nf, anchor=anchor, dist=0.3, side=-1)
        np.testing.assert_array_equal(mask, whole[-1][first:first + cnt], err_msg=str((first, cnt)))
        assert count == mask.sum()
    assert ctx.map_plane_mask(first=5, normal=nf, anchor=anchor, dist=0.3, side=1, want_mask=False) == (None, int(whole[1][5:].sum()))


# ---- 5. removal -----------------------------------------------------------------------------------------------------------------------
def _twin_of(kept):
    twin = _ctx([pc.scene()[:100]])
    twin.map_clear()
    if len(kept):
        twin.map_add(kept, stamp=0.5)
    return twin


def _same_map(ctx, twin, kept, what):
    assert ctx.map_size() == twin.map_size() == len(kept), what
    np.testing.assert_array_equal(ctx.map_points(), kept, err_msg=what)
    np.testing.assert_array_equal(twin.map_points(), kept, err_msg=what)
    assert ctx.grid_selfcheck()[0] == 0 and twin.grid_selfcheck()[0] == 0, what
    q = np.concatenate([kept[:: max(len(kept) // 100, 1)][:100], kept[:: max(len(kept) // 100, 1)][:100] + F(0.03)])
    (i, s, c), (ti, ts, tc) = ctx.knn_k(q, 12, 3.0), twin.knn_k(q, 12, 3.0)
    np.testing.assert_array_equal(i, ti, err_msg=what)
    np.testing.assert_array_equal(bits(s), bits(ts), err_msg=what)
    np.testing.assert_array_equal(c, tc, err_msg=what)
    a, b = ctx.map_clusters(tol=pc.REC_TOL), twin.map_clusters(tol=pc.REC_TOL)
    np.testing.assert_array_equal(a["label"], b["label"], err_msg=what)
    assert a["stats"] == b["stats"], what


@pytest.mark.parametrize("case", [(0, None, 0), (1000, 3000, -1)], ids=["whole-both-sides", "a-range-beneath"])
def test_removal_keeps_the_rest_in_order_and_leaves_a_fresh_map(built, case):
    first, n, side = case
    pts = pc.scene()
    nf, anchor = F([0.0, 0.0, 1.0]), pts[pc.nearest(pts, (2.0, 2.0, 0.0))]
    gone = np.zeros(len(pts), bool)
    m = pc.mask_restate(pts, nf, anchor, 0.05, side, first, n)
    gone[first:first + len(m)] = m
    assert 300 < gone.sum() < 1700
    kept = pts[~gone]
    ctx, twin = _one(pts), _twin_of(kept)
    try:
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        assert ctx.map_remove_plane(first=first, n=n, normal=nf, anchor=anchor, dist=0.05, side=side) == int(gone.sum())
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before
        _same_map(ctx, twin, kept, "after the removal")
        later = pc.cloud(257, seed=9) + F(20.0)                                    # the map goes on: a later add lands in both alike
        ctx.map_add(later, stamp=0.9); twin.map_add(later, stamp=0.9)
        _same_map(ctx, twin, ctx.map_points().copy(), "an add after the removal")
    finally:
        ctx.close(); twin.close()


def test_removing_nothing_changes_nothing_and_removing_everything_empties_the_map(built):
    pts = pc.scene()
    N = len(pts)
    ctx = _one(pts)
    try:
        q = pts[::31]
        before = ctx.knn(q, 5)
        layout = ctx.grid_selfcheck()
        far = dict(normal=(0, 0, 1), anchor=(0, 0, 50.0), dist=0.05)                # a plane nothing lies near
        assert ctx.map_remove_plane(**far) == 0 and ctx.map_remove_plane(dist=0.0, normal=(0, 0, 1), anchor=pts[0]) == 0
        assert ctx.map_size() == N and ctx.grid_selfcheck() == layout              # no build, no merge
        np.testing.assert_array_equal(ctx.map_points(), pts)
        for a, b in zip(before, ctx.knn(q, 5)):
            np.testing.assert_array_equal(a, b)
        t_before = ctx._L.flimo_map_last_time(ctx._h)
        assert ctx.map_remove_plane(normal=(0, 0, 1), anchor=pts[0], dist=INF) == N
        assert ctx.map_size() == 0 and len(ctx.map_points()) == 0
        assert ctx._L.flimo_map_last_time(ctx._h) == t_before                      # as a crop that removes everything
        i, s, c = ctx.knn_k(q[:10], 5)
        assert np.all(c == 0) and np.all(i == -1)
        # the empty map: n = 0 and nh = 0 are fine, a hypothesis is not
        assert ctx.map_plane_mask(normal=(0, 0, 1), anchor=(0, 0, 0))[1] == 0 and ctx.map_remove_plane(normal=(0, 0, 1), anchor=(0, 0, 0)) == 0
        assert len(ctx.map_planes(np.zeros((0, 3), np.int32))["status"]) == 0
        with pytest.raises(Exception, match="invalid"):
            ctx.map_planes([[0, 1, 2]])
        ctx.map_add(pts[:500], stamp=1.5)                                          # and it takes points again
        assert ctx.map_size() == 500 and ctx.grid_selfcheck()[0] == 0
        tri = pc.random_triplets(500, 20, 6)
        pc.same(ctx.map_planes(tri), pc.restate(pts[:500], tri), "after the refill")
    finally:
        ctx.close()


# ---- 6. no side effects ---------------------------------------------------------------------------------------------------------------
def test_the_calls_change_neither_map_nor_scan_nor_a_later_pass(built):
    from fast_limo_amd import _lib, synth
    import outliers_common as oc
    mp = oc.scene()
    scan = np.ascontiguousarray(synth.box_world_scan_random(4096, 12.0, 2)[:, :3])
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    q = mp[::9]

    def run(planes):
        h = _one(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if planes:
                tri = pc.random_triplets(len(mp), 200, 2)
                assert (h.map_planes(tri, dist=0.1)["status"] == pc.OK).sum() > 100
                h.set_plane_chunk(33)
                assert h.map_planes(tri, **pc.REC_CFG)["inliers"].max() > 3
                assert h.map_plane_mask(normal=(0, 0, 1), anchor=mp[0], dist=0.5)[1] > 0
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


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_and_map_are_untouched(std):
    from fast_limo_amd import _lib
    ctx, pts = std["ctx"], std["pts"]
    L, h = ctx._L, ctx._h
    n = len(pts)
    layout = ctx.grid_selfcheck()
    good = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    K = lambda **kw: _lib.plane_cfg(**pc.cfg_of(**kw))

    def planes(tri, nh, k, null=()):
        status, inliers, ssq, plane = np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7.0), np.full((4, 4), 7.0)
        p = dict(tri=None if tri is None else tri.ctypes.data, cfg=None if k is None else C.byref(k), status=status.ctypes.data,
                 inliers=inliers.ctypes.data, sum_sq=ssq.ctypes.data)
        for name in null:
            p[name] = None
        rc = L.flimo_map_planes(h, p["tri"], nh, p["cfg"], p["status"], p["inliers"], p["sum_sq"], plane.ctypes.data)
        assert np.all(status == 7) and np.all(inliers == 7) and np.all(ssq == 7) and np.all(plane == 7)
        return rc

    for bad in pc.BAD_CFGS:
        assert planes(good, 2, K(**bad)) == ERR_INVALID, bad
    for name in ("cfg", "status", "inliers", "sum_sq", "tri"):
        assert planes(good, 2, K(), null=(name,)) == ERR_INVALID, name
    for idx in (-1, n, 2 ** 31 - 1, -2 ** 31):
        for pos in range(3):
            tri = good.copy()
            tri[1, pos] = idx
            assert planes(tri, 2, K()) == ERR_INVALID, (idx, pos)
    assert planes(None, 0, K()) == 0                                               # nh == 0: nothing to read
    assert planes(good, 2 ** 31, K()) == ERR_TOO_LARGE                             # (before any index is read)

    S = lambda **kw: _lib.plane_sel(**dict(dict(normal=(0, 0, 1), anchor=(0, 0, 0), dist=0.05, side=0), **kw))
    cases = [("null sel", None, 0, n), ("nan normal", S(normal=(np.nan, 0, 1)), 0, n), ("infinite normal", S(normal=(0, INF, 1)), 0, n),
             ("nan anchor", S(anchor=(0, 0, np.nan)), 0, n), ("infinite anchor", S(anchor=(-INF, 0, 0)), 0, n), ("nan dist", S(dist=np.nan), 0, n),
             ("negative dist", S(dist=-0.01), 0, n), ("side 2", S(side=2), 0, n), ("side -2", S(side=-2), 0, n),
             ("range beyond the map", S(), 0, n + 1), ("first beyond the map", S(), n + 1, 0), ("first + n wraps", S(), 2, 2 ** 64 - 1),
             ("nan dist, n 0", S(dist=np.nan), 0, 0)]
    for what, s, first, cnt_n in cases:
        sp = None if s is None else C.byref(s)
        mask, count, removed = np.full(n + 1, 7, np.uint8), C.c_size_t(5), C.c_size_t(5)
        assert L.flimo_map_plane_mask(h, first, cnt_n, sp, mask.ctypes.data, C.byref(count)) == ERR_INVALID, what
        assert L.flimo_map_remove_plane(h, first, cnt_n, sp, C.byref(removed)) == ERR_INVALID, what
        assert np.all(mask == 7) and count.value == 5 and removed.value == 5, what
    assert ctx.map_size() == n and ctx.grid_selfcheck() == layout
    np.testing.assert_array_equal(ctx.map_points(), pts)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_planes(good, dist=-1.0)
    with pytest.raises(_lib.FlimoError, match="invalid"):
        ctx.map_remove_plane(first=0, n=n + 1, normal=(0, 0, 1), anchor=(0, 0, 0))
    # both outputs of the mask are optional; equal bounds are a valid window
    assert L.flimo_map_plane_mask(h, 0, n, C.byref(S()), None, None) == 0
    assert ctx.map_plane_mask(first=n, n=0, normal=(0, 0, 1), anchor=(0, 0, 0))[1] == 0
    pc.same(ctx.map_planes(std["tri"], **pc.REC_CFG), std["want"], "after the refusals")


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_ground_goes_and_the_clusters_fall_apart(built, seed):
    from fast_limo_amd import api
    pts = pc.scene()
    ctx = _one(pts)
    try:
        if seed == 0:
            assert ctx.map_clusters(tol=pc.REC_TOL, want=())["stats"]["largest"] == 5060      # floor, wall and cylinder are one component
        best = api.plane_consensus(ctx, pc.REC_NH, seed=seed, top=4, **pc.REC_CFG)
        tri = api.corr_triplets(len(pts), pc.REC_NH, seed)
        want = pc.restate(pts, tri, **pc.REC_CFG)
        order = pc.rank(want)
        np.testing.assert_array_equal(best["index"], order[:4])
        assert best["survivors"] == len(order) and np.array_equal(best["tri"], tri[order[:4]])
        pc.same(dict(status=np.zeros(4, np.int32), inliers=best["inliers"], sum_sq=best["sum_sq"], plane=best["plane"]),
                {k: v[order[:4]] for k, v in want.items()}, "consensus")
        print("seed", seed, "survivors", best["survivors"], "inliers", best["inliers"], "plane", best["plane"][0])
        assert best["inliers"][0] >= 1500 and abs(best["plane"][0, 2]) >= 0.9999
        sel = best["sel"][0]
        assert ctx.map_plane_mask(sel, want_mask=False)[1] == best["inliers"][0]   # the cross property through the ready-made sel
        sel.dist = pc.REC_REMOVE_DIST
        removed = ctx.map_remove_plane(sel)
        print("removed", removed)
        assert 1595 <= removed <= 1605 and ctx.map_size() == len(pts) - removed
        size = np.sort(np.unique(ctx.map_clusters(tol=pc.REC_TOL, want=("label",))["label"], return_counts=True)[1])[::-1]
        assert size[0] == 1860 and size[1] == 1600, size[:4]
    finally:
        ctx.close()


# ---- 9. the Localizer's forms ---------------------------------------------------------------------------------------------------------
def test_the_localizer_forms_equal_the_contexts(built):
    from fast_limo_amd import api
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        assert len(loc.map_planes(np.zeros((0, 3), np.int32))["status"]) == 0      # no map yet: an empty one's answers
        assert loc.map_plane_mask(normal=(0, 0, 1), anchor=(0, 0, 0))[1] == 0 and loc.map_remove_plane(normal=(0, 0, 1), anchor=(0, 0, 0)) == 0
        with pytest.raises(api.FlimoError):
            loc.map_planes([[0, 1, 2]])
        with pytest.raises(api.FlimoError):
            loc.map_plane_mask(first=0, n=5, normal=(0, 0, 1), anchor=(0, 0, 0))
        loc.map_add(pc.scene())
        n = loc.map_size()
        pts = loc.hip.map_points().copy()
        tri = pc.random_triplets(n, 64, 11)
        a, b = loc.map_planes(tri, **pc.REC_CFG), loc.hip.map_planes(tri, **pc.REC_CFG)
        pc.same_bits(a, b, "localizer")
        pc.same(a, pc.restate(pts, tri, **pc.REC_CFG), "localizer")
        best = api.plane_consensus(loc, 512, seed=1, top=1, **pc.REC_CFG)
        sel = best["sel"][0]
        (ma, ca), (mb, cb) = loc.map_plane_mask(sel), loc.hip.map_plane_mask(sel)
        assert ca == cb == best["inliers"][0] and np.array_equal(ma, mb)
        assert loc.map_remove_plane(sel) == ca and loc.map_size() == n - ca
        np.testing.assert_array_equal(loc.hip.map_points(), pts[~ma])
        assert loc.hip.grid_selfcheck()[0] == 0
    finally:
        loc.close()
