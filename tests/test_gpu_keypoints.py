"""GPU suite: ISS keypoints of the stored points -- flimo_map_keypoints forms the saliency of the whole map and suppresses the
non-maxima of a range, all on the device.  The yardstick is the definition restated in numpy (tests/keypoints_common.py), fed with
the eigenvalues and the neighbour lists the same context returns (normals_range, knn_k): saliency bits, cnt, mask and count are
compared with no tolerance.  Chunking, cell size, range form, repetition, a second context and the outputs asked for move no bit.
The last test relocalises a scan in a map through the keypoints (api.relocalize(keypoints=..))."""
import ctypes as C
import time

import numpy as np
import pytest

import corr_common as cc
import desc_common as dc
import fpfh_common as fc
import keypoints_common as kc
import scan_linearize_common as sl
from common import CAPS

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -2, -6
INF = float("inf")
F = np.float32
KS, NMS_KS = (3, 16, 17, 64), (2, 16, 17, 64)                     # the lane plan divides at 16


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_keypoints", "flimo_set_keypoints_chunk"):
        getattr(L, name)
    getattr(H, "flimo_loc_map_keypoints")


def _ctx(pts, cell=0.0, downsample=True):
    """The whole cloud as the first add: the first build neither drops points nor merges duplicates."""
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, downsample, cell)
    ctx.map_add(pts, stamp=0.5)
    assert ctx.map_size() == len(pts)
    np.testing.assert_array_equal(ctx.map_points(), pts)
    return ctx


@pytest.fixture(scope="module")
def scene_ctx(built):
    ctx = _ctx(fc.scene())
    yield ctx
    ctx.close()


_CACHE = {}


def _eig(ctx, k, max_dist, min_pts, memo=None):
    """(eig [N, 6], cnt [N]) of every stored point from the context's own normals_range (memo: a dict that keeps them)."""
    key = ("eig", k, max_dist, min_pts)
    if memo is None or key not in memo:
        out = ctx.normals_range(0, ctx.map_size(), k, max_dist, min_pts, None, want=("eig",))
        if memo is None:
            return out["eig"], out["cnt"]
        memo[key] = (out["eig"], out["cnt"])
    return memo[key]


def _lists(ctx, k, max_dist, memo=None):
    key = ("lists", k, max_dist)
    if memo is None or key not in memo:
        idx, _, cnt = ctx.knn_k(ctx.map_points(), k, max_dist)
        if memo is None:
            return idx, cnt
        memo[key] = (idx, cnt)
    return memo[key]


def _restated(ctx, cfg, first=0, n=None, memo=None):
    """The restatement fed with this context's own eigenvalues and lists."""
    c = kc.full(cfg)
    eig, cnt = _eig(ctx, c["k"], c["max_dist"], c["min_pts"], memo)
    idx, ncnt = _lists(ctx, c["nms_k"], c["nms_max_dist"], memo)
    return kc.restate(eig, cnt, idx, ncnt, cfg, first, n)


def _same_as_restatement(ctx, cfg, what, memo=None):
    out = ctx.map_keypoints(**cfg)
    r = _restated(ctx, cfg, memo=memo)
    print(what, "points", len(r["mask"]), "salient", int((~np.isnan(r["saliency"])).sum()), "keypoints", r["count"], "device", out["count"])
    assert out["mask"].dtype == bool and out["saliency"].dtype == np.float64 and out["cnt"].dtype == np.int32 and out["index"].dtype == np.int64
    kc.same(out, r, what)
    assert np.array_equal(out["index"], np.flatnonzero(r["mask"])), what
    return out, r


def _same_bits(a, b, what):
    for key in ("mask", "saliency", "cnt"):
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (what, key)
    assert a["count"] == b["count"] and np.array_equal(a["index"], b["index"]), what


def _cut(whole, first, n):
    m = whole["mask"][first:first + n]
    return dict(mask=m, saliency=whole["saliency"][first:first + n], cnt=whole["cnt"][first:first + n], count=int(m.sum()), index=np.flatnonzero(m).astype(np.int64))


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_outputs_equal_the_restatement(scene_ctx, k):
    """Every k with every nms_k, without gates and with them (a salient radius of 0.25 m holds about 19 of the scene's points: min_pts
    12 lies below the typical count, 25 above it), at PCL's thresholds and at tighter ones."""
    memo = _CACHE.setdefault("scene", {})
    seen = {None: [], 12: [], 25: []}
    for nms_k in NMS_KS:
        out, r = _same_as_restatement(scene_ctx, dict(k=k, nms_k=nms_k, min_pts=0), "k %d nms_k %d" % (k, nms_k), memo)
        seen[None].append((int((~np.isnan(out["saliency"])).sum()), out["count"]))
        assert np.all(out["cnt"] == k)
        for min_pts in (12, 25):
            cfg = dict(kc.SCENE_GATED, k=k, nms_k=nms_k, min_pts=min_pts)
            out, r = _same_as_restatement(scene_ctx, cfg, "k %d nms_k %d gates min_pts %d" % (k, nms_k, min_pts), memo)
            seen[min_pts].append((int((~np.isnan(out["saliency"])).sum()), out["count"]))
            assert np.all(out["cnt"] <= k) and out["cnt"].min() >= 3
    assert kc.scene_counts_hold(k, seen[None], seen[12], seen[25], len(fc.scene())), seen


# ---- 2. nothing moves the bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,nms_k", [(16, 17), (33, 9)])
def test_bits_do_not_depend_on_the_chunk_the_cell_size_the_range_or_the_call(scene_ctx, k, nms_k):
    cfg = dict(k=k, nms_k=nms_k, max_dist=0.5, nms_max_dist=0.3, gamma21=0.9, gamma32=0.9)
    whole = scene_ctx.map_keypoints(**cfg)
    assert 0 < whole["count"] < (~np.isnan(whole["saliency"])).sum() < len(fc.scene())
    _same_bits(scene_ctx.map_keypoints(**cfg), whole, "twice")
    scene_ctx.set_keypoints_chunk(257)
    try:
        _same_bits(scene_ctx.map_keypoints(**cfg), whole, "chunk 257")
        _same_bits(scene_ctx.map_keypoints(1000, 700, **cfg), _cut(whole, 1000, 700), "range, chunk 257")      # neither a multiple of the chunk
    finally:
        scene_ctx.set_keypoints_chunk(0)
    _same_bits(scene_ctx.map_keypoints(1000, 700, **cfg), _cut(whole, 1000, 700), "range")
    # the edge of a workgroup's queries: KK_BLOCK / lanes = 16 with 16 lanes a query (nms_k <= 16), 4 with a wave
    qpb = 16 if nms_k <= 16 else 4
    for n in (qpb - 1, qpb, qpb + 1):
        _same_bits(scene_ctx.map_keypoints(2001, n, **cfg), _cut(whole, 2001, n), "range of %d" % n)
        _same_bits(scene_ctx.map_keypoints(len(fc.scene()) - n, None, **cfg), _cut(whole, len(fc.scene()) - n, n), "the last %d" % n)
    only = scene_ctx.map_keypoints(4000, None, want=(), **cfg)
    assert sorted(only) == ["count", "index", "mask"] and only["mask"].tobytes() == whole["mask"][4000:].tobytes()
    for cell in (0.5, 1.3):                                               # (each a second context, too)
        ctx = _ctx(fc.scene(), cell=cell)
        try:
            _same_bits(ctx.map_keypoints(**cfg), whole, "cell %g" % cell)
        finally:
            ctx.close()


def test_every_combination_of_outputs_gives_the_same_bits(scene_ctx):
    from fast_limo_amd import _lib
    L, h = scene_ctx._L, scene_ctx._h
    first, n = 300, 1234
    cfg = dict(k=20, nms_k=12, max_dist=0.4, nms_max_dist=0.4)
    want = scene_ctx.map_keypoints(first, n, **cfg)
    k = _lib.keypoint_cfg(**cfg)
    for bits_ in range(16):
        mask, sal, cnt, count = np.full(n + 1, 7, np.uint8), np.full(n + 1, 7.0), np.full(n + 1, 7, np.int32), C.c_size_t(7)
        args = [mask.ctypes.data if bits_ & 1 else None, sal.ctypes.data if bits_ & 2 else None, cnt.ctypes.data if bits_ & 4 else None,
                C.byref(count) if bits_ & 8 else None]
        assert L.flimo_map_keypoints(h, first, n, C.byref(k), *args) == 0, bits_
        assert mask[n] == 7 and sal[n] == 7.0 and cnt[n] == 7                                     # nothing beyond n
        assert mask[:n].tobytes() == (want["mask"].astype(np.uint8).tobytes() if bits_ & 1 else b"\x07" * n), bits_
        assert sal[:n].tobytes() == (want["saliency"].tobytes() if bits_ & 2 else np.full(n, 7.0).tobytes()), bits_
        assert cnt[:n].tobytes() == (want["cnt"].tobytes() if bits_ & 4 else np.full(n, 7, np.int32).tobytes()), bits_
        assert count.value == (want["count"] if bits_ & 8 else 7), bits_


@pytest.mark.parametrize("n", [3, 4, 5, 15, 16, 17])
def test_maps_around_a_workgroups_queries(n):
    """Whole maps of qpb - 1, qpb, qpb + 1 points for both lane plans, in the saliency stage and in the suppression."""
    ctx = _ctx(fc.scene()[:n], downsample=False)
    try:
        for k, nms_k in ((3, 2), (16, 16), (17, 17), (64, 64)):
            _same_as_restatement(ctx, dict(k=k, nms_k=nms_k, min_pts=0, gamma21=1.0, gamma32=1.0), "map of %d, k %d" % (n, k))
    finally:
        ctx.close()


# ---- 3. the walk over the tiles ---------------------------------------------------------------------------------------------------------
def test_lists_that_cross_300_m_take_the_walk_and_are_exact(built):
    pts = fc.two_clusters()
    ctx = _ctx(pts)
    try:
        for cfg in (dict(k=64, nms_k=64), dict(k=64, nms_k=64, max_dist=400.0, nms_max_dist=350.0), dict(k=48, nms_k=16, gamma21=1.0, gamma32=1.0),
                    dict(k=12, nms_k=50, gamma21=1.0, gamma32=1.0)):
            out, r = _same_as_restatement(ctx, cfg, "clusters %r" % (cfg,))
            assert np.all(out["cnt"] == cfg["k"])
        idx, _, _ = ctx.knn_k(pts, 64)
        assert np.all((idx[:40] >= 40).sum(1) == 24) and np.all((idx[40:] < 40).sum(1) == 24)      # every list of 64 crosses over
        idx, _, _ = ctx.knn_k(pts, 48)
        assert np.all((idx[:40] >= 40).sum(1) == 8)
        out = ctx.map_keypoints(k=12, nms_k=50, gamma21=1.0, gamma32=1.0)
        assert (~np.isnan(out["saliency"])).sum() > 40 and out["count"] in (1, 2)      # a list of 50 covers its cluster: one maximum each at most
    finally:
        ctx.close()


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,nms_k", [(16, 16), (20, 40)])
def test_of_exact_duplicates_the_lower_index_survives(k, nms_k):
    pts = kc.corner_twice()
    n = len(pts) // 2
    ctx = _ctx(pts, downsample=False)
    try:
        cfg = dict(k=k, nms_k=nms_k)
        out, r = _same_as_restatement(ctx, cfg, "corner twice")
        idx, sqd, cnt = ctx.knn_k(pts, nms_k)
        assert idx[:n].tobytes() == idx[n:].tobytes() and sqd[:n].tobytes() == sqd[n:].tobytes()      # a duplicate's list is its twin's
        nr = ctx.normals_range(0, 2 * n, k, want=("centroid", "cov", "eig"))
        for key in ("cov", "eig", "cnt"):
            assert nr[key][:n].tobytes() == nr[key][n:].tobytes(), key                             # ... and so are its moments
        s = out["saliency"]
        assert s[:n].tobytes() == s[n:].tobytes() and (~np.isnan(s[:n])).sum() > 100                # saliency ties occur
        assert not out["mask"][n:].any() and 0 < out["count"] == int(out["mask"][:n].sum())
        # without the tie rule both twins of a surviving pair would stay: the twin of every keypoint is salient, equal, and suppressed
        assert not np.isnan(s[n:][out["mask"][:n]]).any()
    finally:
        ctx.close()


# ---- 5. a neighbourhood worked by hand --------------------------------------------------------------------------------------------------
def test_a_neighbourhood_worked_by_hand(built):
    """tests/test_keypoints_host.py works the cross out: l2 = 2/7, l1 = l2 / 4, l0 = l1 / 4, exactly -- and here the device's
    eigenvalues ARE those numbers.  gamma = 1/4 fails the strict compare, the next float32 passes."""
    ctx = _ctx(kc.cross(), downsample=False)
    try:
        eig = ctx.normals_range(0, 7, 7, want=("eig",))["eig"]
        assert eig[:, :3].tobytes() == np.tile(np.float64(kc.CROSS_EIG), (7, 1)).tobytes()
        up = kc.above(0.25)
        for k in (7, 64):
            for g21, g32, salient in ((0.25, 0.25, False), (up, 0.25, False), (0.25, up, False), (up, up, True), (1.0, 1.0, True)):
                out, _ = _same_as_restatement(ctx, dict(k=k, nms_k=k, gamma21=g21, gamma32=g32), "cross %g %g" % (g21, g32))
                assert (~np.isnan(out["saliency"])).tolist() == [salient] * 7 and out["mask"].tolist() == [salient] + [False] * 6
                assert out["count"] == int(salient) and np.all(out["cnt"] == 7)
                if salient:
                    assert np.all(out["saliency"] == kc.CROSS_EIG[0])
    finally:
        ctx.close()


def test_a_planar_lattice_patch_is_not_salient_at_any_gamma(built):
    ctx = _ctx(kc.lattice_patch(), downsample=False)
    try:
        for cfg in (dict(k=9, nms_k=9, gamma21=1.0, gamma32=1.0), dict(k=32, nms_k=4, gamma21=0.5, gamma32=1.0), dict(k=64, nms_k=64)):
            eig = ctx.normals_range(0, 100, cfg["k"], want=("eig",))["eig"]
            assert np.all(eig[:, 0] == 0.0) and np.all(eig[:, 1] > 0.0)
            out, _ = _same_as_restatement(ctx, cfg, "patch")
            assert np.isnan(out["saliency"]).all() and not out["mask"].any() and out["count"] == 0 and np.all(out["cnt"] == cfg["k"])
    finally:
        ctx.close()


# ---- 6. a box on a lattice ----------------------------------------------------------------------------------------------------------------
def test_a_box_on_a_lattice_has_no_keypoint_inside_a_face(built):
    """As tests/test_keypoints_host.py shows with brute-force lists: inside a face, farther than the salient gate from every edge,
    a neighbourhood is planar on the lattice and l0 is exactly 0; every keypoint lies on an edge and none at a corner."""
    pts, ijk = kc.box()
    ctx = _ctx(pts, downsample=False)
    try:
        out, r = _same_as_restatement(ctx, kc.BOX_CFG, "box")
        inside = kc.box_face_interior(ijk, kc.BOX_CFG["max_dist"])
        faces = ((ijk == 0) | (ijk == kc.BOX_SIDE)).sum(1)
        print("box: keypoints", out["count"], "by faces met", np.bincount(faces[out["mask"]], minlength=4).tolist())
        assert inside.sum() > 500 and np.isnan(out["saliency"][inside]).all() and not out["mask"][inside].any()
        assert out["count"] >= 12 and np.all(faces[out["mask"]] == 2)
        assert np.isnan(out["saliency"][faces == 3]).all()
    finally:
        ctx.close()


# ---- 7. edge cases ----------------------------------------------------------------------------------------------------------------------
def test_tiny_maps_a_gate_of_zero_and_neighbourhoods_below_three(scene_ctx):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    try:
        out = ctx.map_keypoints(k=8, nms_k=8)                              # an empty map
        assert out["count"] == 0 and out["mask"].shape == (0,) and out["saliency"].shape == (0,) and out["index"].shape == (0,)
    finally:
        ctx.close()
    for n in (1, 2, 3):
        p = F([[1.0, 2.0, 3.0], [1.0, 2.5, 3.0], [1.5, 2.0, 3.0]])[:n]
        ctx = _ctx(p, downsample=False)
        try:
            for k, nms_k in ((3, 2), (64, 64)):
                out, _ = _same_as_restatement(ctx, dict(k=k, nms_k=nms_k, min_pts=0, gamma21=1.0, gamma32=1.0), "map of %d" % n)
                assert out["cnt"].tolist() == [n] * n and np.isnan(out["saliency"]).all() and out["count"] == 0      # three points span a plane
        finally:
            ctx.close()
    n = len(fc.scene())
    out = scene_ctx.map_keypoints(k=16, nms_k=16, max_dist=0.0)           # a salient gate of 0
    assert not out["cnt"].any() and np.isnan(out["saliency"]).all() and not out["mask"].any() and out["count"] == 0 and len(out["mask"]) == n
    out, _ = _same_as_restatement(scene_ctx, dict(k=16, nms_k=16, nms_max_dist=0.0), "a suppression gate of 0")
    assert out["count"] == (~np.isnan(out["saliency"])).sum() > n // 2     # empty lists: nothing suppresses
    sparse = np.ascontiguousarray(fc.scene()[:64] * F(40.0))               # NaN-free, metres apart: cnt < 3 everywhere under a gate of 0.5 m
    ctx = _ctx(sparse)
    try:
        out, _ = _same_as_restatement(ctx, dict(k=8, nms_k=8, max_dist=0.5, min_pts=0), "sparse")
        assert np.all(out["cnt"] < 3) and out["cnt"].any() and np.isnan(out["saliency"]).all() and out["count"] == 0
    finally:
        ctx.close()


# ---- 8. no side effects -----------------------------------------------------------------------------------------------------------------
def test_the_call_changes_neither_map_nor_scan_nor_a_later_pass(built):
    """Against a twin context that never makes the call: the pass before and the pass after have the twin's HTH / HTh bits.  (Two
    passes over one resident scan are not bit-equal to each other, call or no call: the second prunes with the first one's bound.)"""
    from fast_limo_amd import _lib
    mp = fc.scene()
    scan = np.ascontiguousarray(mp[::3] + F([0.01, -0.01, 0.005]))
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809

    def run(search):
        h = _ctx(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if search:
                assert h.map_keypoints(k=16, nms_k=16)["count"] > 0
                h.set_keypoints_chunk(777)
                assert h.map_keypoints(3000, 1000, k=33, nms_k=40, max_dist=1.0, nms_max_dist=0.5)["mask"].shape == (1000,)
            out.append(h.match_reduce(x, mcfg))
            return out, h.map_size(), h.map_points().copy(), h.scan_get().copy(), h.grid_selfcheck()
        finally:
            h.close()

    (plain, pn, pm, ps, pl), (searched, sn, sm, ss, sl_) = run(False), run(True)
    assert pn == sn == len(mp) and pm.tobytes() == sm.tobytes() == mp.tobytes() and ps.tobytes() == ss.tobytes() and pl == sl_
    for a, b in zip(plain, searched):
        print("matches of the pass", a[2], b[2])
        assert a[2] == b[2] > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 9. arguments -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_are_untouched(scene_ctx):
    from fast_limo_amd import _lib
    L, h = scene_ctx._L, scene_ctx._h
    n = len(fc.scene())
    K = lambda **kw: _lib.keypoint_cfg(**dict(dict(k=10, nms_k=10), **kw))
    # (what, cfg, first, n, the code, a word of the message flimo_last_error must then hold)
    cases = [("null cfg", None, 0, n, ERR_INVALID, "null cfg"), ("range beyond the map", K(), 0, n + 1, ERR_INVALID, "beyond"),
             ("first beyond the map", K(), n + 1, 0, ERR_INVALID, "beyond"), ("first + n wraps", K(), 2, 2 ** 64 - 1, ERR_INVALID, "beyond"),
             ("nan gate", K(max_dist=np.nan), 0, n, ERR_INVALID, "max_dist"), ("negative gate", K(max_dist=-1.0), 0, n, ERR_INVALID, "max_dist"),
             ("nan nms gate", K(nms_max_dist=np.nan), 0, n, ERR_INVALID, "suppression"),
             ("negative nms gate", K(nms_max_dist=-0.5), 0, n, ERR_INVALID, "suppression"), ("nan gamma21", K(gamma21=np.nan), 0, n, ERR_INVALID, "gamma"),
             ("gamma21 0", K(gamma21=0.0), 0, n, ERR_INVALID, "gamma"), ("gamma21 above 1", K(gamma21=kc.above(1.0)), 0, n, ERR_INVALID, "gamma"),
             ("gamma21 negative", K(gamma21=-0.5), 0, n, ERR_INVALID, "gamma"), ("nan gamma32", K(gamma32=np.nan), 0, n, ERR_INVALID, "gamma"),
             ("gamma32 0", K(gamma32=0.0), 0, n, ERR_INVALID, "gamma"), ("gamma32 above 1", K(gamma32=1.5), 0, n, ERR_INVALID, "gamma"),
             ("gamma32 inf", K(gamma32=np.inf), 0, n, ERR_INVALID, "gamma"), ("min_pts -1", K(min_pts=-1), 0, n, ERR_INVALID, "min_pts"),
             ("k 2", K(k=2), 0, n, ERR_UNSUPPORTED, " k must"), ("k 65", K(k=65), 0, n, ERR_UNSUPPORTED, " k must"),
             ("k -3", K(k=-3), 0, n, ERR_UNSUPPORTED, " k must"), ("nms_k 1", K(nms_k=1), 0, n, ERR_UNSUPPORTED, "nms_k must"),
             ("nms_k 65", K(nms_k=65), 0, n, ERR_UNSUPPORTED, "nms_k must"), ("nan gate, n 0", K(max_dist=np.nan), 0, 0, ERR_INVALID, "max_dist"),
             ("k 65, n 0", K(k=65), 5, 0, ERR_UNSUPPORTED, " k must")]
    for what, k, first, cnt_n, want, word in cases:
        kp = None if k is None else C.byref(k)
        mask, sal, cnt, count = np.full(n + 1, 7, np.uint8), np.full(n + 1, 7.0), np.full(n + 1, 7, np.int32), C.c_size_t(7)
        assert L.flimo_map_keypoints(h, first, cnt_n, kp, mask.ctypes.data, sal.ctypes.data, cnt.ctypes.data, C.byref(count)) == want, what
        assert np.all(mask == 7) and np.all(sal == 7.0) and np.all(cnt == 7) and count.value == 7, what
        msg = L.flimo_last_error(h).decode()
        assert msg.startswith("map keypoints") and word in msg, (what, msg)
    assert L.flimo_map_keypoints(None, 0, n, C.byref(K()), None, None, None, None) == ERR_INVALID
    # n == 0: *count = 0, nothing else touched; the limits themselves are accepted
    mask, count = np.full(4, 7, np.uint8), C.c_size_t(7)
    assert L.flimo_map_keypoints(h, 17, 0, C.byref(K()), mask.ctypes.data, None, None, C.byref(count)) == 0 and np.all(mask == 7) and count.value == 0
    assert L.flimo_map_keypoints(h, n, 0, C.byref(K()), None, None, None, None) == 0
    assert scene_ctx.map_keypoints(0, 50, k=3, nms_k=2, gamma21=1.0, gamma32=1.0, min_pts=0)["mask"].shape == (50,)
    assert scene_ctx.map_keypoints(0, 50, k=64, nms_k=64, gamma21=1.0e-30, gamma32=1.0e-30)["count"] == 0
    with pytest.raises(ValueError):
        scene_ctx.map_keypoints(want=("saliency", "eig"), k=10)
    assert scene_ctx.map_size() == n
    np.testing.assert_array_equal(scene_ctx.map_points(), fc.scene())
    # an empty map
    ctx = _lib.HipCtx(0)
    try:
        mask, count = np.full(2, 7, np.uint8), C.c_size_t(7)
        assert ctx._L.flimo_map_keypoints(ctx._h, 0, 0, C.byref(K()), mask.ctypes.data, None, None, C.byref(count)) == 0 and np.all(mask == 7) and count.value == 0
        count = C.c_size_t(7)
        assert ctx._L.flimo_map_keypoints(ctx._h, 0, 1, C.byref(K()), mask.ctypes.data, None, None, C.byref(count)) == ERR_INVALID
        assert np.all(mask == 7) and count.value == 7
    finally:
        ctx.close()


# ---- 10. the Localizer's form -------------------------------------------------------------------------------------------------------------
def test_the_localizer_form_equals_the_contexts(built):
    from fast_limo_amd import _lib, api
    cfg = dict(k=20, nms_k=12, max_dist=1.0, nms_max_dist=0.5, gamma21=0.9)
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        out = loc.map_keypoints(**cfg)                                    # no map yet: an empty one's answer
        assert out["count"] == 0 and out["mask"].shape == (0,) and len(out["cnt"]) == 0
        with pytest.raises(api.FlimoError):
            loc.map_keypoints(0, 5, **cfg)
        with pytest.raises(api.FlimoError):
            loc.map_keypoints(k=2)
        with pytest.raises(api.FlimoError):
            loc.map_keypoints(gamma32=0.0)
        loc.map_add(fc.scene())
        n = loc.map_size()
        whole = loc.map_keypoints(**cfg)
        _same_bits(whole, loc.hip.map_keypoints(**cfg), "whole")
        assert 0 < whole["count"] < n
        a, b = loc.map_keypoints(n - 300, 200, want=("cnt",), **cfg), loc.hip.map_keypoints(n - 300, 200, want=("cnt",), **cfg)
        assert sorted(a) == ["cnt", "count", "index", "mask"] and a["mask"].tobytes() == b["mask"].tobytes() and a["cnt"].tobytes() == b["cnt"].tobytes()
        # the C form itself, every output
        k = _lib.keypoint_cfg(**cfg)
        mask, sal, cnt, count = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32), C.c_size_t(0)
        assert loc._L.flimo_loc_map_keypoints(loc._h, 0, n, C.byref(k), mask.ctypes.data, sal.ctypes.data, cnt.ctypes.data, C.byref(count)) == 0
        assert mask.astype(bool).tobytes() == whole["mask"].tobytes() and sal.tobytes() == whole["saliency"].tobytes()
        assert cnt.tobytes() == whole["cnt"].tobytes() and count.value == whole["count"]
        with pytest.raises(api.FlimoError):
            loc.map_keypoints(0, n + 1, **cfg)
    finally:
        loc.close()


# ---- 11. the chain: a pose from the two clouds through their keypoints ----------------------------------------------------------------
# The scan's true pose, the FPFH parameters, the gates and the bars are tests/test_gpu_desc.py's (test_relocalize_from_descriptors).
# The scene is that test's two planes and cylinder FURNISHED with seven boxes (keypoints_common.chain_scene): on the bare scene the
# restatement with brute-force lists finds 40 - 250 keypoints a side of which at most 6 pair up truly, badly spread (an ISS maximum on
# an edge slides along it from one jitter to the next) -- too few for a sample of three.  The un-keypointed chain runs on the same
# furnished scene for the comparison that profiles/keypoints/README.md records.
CHAIN_FPFH = dict(k=64, normal_k=30)
RELOC = dict(ratio=1.0, mutual=True, nh=1 << 20, top=64, corr=dict(edge_sim=0.9, min_edge=1.5, max_dist=0.15), fitness_max_dist=0.5,
             align=dict(k=5, max_dist=1.0, max_curv=0.05, iters=12))
TRUE_T, CHAIN_KEYPOINTS, body_scan = kc.TRUE_T, kc.CHAIN_KEYPOINTS, kc.body_scan


class _Timed:
    """A context whose desc_match calls are timed (the wall time of each call, which ends synchronised)."""

    def __init__(self, ctx):
        self._ctx, self.times = ctx, []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def desc_match(self, *a, **kw):
        t = time.perf_counter()
        out = self._ctx.desc_match(*a, **kw)
        self.times.append(time.perf_counter() - t)
        return out


def _chain(s, keypoints, nh=RELOC["nh"]):
    from fast_limo_amd import api
    body, world, x_true = body_scan(s)
    mp = kc.chain_scene()
    map_ctx, scan_ctx = _Timed(_ctx(mp)), _Timed(_ctx(body))
    try:
        map_ctx.scan_set(body)
        out = api.relocalize(map_ctx, scan_ctx, fpfh=dict(CHAIN_FPFH, viewpoint=TRUE_T), scan_fpfh=dict(CHAIN_FPFH, viewpoint=(0.0, 0.0, 0.0)), seed=s,
                             keypoints=keypoints, **dict(RELOC, nh=nh))
        qi, rj = out["pairs"]
        true = np.linalg.norm(world[qi].astype(np.float64) - mp[rj].astype(np.float64), axis=1) < 0.1
        dt1, dr1 = cc.pose_error(out["fitness"]["x26"][0], x_true)
        dt2, dr2 = cc.pose_error(out["x26"], x_true)
        kp = out.get("keypoints")
        print(f"seed {s} keypoints {'off' if kp is None else '%d scan / %d map' % (len(kp[0]), len(kp[1]))}: {len(body)} scan points, {len(mp)} map points, "
              f"{len(qi)} pairs, {int(true.sum())} true ({true.mean() if len(true) else 0.0:.3f}); nh {nh}; ranked first {dt1:.4f} m {dr1:.3f} deg; "
              f"aligned {dt2 * 1e3:.2f} mm {dr2:.4f} deg; desc_match {sum(map_ctx.times) * 1e3:.2f} + {sum(scan_ctx.times) * 1e3:.2f} ms")
        return out, (body, world, mp), (dt1, dr1, dt2, dr2)
    finally:
        map_ctx.close()
        scan_ctx.close()


@pytest.mark.parametrize("s", [0, 1, 2])
def test_relocalize_through_keypoints(s):
    """api.relocalize(keypoints=..) with the parameters fixed above.  The pairs are the restatement's (desc_common.pairs) on the
    keypoints' FPFH rows, mapped back to the original indices; the first row after the scan_fitness ranking lies within
    tests/test_gpu_corr.py's first bar (0.05 m, 0.5 degrees); scan_align ends within scan_linearize_common's POS_BAR / ROT_BAR_DEG.
    The counts are printed, not asserted: profiles/keypoints/README.md records them.

    Measured on an MI355X with the parameters above: 764 / 781 / 748 keypoints of the scan and 995 of the map, 351 / 331 / 346 pairs of
    which 112 / 97 / 95 are true (32 %, 29 %, 28 %; without keypoints 1 937 pairs, 766 true, 40 %); the first ranked row 0.015 m /
    0.35 deg, 0.004 m / 0.19 deg, 0.004 m / 0.04 deg off; scan_align ends 1.9 mm / 0.057 deg, 1.8 mm / 0.049 deg, 2.6 mm / 0.074 deg off."""
    out, (body, world, mp), (dt1, dr1, dt2, dr2) = _chain(s, CHAIN_KEYPOINTS)
    ks, km = out["keypoints"]
    f_scan, f_map = out["fpfh"]
    assert f_scan.shape == (len(body), 33) and f_map.shape == (len(mp), 33)                        # FPFH of every point
    assert 0 < len(ks) < len(body) and 0 < len(km) < len(mp) and np.all(np.diff(ks) > 0) and np.all(np.diff(km) > 0)
    wi, wj = dc.pairs(f_scan[ks], f_map[km], RELOC["ratio"], RELOC["mutual"])
    qi, rj = out["pairs"]
    assert np.array_equal(qi, ks[wi]) and np.array_equal(rj, km[wj])
    assert np.array_equal(out["src"], body[qi]) and np.array_equal(out["dst"], mp[rj])
    assert dt1 <= 0.05 and dr1 <= 0.5
    assert dt2 <= sl.POS_BAR and dr2 <= sl.ROT_BAR_DEG
    if s == 0:                                                            # the same scene without keypoints, for the record
        _chain(s, None)
