"""GPU: flimo_corr_poses (pose hypotheses from point correspondences: the polygon pre-rejection, the closed-form pose and the count of
the correspondences it explains, per sample of three) through the C ABI, and api.corr_consensus over it.

The yardstick (tests/corr_common.py) is the definition of include/flimo_c.h restated in numpy; status, inliers and the bits of pose,
pair_sqd and sum_sqd are compared with no tolerance, sum_sqd also within m * 2^-52 * fsum of math.fsum.  Wherever two calls must give
the same result the arrays are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import corr_common as cc
import scan_fitness_common as sf
import scan_linearize_common as sl
pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5
INF = float("inf")
CFG = dict(edge_sim=0.8, min_edge=0.5, max_dist=0.3)      # of the small scenes: a fifth to a half of the samples survive
ALL = ("pose", "pair_sqd")


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device; an empty context will do
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def stored():
    return np.concatenate(sf.standard_batches())


def small_scene(m, stored, nh=300):
    """m putative pairs (60 % true; all true for m <= 3), nh samples: distinct indices (all indices 0 for m = 1), every tenth with a
    repeated index."""
    from fast_limo_amd import api
    src, dst, _ = cc.scene(100 + m, stored, m, keep=1.0 if m <= 3 else 0.6)
    tri = api.corr_triplets(m, nh, m) if m >= 3 else np.zeros((nh, 3), np.int32)
    tri[9::10, 2] = tri[9::10, 0]
    return src, dst, tri


@pytest.fixture(scope="module")
def scene513(stored):
    src, dst, tri = small_scene(513, stored)
    return dict(src=src, dst=dst, tri=tri, ref=cc.reference(src, dst, tri, **CFG))


# ---- 1. against the host function and the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 255, 256, 257, 513])
def test_against_the_restatement(hip, stored, m):
    """m around the reduction's 256 threads (one slot each, one short, one more, two rows and one), nh around the count's group of 4
    survivors and its multiples (with m = 3 nine samples of ten survive) and past one solve workgroup.  The reference of the 300
    samples is computed once; a smaller nh is a prefix."""
    from fast_limo_amd import api
    src, dst, tri = small_scene(m, stored)
    ref = cc.reference(src, dst, tri, **CFG)
    counts = [int((ref["status"] == s).sum()) for s in (cc.OK, cc.DEGENERATE, cc.REJECTED)]
    print(f"m {m}: OK / DEGENERATE / REJECTED {counts}, inliers up to {ref['inliers'].max()}")
    assert counts[1] >= 30 and (m < 255 or (counts[0] >= 16 and counts[2] >= 16 and ref["inliers"].max() > 0.4 * m))
    for nh in (1, 4, 5, 7, 8, 9, 65, 300):
        got = hip.corr_poses(src, dst, tri[:nh], want=ALL, **CFG)
        cc.check(got, {k: v[:nh] for k, v in ref.items()}, f"m {m}, nh {nh}")
        bad = got["status"] != cc.OK
        assert np.all(got["inliers"][bad] == 0) and np.all(got["sum_sqd"][bad].view(np.uint64) == 0) and np.all(got["pair_sqd"][bad] == -1)
    # the solve kernel runs the host function: the same status, pose bits and matrix for every sample
    for j in range(0, 300, 7):
        st, pose, rt = api.corr_pose_host(src[tri[j]], dst[tri[j]], **CFG)
        if len(set(tri[j])) < 3:
            st, pose = cc.DEGENERATE, np.full(7, np.nan)
        assert st == got["status"][j] and np.array_equal(pose, got["pose"][j], equal_nan=True), j
        if st == cc.OK:
            assert np.array_equal(rt, ref["rt"][j]), j


def test_the_sum_is_the_stated_shape_written_out(hip, stored):
    """sum_sqd against the header's shape written out with Python floats over the call's own pair_sqd, for 600 pairs (two rows of
    256 and a part of a third): partial t adds slots t, t + 256, .. in ascending order, a non-inlier adds nothing, then
    partial[t] += partial[t + o] for o = 128 .. 1.  corr_common.tree_sum, the yardstick of every other test, is held to it as well."""
    import math
    src, dst, tri = small_scene(600, stored, nh=40)
    got = hip.corr_poses(src, dst, tri, want=ALL, **CFG)
    ok = np.nonzero(got["status"] == cc.OK)[0]
    assert ok.size >= 4
    for j in ok:
        v = got["pair_sqd"][j]
        partial = [0.0] * 256
        for i, x in enumerate(v):
            if x >= 0:
                partial[i % 256] = partial[i % 256] + float(x)
        o = 128
        while o >= 1:
            for t in range(o):
                partial[t] = partial[t] + partial[t + o]
            o //= 2
        assert got["sum_sqd"][j] == partial[0] == cc.tree_sum(v) and got["inliers"][j] == int((v >= 0).sum()), j
        assert abs(partial[0] - math.fsum(float(x) for x in v if x >= 0)) <= sf.sum_bound(600, partial[0])
    assert 0 < got["inliers"][ok].max() < 600      # (some slots of a row add, some do not)
    assert cc.tree_sum(np.float32([])) == 0.0 and cc.tree_sum(np.float32([-1, -1])) == 0.0


# ---- 2. invariance of the bits ---------------------------------------------------------------------------------------------------
def test_the_bits_do_not_depend_on_the_batch_the_order_or_the_chunks(hip, scene513):
    src, dst, tri, ref = (scene513[k] for k in ("src", "dst", "tri", "ref"))
    first = hip.corr_poses(src, dst, tri, want=ALL, **CFG)
    cc.check(first, ref, "the whole batch")
    cc.same_bytes(first, hip.corr_poses(src, dst, tri, want=ALL, **CFG), "called twice")
    some = np.concatenate([np.nonzero(ref["status"] == cc.OK)[0][:12], np.nonzero(ref["status"] != cc.OK)[0][:4]])
    single = [hip.corr_poses(src, dst, tri[j:j + 1], want=ALL, **CFG) for j in some]
    cc.same_bytes({k: v[some] for k, v in first.items()}, {k: np.concatenate([r[k] for r in single]) for k in first}, "nh = 1 per hypothesis")
    back = hip.corr_poses(src, dst, tri[::-1], want=ALL, **CFG)
    cc.same_bytes(first, {k: v[::-1] for k, v in back.items()}, "the batch reversed")
    order = np.random.RandomState(1).permutation(len(tri))
    mixed = hip.corr_poses(src, dst, tri[order], want=ALL, **CFG)
    cc.same_bytes({k: v[order] for k, v in first.items()}, mixed, "the batch permuted")
    try:
        for n in (1, 3, 64, 0):
            hip.set_corr_chunk(n)
            cc.same_bytes(first, hip.corr_poses(src, dst, tri, want=ALL, **CFG), f"chunks of {n}")
    finally:
        hip.set_corr_chunk(0)


def test_the_bits_do_not_depend_on_the_other_hypotheses_or_on_the_outputs_asked_for(hip, scene513):
    src, dst, tri, ref = (scene513[k] for k in ("src", "dst", "tri", "ref"))
    first = hip.corr_poses(src, dst, tri, want=ALL, **CFG)
    ok = np.nonzero(ref["status"] == cc.OK)[0]
    # every other hypothesis made degenerate (a repeated index): the survivors share their workgroups with other ones, or with none
    for keep in (ok[::2], ok[:1], ok[5:14]):
        alone = tri.copy()
        drop = np.setdiff1d(np.arange(len(tri)), keep)
        alone[drop, 1] = alone[drop, 0]
        got = hip.corr_poses(src, dst, alone, want=ALL, **CFG)
        assert np.all(got["status"][drop] == cc.DEGENERATE) and np.all(got["status"][keep] == cc.OK)
        cc.same_bytes({k: v[keep] for k, v in first.items()}, {k: v[keep] for k, v in got.items()}, f"{len(keep)} survivors left")
    # ... and without pre-rejection, where every sample with distinct, non-degenerate points survives
    loose = dict(CFG, edge_sim=0.0)
    wide = hip.corr_poses(src, dst, tri, want=ALL, **loose)
    assert (wide["status"] == cc.OK).sum() > 2 * ok.size
    cc.same_bytes({k: v[ok] for k, v in first.items()}, {k: v[ok] for k, v in wide.items()}, "no pre-rejection")
    for want in ((), ("pose",), ("pair_sqd",)):
        got = hip.corr_poses(src, dst, tri, want=want, **CFG)
        assert sorted(got) == sorted(("status", "inliers", "sum_sqd") + want)
        cc.same_bytes(got, first, f"want {want}", names=sorted(got))


# ---- 3. consistency with flimo_scan_fitness ----------------------------------------------------------------------------------------
def x26_rows(pose):
    x = np.zeros((pose.shape[0], 26))
    x[:, 0:7] = pose
    x[:, 10] = 1.0
    return x


def test_an_inlier_pair_is_no_closer_than_the_scans_nearest_stored_point(built, hip, scene513):
    """dst loaded as the map of a second context (no downsampling: every point is stored), src as its resident scan: the world point
    of pair i under a hypothesis is scan_fitness' w(j, i) bit for bit, dst[i] is one of the stored points, so nn_sqd <= sqd_i."""
    from fast_limo_amd import _lib
    src, dst, tri, ref = (scene513[k] for k in ("src", "dst", "tri", "ref"))
    got = hip.corr_poses(src, dst, tri, want=ALL, **CFG)
    ok = np.nonzero(got["status"] == cc.OK)[0][:24]
    other = _lib.HipCtx(0)
    try:
        other.map_config(downsample=False)
        other.map_add(dst)
        other.scan_set(src)
        assert other.map_size() == dst.shape[0]
        inl, _, nn_sqd, _ = other.scan_fitness(x26_rows(got["pose"][ok]), INF, want_nn=True)
    finally:
        other.close()
    pairs = got["pair_sqd"][ok]
    is_in = pairs >= 0
    assert is_in.sum() > 200 and np.all(inl == src.shape[0])
    assert np.all(nn_sqd[is_in] <= pairs[is_in])
    assert (nn_sqd[is_in] == pairs[is_in]).mean() > 0.5      # (mostly the mate itself)


def test_on_a_lattice_map_an_inlier_pairs_distance_is_scan_fitness_own(built, hip):
    """The construction: dst = 343 points of the integer lattice {-3..3}^3 in a random order -- stored points 1 m apart --, src = the
    true pose's inverse of dst plus up to 0.05 m per coordinate, every pair true.  With max_dist 0.3 m an inlier's world point lies
    within 0.3 m of dst[i] and at least 0.7 m from every other stored point: dst[i] is its unique nearest stored point, so
    scan_fitness' nn_idx is i and its nn_sqd equals pair_sqd bit for bit; with the same gate the inlier counts and sums of a pose that
    brings no point within 0.3 m of a wrong lattice point are equal too."""
    from fast_limo_amd import _lib, api
    rs = np.random.RandomState(4)
    g = np.arange(-3, 4, dtype=np.float64)
    dst = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rs.permutation(343)]
    x_true = sf.x26_of()
    R = sf.pose_rt(x_true).astype(np.float64)
    src = ((dst - R[:, 3]) @ R[:, :3] + (rs.rand(343, 3) - 0.5) * 0.1).astype(np.float32)
    dst = dst.astype(np.float32)
    tri = api.corr_triplets(343, 96, 4)
    cfg = dict(edge_sim=0.9, min_edge=1.0, max_dist=0.3)
    got = hip.corr_poses(src, dst, tri, want=ALL, **cfg)
    cc.check(got, cc.reference(src, dst, tri, **cfg), "lattice")
    ok = np.nonzero(got["status"] == cc.OK)[0]
    assert ok.size >= 48
    other = _lib.HipCtx(0)
    try:
        other.map_config(downsample=False)
        other.map_add(dst)
        other.scan_set(src)
        assert other.map_size() == 343 and np.array_equal(other.map_points(), dst)
        inl, s, nn_sqd, nn_idx = other.scan_fitness(x26_rows(got["pose"][ok]), 0.3, want_nn=True)
    finally:
        other.close()
    pairs = got["pair_sqd"][ok]
    is_in = pairs >= 0
    assert is_in.sum() > 0.5 * is_in.size
    assert np.array_equal(nn_sqd[is_in].view(np.uint32), pairs[is_in].view(np.uint32))
    assert np.array_equal(nn_idx[is_in], np.broadcast_to(np.arange(343), pairs.shape)[is_in])
    clean = np.all((nn_idx >= 0) == is_in, axis=1)      # poses whose scan_fitness inliers are the pairs' own
    assert clean.sum() >= 24
    assert np.array_equal(inl[clean], got["inliers"][ok][clean])
    assert np.array_equal(s[clean].view(np.uint64), got["sum_sqd"][ok][clean].view(np.uint64))      # (the same shape over the same slots)


# ---- 4. edges and errors -----------------------------------------------------------------------------------------------------------
def test_all_rejected_all_degenerate_and_the_gates_ends(hip, scene513):
    src, dst, tri = (scene513[k] for k in ("src", "dst", "tri"))
    m = src.shape[0]
    distinct = tri[:, 2] != tri[:, 0]
    got = hip.corr_poses(src, dst, tri, want=ALL, edge_sim=1.0, min_edge=0.0, max_dist=0.3)      # (noisy pairs: no congruent triangle)
    cc.check(got, cc.reference(src, dst, tri, edge_sim=1.0, min_edge=0.0, max_dist=0.3), "all rejected")
    assert np.all(got["status"][distinct] == cc.REJECTED) and np.all(got["status"][~distinct] == cc.DEGENERATE)
    got = hip.corr_poses(src, dst, tri, want=ALL, edge_sim=0.0, min_edge=1000.0, max_dist=0.3)
    assert np.all(got["status"] == cc.DEGENERATE) and np.all(got["inliers"] == 0) and np.all(got["sum_sqd"].view(np.uint64) == 0)
    assert np.isnan(got["pose"]).all() and np.all(got["pair_sqd"] == -1)
    for gate in (0.0, INF):
        cfg = dict(CFG, max_dist=gate)
        ref = cc.reference(src, dst, tri, **cfg)
        got = hip.corr_poses(src, dst, tri, want=ALL, **cfg)
        cc.check(got, ref, f"max_dist {gate}")
        ok = got["status"] == cc.OK
        assert ok.sum() >= 16
        if gate == 0.0:
            assert np.all(got["inliers"] == 0) and np.all(got["pair_sqd"] == -1) and not np.isnan(got["pose"][ok]).any()
        else:
            assert np.all(got["inliers"][ok] == m) and np.all(got["pair_sqd"][ok] >= 0)


def test_a_nan_in_a_pair_that_is_in_no_triplet(hip, scene513):
    src, dst, tri = (scene513[k].copy() for k in ("src", "dst", "tri"))
    free = np.setdiff1d(np.arange(src.shape[0]), tri.reshape(-1))[:2]
    assert free.size == 2
    src[free[0], 1] = np.nan
    dst[free[1], 2] = np.nan
    for gate in (CFG["max_dist"], INF):
        cfg = dict(CFG, max_dist=gate)
        got = hip.corr_poses(src, dst, tri, want=ALL, **cfg)
        cc.check(got, cc.reference(src, dst, tri, **cfg), f"NaN pairs, gate {gate}")
        ok = got["status"] == cc.OK
        assert ok.sum() >= 16 and np.all(got["pair_sqd"][:, free] == -1) and np.all(got["inliers"][ok] <= src.shape[0] - 2)
    cc.same_bytes({k: v for k, v in got.items() if k in ("status", "pose")},
                  {k: v for k, v in hip.corr_poses(scene513["src"], scene513["dst"], tri, want=ALL, **cfg).items() if k in ("status", "pose")},
                  "the poses do not see them")


def test_rejected_arguments_and_limits_leave_the_outputs_alone(hip, scene513):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    src, dst, tri = scene513["src"], scene513["dst"], np.ascontiguousarray(scene513["tri"][:4])
    m = src.shape[0]
    status, inl, s = np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7.0)
    pose, pairs = np.full((4, 7), 7.0), np.full((4, m), 7, np.float32)
    good = _lib.corr_cfg(**CFG)

    def call(src_p=src.ctypes.data, dst_p=dst.ctypes.data, m_=m, tri_p=tri.ctypes.data, nh=4, cfg=good, status_p=status.ctypes.data,
             inl_p=inl.ctypes.data, s_p=s.ctypes.data, pose_p=pose.ctypes.data, pairs_p=pairs.ctypes.data):
        return L.flimo_corr_poses(hip._h, src_p, dst_p, m_, tri_p, nh, None if cfg is None else C.byref(cfg), status_p, inl_p, s_p, pose_p, pairs_p)
    for kw in (dict(src_p=None), dict(dst_p=None), dict(tri_p=None), dict(cfg=None), dict(status_p=None), dict(inl_p=None), dict(s_p=None)):
        assert call(**kw) == ERR_INVALID, kw
    for bad in ((-0.1, 0.5, 0.3), (1.0001, 0.5, 0.3), (float("nan"), 0.5, 0.3), (0.8, -0.5, 0.3), (0.8, float("nan"), 0.3), (0.8, 0.5, -0.3),
                (0.8, 0.5, float("nan")), (0.8, INF, float("nan"))):
        assert call(cfg=_lib.corr_cfg(*bad)) == ERR_INVALID, bad
    for at, v in ((0, -1), (5, m), (11, 2 ** 31 - 1), (7, -2 ** 31)):
        t = tri.copy()
        t.reshape(-1)[at] = v
        assert call(tri_p=t.ctypes.data) == ERR_INVALID, (at, v)
        assert b"outside" in L.flimo_last_error(hip._h)
    assert call(m_=0) == ERR_INVALID                                   # (no index lies in [0, 0))
    assert call(m_=2 ** 31) == ERR_TOO_LARGE and call(nh=2 ** 31) == ERR_TOO_LARGE
    assert call(m_=2 ** 15, nh=2 ** 16) == ERR_TOO_LARGE               # nh * m = 2^31 with pair_sqd asked for
    for a in (status, inl, s, pose, pairs):
        assert np.all(a == 7)
    assert call(nh=0) == 0 and call(nh=0, tri_p=None) == 0
    for a in (status, inl, s, pose, pairs):
        assert np.all(a == 7)
    # the arrays were good all along; the optional ones may be left out
    assert call(pose_p=None, pairs_p=None) == 0 and np.all(pose == 7) and np.all(pairs == 7) and not np.all(status == 7)
    assert call() == 0
    ref = cc.reference(src, dst, tri, **CFG)
    cc.check(dict(status=status, inliers=inl, sum_sqd=s, pose=pose, pair_sqd=pairs), ref, "through ctypes")
    with pytest.raises(ValueError):
        hip.corr_poses(src, dst, tri, want=("rt",), **CFG)
    with pytest.raises(ValueError):
        hip.corr_poses(src, dst[:-1], tri, **CFG)
    with pytest.raises(_lib.FlimoError):
        hip.corr_poses(src, dst, tri, edge_sim=2.0)


def test_the_localizer_forwards(hip, scene513):
    from fast_limo_amd import api
    src, dst, tri = (scene513[k] for k in ("src", "dst", "tri"))
    first = hip.corr_poses(src, dst, tri, want=ALL, **CFG)
    loc = api.Localizer(api.default_cfg())
    try:
        cc.same_bytes(first, loc.corr_poses(src, dst, tri, want=ALL, **CFG), "Localizer with no map")
        loc.map_add(np.concatenate(sf.standard_batches()[:1]))
        size = loc.map_size()
        cc.same_bytes(first, loc.corr_poses(src, dst, tri, want=ALL, **CFG), "Localizer with a map")
        assert loc.map_size() == size
        with pytest.raises(api.FlimoError):
            loc.corr_poses(src, dst, tri, edge_sim=-1.0)
    finally:
        loc.close()


# ---- 5. recovery: from putative pairs to a refined pose -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mapped(built):
    """The standard map with standard_scan(512) resident: what scan_fitness and scan_align of the recovered rows run against."""
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    for b in sf.standard_batches():
        ctx.map_add(b)
    ctx.scan_set(sf.standard_scan(512))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_recovery_from_thirty_percent_true_pairs(mapped, seed):
    """512 pairs of which about 30 % are true (their dst: the scan's world point at the true pose plus N(0, 0.01)), the rest random
    stored points; 2048 samples, edge_sim 0.9, min_edge 0.5 m, max_dist 0.15 m.  First bar: the first row of api.corr_consensus lies
    within 0.05 m and 0.5 degrees of the true pose (the numpy restatement on these seeds: at most 0.0071 m and 0.047 degrees,
    tests/test_corr_host.py).  Second bar: api.scan_align from that row ends within test_gpu_scan_linearize.py's 1 cm and 0.1 degrees."""
    from fast_limo_amd import api
    src, dst, true = cc.scene(seed, mapped.map_points())
    cfg = dict(edge_sim=0.9, min_edge=0.5, max_dist=0.15)
    best = api.corr_consensus(mapped, src, dst, 2048, seed=seed, **cfg)
    dt, dr = cc.pose_error(best["x26"][0], sf.x26_of())
    print(f"seed {seed}: {int(true.sum())} true pairs, {best['survivors']} survivors, best has {best['inliers'][0]} inliers, off by {dt:.4f} m, {dr:.3f} deg")
    # the rows are the restatement's ranking of the same samples
    ref = cc.reference(src, dst, best["tri"], **cfg)
    assert np.array_equal(ref["inliers"], best["inliers"]) and np.array_equal(ref["sum_sqd"], best["sum_sqd"])
    assert np.array_equal(ref["pose"], best["x26"][:, 0:7]) and np.all(best["x26"][:, 10] == 1.0) and np.all(best["x26"][:, 11:] == 0.0)
    assert best["x26"].shape == (8, 26) and np.all(np.diff(best["inliers"]) <= 0) and 8 <= best["survivors"] < 2048
    assert dt <= 0.05 and dr <= 0.5
    assert sl.pose_error(best["x26"][0])[0] == pytest.approx(dt, abs=1e-12)
    # the rows feed the two calls that exist
    inl, s = mapped.scan_fitness(best["x26"], 0.5)
    assert inl[0] >= 0.9 * src.shape[0]
    res = api.scan_align(mapped, best["x26"][:1], k=5, max_dist=1.0, max_curv=0.05, iters=12)
    dp, da = sl.pose_error(res["x26"][0])
    print(f"seed {seed}: scan_fitness inliers {inl[0]} of {src.shape[0]}; scan_align -> {dp * 1e3:.2f} mm, {da:.4f} deg")
    assert dp <= sl.POS_BAR and da <= sl.ROT_BAR_DEG
