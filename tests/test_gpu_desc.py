"""GPU suite: nearest descriptors -- flimo_desc_ref_set / flimo_desc_match, the dot products on v_mfma_f32_32x32x2_f32.  The yardstick
is the definition of include/flimo_c.h restated in numpy (tests/desc_common.py, whose fmaf tests/test_desc_host.py holds to libm's):
cnt, idx and the BITS of dist are compared with no tolerance at every edge of the tiling, for every dim and k, on exact ties, on
real FPFH rows and on rows that must be excluded; chunks, splits, the other queries and repetition move no bit.  The last test
relocalises a scan in a map from the two clouds alone (api.relocalize)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import corr_common as cc
import desc_common as dc
import fpfh_common as fc
import scan_fitness_common as sf
import scan_linearize_common as sl
from common import CAPS

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -5, -6
F = np.float32
NQS = (1, 31, 32, 33, 127, 128, 129, 257)
NRS = (1, 2, 31, 33, 127, 129, 1025, 4099)
FPFH = dict(k=10, normal_k=10)


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_desc_ref_set", "flimo_desc_match", "flimo_desc_dist_host", "flimo_set_desc_chunk"):
        getattr(L, name)
    getattr(H, "flimo_loc_desc_match")


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device; an empty context will do
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def default_chunks(hip):
    yield
    hip.set_desc_chunk(0, 0)


@functools.lru_cache(maxsize=None)
def base():
    """257 queries, 4 099 references, dim 33, and every pair's restated distance: the sub-shapes are its corners (a pair's distance
    depends on its two rows alone)."""
    Q, R = dc.random_rows(11, 257, 33), dc.random_rows(12, 4099, 33)
    return Q, R, dc.dist_matrix(Q, R)


def same(got, want, tag):
    np.testing.assert_array_equal(got["cnt"], want["cnt"], err_msg=f"{tag}: cnt")
    np.testing.assert_array_equal(got["idx"], want["idx"], err_msg=f"{tag}: idx")
    np.testing.assert_array_equal(dc.bits(got["dist"]), dc.bits(want["dist"]), err_msg=f"{tag}: dist bits")


def same_bytes(a, b, tag):
    for name in ("idx", "dist", "cnt"):
        assert a[name].tobytes() == b[name].tobytes(), f"{tag}: {name}"


def _map_ctx(pts):
    """The whole cloud as the first add: the first build neither drops points nor merges duplicates."""
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, True, 0.0)
    ctx.map_add(pts, stamp=0.5)
    assert ctx.map_size() == len(pts)
    return ctx


# ---- 1. shapes around every edge of the tiling ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr", NRS)
def test_shapes_around_every_edge_of_the_tiling(hip, nr):
    """dim 33, k 2: query counts around the tile of 32 and the workgroup's 128, reference counts around the tile of 32 and across the
    splits -- the default's (1 024 rows at least) and splits of 128 rows, which every nr above 128 crosses."""
    Q, R, D = base()
    hip.desc_ref_set(R[:nr])
    assert hip.desc_ref_size() == nr and hip.desc_ref_dim() == 33
    for split in (0, 128):
        hip.set_desc_chunk(0, split)
        for nq in NQS:
            same(hip.desc_match(Q[:nq], k=2), dc.match(Q[:nq], R[:nr], 2, D=D[:nq, :nr]), f"nq {nq}, nr {nr}, split {split}")


# ---- 2. other dims and k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3, 32, 33, 34, 63, 64])
def test_other_dims_and_k(hip, dim):
    """97 queries against 300 references, and against 3 (fewer than k: the slots beyond cnt are padded), at every kernel variant's
    dim and list length; signed rows as well."""
    rs = np.random.RandomState(dim)
    for Q, R in ((dc.random_rows(20 + dim, 97, dim), dc.random_rows(40 + dim, 300, dim)),
                 (rs.standard_normal((97, dim)).astype(F), rs.standard_normal((300, dim)).astype(F))):
        D = dc.dist_matrix(Q, R)
        for n in (300, 3):
            hip.desc_ref_set(R[:n])
            for k in (1, 2, 5, 8):
                want = dc.match(Q, R[:n], k, D=D[:, :n])
                got = hip.desc_match(Q, k=k)
                same(got, want, f"dim {dim}, nr {n}, k {k}")
                assert got["idx"].shape == (97, k) and np.all(got["cnt"] == min(k, n))
                assert np.all(got["idx"][:, n:] == -1) and np.all(dc.bits(got["dist"][:, n:]) == 0)


# ---- 3. exact ties -------------------------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_lowest_index(hip):
    """Rows of zeros and ones: d is the Hamming distance and over a hundred references tie at a query's commonest distance.  One row stored at 5, 37, 700 and
    1 299 -- four tiles, and with splits of 128 rows four splits --, another at 64 .. 95 (one whole tile)."""
    Q, R = dc.tie_scene()
    D = dc.dist_matrix(Q, R)
    want_int = ((Q[:, None, :].astype(np.int64) - R[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
    assert np.array_equal(D.astype(np.int64), want_int)
    ties = [np.unique(row, return_counts=True)[1].max() for row in want_int]
    print("largest group of equal distances per query: min", min(ties), "max", max(ties))
    assert min(ties) >= 100
    hip.desc_ref_set(R)
    for chunk, split in ((0, 0), (0, 128), (32, 32), (0, 640)):
        hip.set_desc_chunk(chunk, split)
        for k in (1, 2, 8):
            got = hip.desc_match(Q, k=k)
            same(got, dc.match(Q, R, k, D=D), f"chunk {chunk}, split {split}, k {k}")
        assert list(got["idx"][0, :4]) == [5, 37, 700, 1299] and np.all(dc.bits(got["dist"][0, :4]) == 0)
        assert list(got["idx"][1]) == list(range(64, 72)) and np.all(dc.bits(got["dist"][1]) == 0)


# ---- 4. invariance -------------------------------------------------------------------------------------------------------------------
def test_the_bits_do_not_move_with_chunks_splits_the_other_queries_or_repetition(hip):
    Q, R, D = base()
    hip.desc_ref_set(R)
    first = hip.desc_match(Q, k=2)
    same(first, dc.match(Q, R, 2, D=D), "default")
    same_bytes(first, hip.desc_match(Q, k=2), "the call again")
    hip.desc_ref_set(R.copy())
    same_bytes(first, hip.desc_match(Q, k=2), "the same rows set again")
    for chunk, split in ((32, 32), (33, 96), (100, 0), (0, 4096)):
        hip.set_desc_chunk(chunk, split)
        same_bytes(first, hip.desc_match(Q, k=2), f"chunk {chunk}, split {split}")
    hip.set_desc_chunk(0, 0)
    for sel in (slice(0, 100), slice(50, 60), slice(256, 257), slice(None, None, -1)):
        part = hip.desc_match(Q[sel], k=2)
        same_bytes(part, {n: np.ascontiguousarray(first[n][sel]) for n in first}, f"queries {sel}")
    # k = 8 and its prefix
    eight = hip.desc_match(Q, k=8)
    same(eight, dc.match(Q, R, 8, D=D), "k 8")
    assert np.array_equal(eight["idx"][:, :2], first["idx"]) and np.array_equal(dc.bits(eight["dist"][:, :2]), dc.bits(first["dist"]))


def test_the_host_function_returns_the_devices_distance(hip):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    Q, R, _ = base()
    hip.desc_ref_set(R)
    got = hip.desc_match(Q, k=2)
    d = np.zeros(1, F)
    for i in range(Q.shape[0]):
        for j in range(2):
            r = np.ascontiguousarray(R[got["idx"][i, j]])
            assert L.flimo_desc_dist_host(Q[i].ctypes.data, r.ctypes.data, 33, d.ctypes.data) == 0
            assert dc.bits(d)[0] == dc.bits(got["dist"])[i, j], (i, j)


# ---- 5. real descriptors ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_fpfh(seed):
    ctx = _map_ctx(fc.scene(seed))
    try:
        rows = ctx.map_fpfh(want=(), **FPFH)["fpfh"]
    finally:
        ctx.close()
    rows.setflags(write=False)
    return rows


def test_real_fpfh_rows(hip):
    """The FPFH rows of the scene as references, those of the same surfaces under another jitter and order as queries, their all-zero
    rows included."""
    R, Q = scene_fpfh(7), scene_fpfh(8)
    zq, zr = int((~Q.any(axis=1)).sum()), int((~R.any(axis=1)).sum())
    print(f"all-zero rows: {zq} of {len(Q)} queries, {zr} of {len(R)} references; largest norm {float(dc.norms(R).max()):.1f}")
    hip.desc_ref_set(R)
    got = hip.desc_match(Q, k=2)
    same(got, dc.match(Q, R, 2), "fpfh")
    assert np.all(got["cnt"] == 2)


# ---- 6. exclusions -------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_and_overflowing_pairs_are_excluded(hip):
    Q, R, _ = base()
    Q, R = Q[:70].copy(), R[:200].copy()
    Q[3, 7] = np.nan            # a query with a NaN
    Q[40] = 1.0e20              # every chain of this row with itself or its like overflows
    Q[41, 32] = -np.inf
    R[5, 0] = np.nan            # never returned
    R[33, 32] = np.inf          # never returned
    R[64] = 1.0e20              # against an ordinary query d = +inf: a distance like any other, the last in the order
    R[100] = 1.0e20
    D = dc.dist_matrix(Q, R)
    assert np.isnan(D[3]).all() and np.isnan(D[41]).all() and np.isnan(D[:, 5]).all() and np.isnan(D[:, 33]).all()
    assert np.isnan(D[40, 64]) and np.isnan(D[40, 100]) and np.isposinf(D[0, 64]) and np.isposinf(D[40, 0])
    hip.desc_ref_set(R)
    for k in (2, 8):
        got = hip.desc_match(Q, k=k)
        same(got, dc.match(Q, R, k, D=D), f"k {k}")
        assert got["cnt"][3] == 0 and got["cnt"][41] == 0 and np.all(got["idx"][3] == -1) and np.all(dc.bits(got["dist"][3]) == 0)
        assert not np.isin(got["idx"], [5, 33]).any()
        # the huge query: +inf to every ordinary row, in index order; NaN to the huge rows
        assert list(got["idx"][40]) == [j for j in range(200) if j not in (5, 33, 64, 100)][:k] and np.all(np.isposinf(got["dist"][40]))
    # only excluded and huge rows resident: an ordinary query finds the huge ones at +inf, the huge query nothing
    hip.desc_ref_set(R[[5, 33, 64, 100]])
    got = hip.desc_match(Q[[0, 40]], k=8)
    assert list(got["cnt"]) == [2, 0] and list(got["idx"][0, :3]) == [2, 3, -1] and np.all(np.isposinf(got["dist"][0, :2]))


# ---- 7. trivial and rejected calls ---------------------------------------------------------------------------------------------------
def test_trivial_and_rejected_calls_leave_the_outputs_alone(built):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    Q, R, _ = base()
    Q = np.ascontiguousarray(Q[:4])
    ctx = _lib.HipCtx(0)
    try:
        # no resident set
        assert ctx.desc_ref_size() == 0 and ctx.desc_ref_dim() == 0
        got = ctx.desc_match(Q, k=3)
        assert np.all(got["cnt"] == 0) and np.all(got["idx"] == -1) and np.all(dc.bits(got["dist"]) == 0) and got["idx"].shape == (4, 3)
        ctx.desc_ref_set(R[:50])
        assert ctx.desc_ref_size() == 50 and ctx.desc_ref_dim() == 33
        idx, dist, cnt = np.full((4, 2), 7, np.int32), np.full((4, 2), 7, F), np.full(4, 7, np.int32)

        def call(q_p=Q.ctypes.data, nq=4, dim=33, k=2, idx_p=idx.ctypes.data, dist_p=dist.ctypes.data, cnt_p=cnt.ctypes.data):
            return L.flimo_desc_match(ctx._h, q_p, nq, dim, k, idx_p, dist_p, cnt_p)
        for kw in (dict(q_p=None), dict(idx_p=None), dict(dist_p=None), dict(cnt_p=None), dict(dim=32), dict(dim=34), dict(dim=1)):
            assert call(**kw) == ERR_INVALID, kw
        for kw in (dict(dim=0), dict(dim=-3), dict(dim=65), dict(k=0), dict(k=9), dict(k=-1)):
            assert call(**kw) == ERR_UNSUPPORTED, kw
        for kw in (dict(nq=2 ** 31), dict(nq=2 ** 30, k=2), dict(nq=2 ** 28, k=8)):
            assert call(**kw) == ERR_TOO_LARGE, kw
        assert L.flimo_desc_ref_set(ctx._h, None, 5, 33) == ERR_INVALID
        assert L.flimo_desc_ref_set(ctx._h, R.ctypes.data, 5, 0) == ERR_UNSUPPORTED
        assert L.flimo_desc_ref_set(ctx._h, R.ctypes.data, 5, 65) == ERR_UNSUPPORTED
        assert L.flimo_desc_ref_set(ctx._h, R.ctypes.data, 2 ** 31, 33) == ERR_TOO_LARGE
        assert np.all(idx == 7) and np.all(dist == 7) and np.all(cnt == 7)
        assert ctx.desc_ref_size() == 50      # (a rejected set leaves the resident one)
        assert call(nq=0) == 0 and call(nq=0, q_p=None) == 0
        assert np.all(idx == 7) and np.all(dist == 7) and np.all(cnt == 7)
        assert call() == 0
        same(dict(idx=idx, dist=dist, cnt=cnt), dc.match(Q, R[:50], 2), "through ctypes")
        with pytest.raises(_lib.FlimoError):
            ctx.desc_match(Q[:, :32])
        # another dim replaces the set; no rows clear it
        ctx.desc_ref_set(R[:10, :5])
        assert (ctx.desc_ref_size(), ctx.desc_ref_dim()) == (10, 5)
        same(ctx.desc_match(Q[:, :5], k=2), dc.match(Q[:, :5], R[:10, :5], 2), "dim 5")
        ctx.desc_ref_set(R[:0])
        assert (ctx.desc_ref_size(), ctx.desc_ref_dim()) == (0, 0)
        assert np.all(ctx.desc_match(Q, k=2)["cnt"] == 0) and np.all(ctx.desc_match(Q[:, :7], k=1)["idx"] == -1)
    finally:
        ctx.close()


# ---- 8. no side effects, the Localizer -----------------------------------------------------------------------------------------------
def test_the_calls_touch_neither_the_map_nor_the_scan_nor_a_later_pass():
    """Against a twin context that never makes the calls: the pass before and the pass after have the twin's HTH / HTh bits."""
    from fast_limo_amd import _lib
    mp = fc.scene()
    scan = np.ascontiguousarray(mp[::3] + F([0.01, -0.01, 0.005]))
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    Q, R, _ = base()

    def run(matching):
        h = _map_ctx(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if matching:
                h.desc_ref_set(R)
                assert np.all(h.desc_match(Q, k=2)["cnt"] == 2)
                h.set_desc_chunk(64, 256)
                assert np.all(h.desc_match(Q, k=8)["cnt"] == 8)
            out.append(h.match_reduce(x, mcfg))
            return out, h.map_size(), h.map_points().copy(), h.scan_get().copy()
        finally:
            h.close()

    (plain, pn, pm, ps), (matched, mn, mm, ms) = run(False), run(True)
    assert pn == mn == len(mp) and pm.tobytes() == mm.tobytes() == mp.tobytes() and ps.tobytes() == ms.tobytes() == scan.tobytes()
    for a, b in zip(plain, matched):
        assert a[2] == b[2] > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_localizer_forwards(hip):
    from fast_limo_amd import api
    Q, R, _ = base()
    hip.desc_ref_set(R)
    first = hip.desc_match(Q, k=2)
    loc = api.Localizer(api.default_cfg())
    try:
        assert loc.desc_ref_size() == 0
        assert np.all(loc.desc_match(Q, k=2)["cnt"] == 0)
        loc.desc_ref_set(R)
        assert loc.desc_ref_size() == len(R)
        same_bytes(first, loc.desc_match(Q, k=2), "Localizer with no map")
        loc.map_add(np.concatenate(sf.standard_batches()[:1]))
        size = loc.map_size()
        same_bytes(first, loc.desc_match(Q, k=2), "Localizer with a map")
        assert loc.map_size() == size and loc.desc_ref_size() == len(R)
        with pytest.raises(api.FlimoError):
            loc.desc_match(Q, k=9)
    finally:
        loc.close()


# ---- 9. the whole chain: a pose from the two clouds alone ----------------------------------------------------------------------------
# The scan's true pose: the sensor 1.2 m in front of the wall, 2 m above the floor, clear of the cylinder; metres and tens of degrees
# from identity.  The normals of both clouds face the sensor: the map's from its world position, the scan's from the body origin.
TRUE_T, TRUE_RPY = (1.2, 3.4, 2.0), (10.0, -15.0, 40.0)
# The parameters, and why.  Two planes and a cylinder give a local descriptor little to tell points apart by, and the map and the
# scan are two jitters (sigma 1 cm) of one 0.1 m grid, so a true pair is itself about 2.4 cm off.  Measured on the three seeds:
#  - FPFH k 64, normal_k 30, the largest neighbourhood there is (0.45 m): 6 % of the returned pairs are true; k 10 gives 0.5 %,
#    k 33 gives 2 % -- with those no sample of three is all true at any affordable nh.
#  - ratio 1.0 (the mutual check alone): at 0.95 and 0.9 the share of true pairs is the same (6 %, 5 %) and their number smaller
#    (71 - 75, 50 against 85 - 96): on this scene the ratio test removes true and false pairs alike.  (The ratio test itself is
#    covered on the CPU: tests/test_desc_host.py.)
#  - nh 2^20 samples, min_edge 1.5 m: a pose from three pairs 2.4 cm off is within 0.5 degrees only over a long baseline, and
#    0.06^3 of the samples are all true; what flimo_corr_poses is built for (the whole call: 0.04 s).
#  - the best 64 rows to the scan_fitness ranking, which picks the most accurate among them; max_dist 0.15 m, the gates as in
#    tests/test_gpu_corr.py.
CHAIN_FPFH = dict(k=64, normal_k=30)
RELOC = dict(ratio=1.0, mutual=True, nh=1 << 20, top=64, corr=dict(edge_sim=0.9, min_edge=1.5, max_dist=0.15), fitness_max_dist=0.5,
             align=dict(k=5, max_dist=1.0, max_curv=0.05, iters=12))


def body_scan(s):
    """The scan of seed s: the scene's surfaces under another jitter and order, cut at y < 2.9 m (the floor, the wall and the
    cylinder are nearly mirror-symmetric about y = 2: the cut breaks that), moved into the body frame of the true pose.  Returns
    (body points float32, their world points, the true x26)."""
    world = fc.scene(seed=8 + s)
    world = world[world[:, 1] < 2.9]
    x = sf.x26_of(TRUE_T, TRUE_RPY)
    Rm = sl.quat_R(x[3:7])
    body = ((world.astype(np.float64) - np.float64(TRUE_T)) @ Rm).astype(F)      # R^T (w - t), row-wise
    return np.ascontiguousarray(body), world, x


@pytest.mark.parametrize("s", [0, 1, 2])
def test_relocalize_from_descriptors(s):
    """api.relocalize with the parameters fixed above.  The pairs api.desc_pairs returns are the restatement's on the same
    descriptors, exactly; the first row after the scan_fitness ranking lies within tests/test_gpu_corr.py's first bar (0.05 m,
    0.5 degrees); scan_align ends within scan_linearize_common's POS_BAR / ROT_BAR_DEG.  The share of true pairs (the paired map
    point within 0.1 m of the scan point's true world position) is printed, not asserted: profiles/desc_match/README.md records it.

    Measured on an MI355X with the parameters above: 1 448 / 1 394 / 1 422 pairs of which 96 / 85 / 88 are true (6.6 %, 6.1 %,
    6.2 %); the first ranked row 0.013 m / 0.18 deg, 0.016 m / 0.23 deg, 0.004 m / 0.28 deg off; scan_align ends 2.3 mm / 0.053 deg,
    2.0 mm / 0.043 deg, 3.0 mm / 0.083 deg off."""
    from fast_limo_amd import api
    body, world, x_true = body_scan(s)
    map_ctx, scan_ctx = _map_ctx(fc.scene()), _map_ctx(body)
    try:
        map_ctx.scan_set(body)
        out = api.relocalize(map_ctx, scan_ctx, fpfh=dict(CHAIN_FPFH, viewpoint=TRUE_T), scan_fpfh=dict(CHAIN_FPFH, viewpoint=(0.0, 0.0, 0.0)),
                             seed=s,
                             **RELOC)
        qi, rj = out["pairs"]
        f_scan, f_map = out["fpfh"]
        wi, wj = dc.pairs(f_scan, f_map, RELOC["ratio"], RELOC["mutual"])
        true = np.linalg.norm(world[qi].astype(np.float64) - fc.scene()[rj].astype(np.float64), axis=1) < 0.1
        dt0, dr0 = cc.pose_error(out["consensus"]["x26"][0], x_true)
        dt1, dr1 = cc.pose_error(out["fitness"]["x26"][0], x_true)
        dt2, dr2 = cc.pose_error(out["x26"], x_true)
        print(f"seed {s}: {len(body)} scan points, {len(qi)} pairs, {int(true.sum())} true ({true.mean():.3f}); survivors "
              f"{out['consensus']['survivors']}, best inliers {out['consensus']['inliers'][0]}; consensus first {dt0:.4f} m {dr0:.3f} deg; "
              f"ranked first {dt1:.4f} m {dr1:.3f} deg; aligned {dt2 * 1e3:.2f} mm {dr2:.4f} deg")
        assert np.array_equal(qi, wi) and np.array_equal(rj, wj)
        assert np.array_equal(out["src"], body[qi]) and np.array_equal(out["dst"], fc.scene()[rj])
        assert dt1 <= 0.05 and dr1 <= 0.5
        assert dt2 <= sl.POS_BAR and dr2 <= sl.ROT_BAR_DEG
    finally:
        map_ctx.close()
        scan_ctx.close()
