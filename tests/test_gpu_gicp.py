"""GPU: the resident GICP model (flimo_gicp_build / _model / _info / _clear), the scan's covariances (flimo_scan_cov_set),
flimo_scan_gicp and api.gicp_align over them.

The model is compared with the same context's ``normals_range(cov)`` put through flimo_gicp_regularize_host row by row, bit for bit.
A pass is compared with the numpy restatement (tests/gicp_common.py) fed the downloaded model, the uploaded scan covariances and
``map_points()``, its neighbours found by brute force: pair_idx, valid, pair_m and all 28 sums with no tolerance, the sums in the
shape written out in numpy.  Wherever two calls must give the same result the arrays are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import gicp_common as gc
import scan_fitness_common as sf
import scan_linearize_common as sl
from common import CAPS, cfg1_scene, drive_two_scans
from test_gicp_host import EPS, GATE, K_COV, REF_END

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NOMAP, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -4, -5, -6
INF = float("inf")
NAMES = ("valid", "H", "g", "cost", "pair_idx", "pair_m")
IDENT = sf.x26_of((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))


def fresh(batches, scan=None, cell_size=0.0, downsample=True):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    ctx.map_config(cell_size=cell_size, downsample=downsample)
    for b in batches:
        ctx.map_add(b)
    if scan is not None:
        ctx.scan_set(scan)
    return ctx


def same_bytes(a, b, tag, names=NAMES):
    for name in names:
        if name in a or name in b:
            assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), f"{tag}: {name}"


def spd_rows(n, seed):
    """n regularised covariances of random shapes (what a caller uploads with scan_cov_set)."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 8, 3)) * rng.uniform(0.02, 0.5, (n, 1, 3))
    d = pts - pts.mean(1, keepdims=True)
    cov = np.stack([(d[:, :, i] * d[:, :, j]).mean(1) for i, j in gc.PAIRS], 1)
    return gc.regularize_numpy(cov, gc.PLANE, EPS)


def check_model(ctx, k=5, max_dist=INF, min_pts=3, rule=gc.PLANE, eps=EPS, tag=""):
    """Builds, and holds the model to the same context's covariances through the host's regularize.  Returns the model."""
    from fast_limo_amd import api
    n_cov = ctx.gicp_build(k, max_dist, min_pts, rule, eps)
    N = ctx.map_size()
    model, info = ctx.gicp_model(), ctx.gicp_info()
    assert model.shape == (N, 6) and info["points"] == N and info["n_cov"] == n_cov and info["stale"] == 0, tag
    assert (info["k"], info["min_pts"], info["rule"], info["eps"], info["max_dist"]) == (k, min_pts, rule, eps, np.float32(max_dist)), tag
    if N == 0:
        assert n_cov == 0
        return model
    nr = ctx.normals_range(0, N, k, max_dist, min_pts, want=("cov",))
    few = nr["cnt"] < max(3, min_pts)
    assert np.array_equal(np.isnan(nr["cov"]).any(1), few), tag
    want, has = np.full((N, 6), np.nan), np.zeros(N, bool)
    for i in np.nonzero(~few)[0]:
        has[i], want[i] = api.gicp_regularize_host(nr["cov"][i], rule, eps)
    assert np.array_equal(np.isnan(model).any(1), ~has) and np.all(np.isnan(model[~has])), f"{tag}: the NaN rows"
    assert model[has].tobytes() == want[has].tobytes(), f"{tag}: the regularised rows"
    assert n_cov == int(has.sum()), f"{tag}: n_cov {n_cov}, {int(has.sum())} rows hold a covariance"
    if has.any():
        assert np.linalg.eigvalsh(gc.sym3(model[has])).min() > 0.0, f"{tag}: positive definite"
    return model


@pytest.fixture(scope="module")
def lab(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(downsample=False)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scan_all(built):
    """4 097 scan points and one covariance each, from a context whose map is the scan (api.gicp_covs)."""
    from fast_limo_amd import api
    scan = sf.standard_scan(4097)
    ctx = fresh([scan], downsample=False)
    try:
        assert np.array_equal(ctx.map_points(), scan)
        cov = api.gicp_covs(ctx, k=K_COV, rule=gc.PLANE, eps=EPS)
        again = api.gicp_covs(ctx, scan, k=K_COV, rule=gc.PLANE, eps=EPS)
    finally:
        ctx.close()
    assert cov.shape == (4097, 6) and np.all(np.isfinite(cov)) and cov.tobytes() == again.tobytes()
    return scan, cov


@pytest.fixture(scope="module")
def hip(built, scan_all):
    """The standard scene (20 000 map points in four batches, its 1 024-point scan) with the model and the scan's covariances."""
    from fast_limo_amd import api
    scan = sf.standard_scan()
    ctx = fresh(sf.standard_batches(), scan)
    sctx = fresh([scan], downsample=False)
    try:
        scov = api.gicp_covs(sctx, k=K_COV, rule=gc.PLANE, eps=EPS)
    finally:
        sctx.close()
    ctx.gicp_build(K_COV, INF, 3, gc.PLANE, EPS)
    ctx.scan_cov_set(scov)
    ctx.scov = scov
    yield ctx
    ctx.close()


def compare(ctx, scov, poses, max_dist, tag, host_terms=0):
    """scan_gicp(want_pairs) against the restatement with brute-force neighbours, scan_fitness' nn_idx and the host term."""
    from fast_limo_amd import api
    scan, mp, model = ctx.scan_get(), ctx.map_points(), ctx.gicp_model()
    poses = np.asarray(poses).reshape(-1, 26)
    got = ctx.scan_gicp(poses, max_dist, want_pairs=True)
    per = [gc.restate(x, scan, scov, mp, model, max_dist) for x in poses]
    ref = gc.as_call(per)
    fit = ctx.scan_fitness(poses, max_dist, want_nn=True)
    assert np.array_equal(got["pair_idx"], fit[3]), f"{tag}: pair_idx against scan_fitness' nn_idx"
    assert np.array_equal(got["pair_idx"], ref["pair_idx"]), f"{tag}: pair_idx against brute force"
    assert np.array_equal(got["valid"], ref["valid"]), f"{tag}: valid {got['valid']} against {ref['valid']}"
    assert np.array_equal(np.isnan(got["pair_m"]), np.isnan(ref["pair_m"])), f"{tag}: the invalid pairs"
    same_bytes(got, ref, tag)
    for j, r in enumerate(per):
        F, A, terms = gc.fsum_sums(r["C"])
        mine = np.concatenate([got["H"][j], got["g"][j], got["cost"][j:j + 1]])
        assert np.all(np.abs(mine - F) <= sl.sum_bound(terms, A)), f"{tag}: against fsum"
        R = sf.pose_rt(poses[j])[:, :3]
        for i in np.nonzero(r["idx"] >= 0)[0][:host_terms]:
            live, m, _, sums = api.gicp_term_host(r["w"][i], mp[r["idx"][i]], scan[i], R, scov[i], model[r["idx"][i]])
            assert live == bool(r["valid"][i]) and sums.tobytes() == r["C"][i].tobytes()
            assert (m == got["pair_m"][j, i]) if live else np.isnan(got["pair_m"][j, i])
    return got


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_small_maps(lab, n):
    rng = np.random.default_rng(n)
    lab.map_clear()
    lab.map_add(rng.uniform(-2, 2, (n, 3)).astype(np.float32))
    model = check_model(lab, k=5, tag=f"{n} points")
    assert np.isnan(model).all() == (n < 3)
    if n == 257:
        lab.set_normals_chunk(100)      # three chunks
        try:
            assert check_model(lab, k=5, tag="chunked").tobytes() == model.tobytes()
        finally:
            lab.set_normals_chunk(0)
        for rule, eps in ((gc.CLAMP, 0.01), (gc.PLANE, 1.0), (gc.CLAMP, 1.0)):
            other = check_model(lab, k=8, max_dist=1.5, min_pts=5, rule=rule, eps=eps, tag=f"rule {rule} eps {eps}")
            assert other.tobytes() != model.tobytes()


def test_duplicates_coplanar_and_collinear_neighbourhoods_and_a_map_ten_kilometres_away(lab):
    lab.map_clear()
    lab.map_add(np.concatenate([np.tile(np.float32([[1, 2, 3]]), (300, 1)), np.float32([[1.5, 2, 3]])]))
    model = check_model(lab, k=20, tag="300 duplicates and one point")
    assert np.isnan(model[:300]).all(), "twenty copies of one point have no covariance"
    g = np.arange(8, dtype=np.float32) * 0.25
    plane = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    lab.map_clear()
    lab.map_add(np.concatenate([np.c_[plane, np.zeros(len(plane), np.float32)], np.c_[np.zeros((16, 2), np.float32) + 50, 50 + np.arange(16) * 0.25]]).astype(np.float32))
    model = check_model(lab, k=6, max_dist=1.0, tag="a plane and a line")
    assert np.all(np.isfinite(model)) and np.all(model[:64, 5] == EPS) and np.all(model[:64, [2, 4]] == 0.0), "eps across the plane z = 0"
    clamp = check_model(lab, k=6, max_dist=1.0, rule=gc.CLAMP, eps=0.01, tag="the same, clamped")
    assert np.all(clamp[:64, 5] > 0.0) and np.all(clamp[64:, 0] > 0.0) and np.all(clamp[64:, 0] == clamp[64:, 3])
    rng = np.random.default_rng(4)
    lab.map_clear()
    lab.map_add((rng.uniform(-3, 3, (500, 3)) + 10000.0).astype(np.float32))
    far = check_model(lab, k=10, tag="ten kilometres away")
    assert np.all(np.isfinite(far))
    lab.map_clear()
    assert check_model(lab, tag="an empty map").shape == (0, 6)


def test_batches_and_index_cell_sizes_move_no_byte(hip):
    model = check_model(hip, k=K_COV, tag="the standard scene")
    mp = hip.map_points().copy()
    for tag, batches, cell in (("one batch", [mp], 0.0), ("five batches", np.array_split(mp, 5), 0.0), ("cells of 0.25 m", [mp], 0.25),
                               ("cells of 1 m", [mp], 1.0)):
        ctx = fresh(batches, cell_size=cell, downsample=False)
        try:
            assert np.array_equal(ctx.map_points(), mp)
            ctx.gicp_build(K_COV, INF, 3, gc.PLANE, EPS)
            assert ctx.gicp_model().tobytes() == model.tobytes(), tag
            assert ctx.gicp_model(7, 5).tobytes() == model[7:12].tobytes()
        finally:
            ctx.close()


# ---- 2. the pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097])
def test_a_pass_against_the_restatement(hip, scan_all, n):
    scan, cov = scan_all[0][:n], scan_all[1][:n]
    ctx = fresh([hip.map_points().copy()], scan, downsample=False)
    try:
        ctx.gicp_build(K_COV, INF, 3, gc.PLANE, EPS)
        ctx.scan_cov_set(cov)
        assert ctx.scan_cov_size() == n
        got = compare(ctx, cov, sl.start_poses(((0.2, -0.1, 2),)), GATE, f"{n} points", host_terms=40)
        assert n < 255 or got["valid"][0] > 0.5 * n
    finally:
        ctx.close()


def test_poses_their_order_chunks_outputs_and_the_walk_over_the_tiles(hip):
    n = hip.scan_size()
    poses = np.stack([sf.displaced(), sf.displaced(dx=0.5, dyaw_deg=5), sf.displaced(dx=60.0), sf.displaced(dy=-1, dyaw_deg=-10), sf.displaced(dx=0.05)])
    one = compare(hip, hip.scov, poses, GATE, "five poses")
    assert one["valid"][2] == 0 and np.all(one["pair_idx"][2] == -1) and one["valid"][0] > 900
    back = hip.scan_gicp(poses[::-1], GATE, want_pairs=True)
    same_bytes({k: v[::-1].copy() for k, v in back.items()}, one, "pose order reversed")
    for j in range(5):
        same_bytes({k: v[j:j + 1].copy() for k, v in one.items()}, hip.scan_gicp(poses[j:j + 1], GATE, want_pairs=True), f"pose {j} alone")
    for pairs in (n, 3 * n):
        hip.set_gicp_chunk(pairs)
        try:
            same_bytes(hip.scan_gicp(poses, GATE, want_pairs=True), one, f"chunks of {pairs // n} poses")
        finally:
            hip.set_gicp_chunk(0)
    # every combination of the optional outputs
    x = np.ascontiguousarray(poses)
    for want_idx in (False, True):
        for want_m in (False, True):
            out = dict(valid=np.zeros(5, np.int32), H=np.zeros((5, 21)), g=np.zeros((5, 6)), cost=np.zeros(5), pair_idx=np.zeros((5, n), np.int32),
                       pair_m=np.zeros((5, n)))
            rc = hip._L.flimo_scan_gicp(hip._h, x.ctypes.data, 5, GATE, *(out[k].ctypes.data for k in NAMES[:4]),
                                        out["pair_idx"].ctypes.data if want_idx else None, out["pair_m"].ctypes.data if want_m else None)
            assert rc == 0
            same_bytes(out, one, f"outputs {want_idx} {want_m}", NAMES[:4] + (("pair_idx",) if want_idx else ()) + (("pair_m",) if want_m else ()))
    same_bytes(hip.scan_gicp(poses, GATE), one, "without the pairs", NAMES[:4])
    # the walk over the tiles: the scan thrown 60 m from the map, no gate
    far = compare(hip, hip.scov, poses[2:3], INF, "no gate, 60 m away")
    assert np.all(far["pair_idx"] >= 0) and far["valid"][0] > 0.9 * n
    # a gate that admits no pair
    none = compare(hip, hip.scov, poses[:1], 1e-6, "a gate of a micrometre")
    assert none["valid"][0] == 0 and not none["H"].any() and np.isnan(none["pair_m"]).all()
    zero = hip.scan_gicp(poses[:2], 0.0, want_pairs=True)
    assert not zero["valid"].any() and not zero["H"].any() and not zero["g"].any() and not zero["cost"].any()
    assert np.all(zero["pair_idx"] == -1) and np.isnan(zero["pair_m"]).all()
    x = poses.copy()
    x[:, 7:] = np.nan      # only pos and rot of a pose are read
    same_bytes(hip.scan_gicp(x, GATE, want_pairs=True), one, "the rest of a pose")


def test_nan_rows_nan_points_ties_and_a_gate_for_one_pair(lab):
    rng = np.random.default_rng(9)
    cluster = rng.uniform(0, 3, (300, 3)).astype(np.float32)
    lone, tie = np.float32([[50, 50, 50]]), np.float32([[10, 10, 10.5], [10, 10, 9.5]])
    lab.map_clear()
    lab.map_add(np.concatenate([cluster, lone, tie]))
    model = check_model(lab, k=5, max_dist=1.0, tag="the lab map")
    assert np.isfinite(model[:300]).all(1).sum() > 290 and np.isnan(model[300:]).all(), "the lone point and the tie pair have no covariance"
    near = (cluster[:40] + rng.normal(0, 0.02, (40, 3))).astype(np.float32)
    scan = np.concatenate([near, np.float32([[50, 50, 50.125], [10, 10, 10], [np.nan, 0, 0], [-100, 0, 0]])])
    scov = spd_rows(len(scan), 2)
    scov[7] = np.nan
    scov[11, 3] = np.nan
    lab.scan_set(scan)
    assert lab.scan_cov_size() == 0
    lab.scan_cov_set(scov)
    got = compare(lab, scov, IDENT[None], 1.0, "the lab scan", host_terms=44)
    idx, m = got["pair_idx"][0], got["pair_m"][0]
    assert idx[40] == 300 and np.isnan(m[40]), "a neighbour whose model row is NaN: the neighbour is reported, the pair is invalid"
    assert idx[41] == 301 and np.isnan(m[41]), "two stored points equally far: the lower index"
    assert idx[42] == -1 and idx[43] == -1 and np.isnan(m[42:]).all(), "a NaN scan point and a point beyond the gate"
    assert idx[7] >= 0 and idx[11] >= 0 and np.isnan(m[7]) and np.isnan(m[11]), "a scan point whose covariance row has a NaN"
    assert got["valid"][0] == int(np.isfinite(m).sum()) >= 30
    # a gate that admits exactly one pair: scan point 0 put 2^-6 m from stored point 0, every other one far from the map; gate 2^-5 m
    scan2 = scan.copy()
    scan2[:40] = np.float32([-100, 0, 0]) - np.arange(40, dtype=np.float32)[:, None] * np.float32([1, 0, 0])
    scan2[0] = cluster[0] + np.float32([2.0 ** -6, 0, 0])
    lab.scan_set(scan2)
    lab.scan_cov_set(scov)
    only = compare(lab, scov, IDENT[None], 2.0 ** -5, "a gate for one pair", host_terms=1)
    has = only["pair_idx"][0] >= 0
    assert has.sum() == 1 and has[0]
    assert only["valid"][0] == int(np.isfinite(model[only["pair_idx"][0][0]]).all())


# ---- 3. the lifecycle -------------------------------------------------------------------------------------------------------------
def raw_pass(ctx, poses, max_dist=GATE):
    x = np.ascontiguousarray(poses, np.float64).reshape(-1, 26)
    m = len(x)
    out = dict(valid=np.full(m, -7, np.int32), H=np.full((m, 21), -7.0), g=np.full((m, 6), -7.0), cost=np.full(m, -7.0))
    rc = ctx._L.flimo_scan_gicp(ctx._h, x.ctypes.data, m, max_dist, *(out[k].ctypes.data for k in NAMES[:4]), None, None)
    return rc, out, ctx._L.flimo_last_error(ctx._h).decode()


def test_the_lifecycle_of_the_model_and_of_the_scans_covariances(scan_all):
    batches = sf.standard_batches()
    scan, cov = scan_all[0][:512], scan_all[1][:512]
    poses = sf.standard_poses()[[sf.TRUE_POSE, 30]]
    ctx = fresh(batches[:3], scan)
    try:
        rc, out, msg = raw_pass(ctx, poses)
        assert rc == ERR_NOMAP and "flimo_gicp_build" in msg and np.all(out["valid"] == -7)
        with pytest.raises(Exception, match="no map"):
            ctx.gicp_info()
        with pytest.raises(Exception, match="no map"):
            ctx.gicp_model(0, 0)
        n_cov = ctx.gicp_build(10, INF, 3, gc.PLANE, EPS)
        assert n_cov == ctx.map_size()
        rc, out, msg = raw_pass(ctx, poses)
        assert rc == ERR_NOMAP and "flimo_scan_cov_set" in msg and np.all(out["cost"] == -7)
        for bad in (cov[:511], np.concatenate([cov, cov[:1]])):
            assert ctx._L.flimo_scan_cov_set(ctx._h, np.ascontiguousarray(bad).ctypes.data, len(bad)) == ERR_INVALID
        assert ctx.scan_cov_size() == 0
        ctx.scan_cov_set(cov)
        assert ctx.scan_cov_size() == 512
        first = ctx.scan_gicp(poses, GATE, want_pairs=True)
        assert raw_pass(ctx, poses)[0] == 0 and first["valid"][0] > 400
        # the stored points change: the model is stale until it is rebuilt
        ctx.map_add(batches[3])
        rc, out, msg = raw_pass(ctx, poses)
        assert rc == ERR_NOMAP and "stale" in msg and np.all(out["H"] == -7) and ctx.gicp_info()["stale"] == 1
        assert ctx.gicp_info()["points"] < ctx.map_size() and ctx.gicp_model().shape[0] == ctx.gicp_info()["points"]
        ctx.gicp_build(10, INF, 3, gc.PLANE, EPS)
        assert raw_pass(ctx, poses)[0] == 0 and ctx.gicp_info()["stale"] == 0
        assert ctx.map_crop_box(np.float32([-30, -4, -5]), np.float32([6, 30, 30])) > 500
        rc, _, msg = raw_pass(ctx, poses)
        assert rc == ERR_NOMAP and "stale" in msg
        ctx.gicp_build(10, INF, 3, gc.PLANE, EPS)
        plane = ctx.gicp_model()
        assert raw_pass(ctx, poses)[0] == 0
        # a failed build leaves the old model intact; a rebuild with another rule replaces it
        keep = C.c_size_t(77)
        from fast_limo_amd import _abi
        assert ctx._L.flimo_gicp_build(ctx._h, C.byref(_abi.GicpCfg(2, INF, 3, gc.PLANE, EPS)), C.byref(keep)) == ERR_UNSUPPORTED
        assert keep.value == 77 and ctx.gicp_model().tobytes() == plane.tobytes() and ctx.gicp_info()["rule"] == gc.PLANE
        ctx.gicp_build(10, INF, 3, gc.CLAMP, 0.01)
        assert ctx.gicp_info()["rule"] == gc.CLAMP and ctx.gicp_model().tobytes() != plane.tobytes()
        # a new scan drops the covariances; a pending change of the map does not bring them back
        ctx.scan_set(scan[:300])
        assert ctx.scan_cov_size() == 0
        rc, _, msg = raw_pass(ctx, poses)
        assert rc == ERR_NOMAP and "flimo_scan_cov_set" in msg
        ctx.scan_cov_set(cov[:300])
        assert raw_pass(ctx, poses)[0] == 0
        ctx.scan_cov_set(None)
        assert ctx.scan_cov_size() == 0 and raw_pass(ctx, poses)[0] == ERR_NOMAP
        ctx.scan_cov_set(cov[:300])
        # map_clear: stale; a model of the empty map: every pass is empty
        ctx.map_clear()
        rc, _, msg = raw_pass(ctx, poses)
        assert rc == ERR_NOMAP and "stale" in msg
        assert ctx.gicp_build(10, INF, 3, gc.PLANE, EPS) == 0 and ctx.gicp_info()["points"] == 0
        rc, out, _ = raw_pass(ctx, poses)
        assert rc == 0 and not out["valid"].any() and not out["H"].any() and not out["g"].any() and not out["cost"].any()
        ctx.gicp_clear()
        assert raw_pass(ctx, poses)[0] == ERR_NOMAP
        with pytest.raises(Exception, match="no map"):
            ctx.gicp_info()
    finally:
        ctx.close()


# ---- 4. no side effects -------------------------------------------------------------------------------------------------------------
def test_the_calls_leave_map_scan_knn_an_ndt_model_and_the_passes_alone(scan_all):
    from fast_limo_amd import _lib
    cfg = _lib.default_match_cfg(**CAPS)
    poses = sf.standard_poses()[[sf.TRUE_POSE, 30, 99]]
    scan, cov = sf.standard_scan(), scan_all[1][:sf.N_SCAN]
    q = np.ascontiguousarray(scan_all[0][:200])

    def run(call):
        ctx = fresh(sf.standard_batches()[:3], scan)
        try:
            gicp = []
            if call:
                ctx.gicp_build(10, INF, 3, gc.PLANE, EPS)
                ctx.scan_cov_set(cov)
                gicp.append(ctx.scan_gicp(poses, GATE, want_pairs=True))
            passes = [ctx.match_reduce(poses[0], cfg)]
            ctx.ndt_build(0, 1.0, 6, 0.01)
            if call:
                gicp.append(ctx.scan_gicp(poses, GATE, want_pairs=True))
                ctx.gicp_model()
            passes.append(ctx.match_reduce(poses[0], cfg))
            knn = ctx.knn_k(q, 8)
            lin = ctx.scan_linearize(poses, 5, 1.0)
            if call:
                ctx.gicp_build(10, INF, 3, gc.CLAMP, 0.01)
                gicp.append(ctx.scan_gicp(poses, GATE))
                ctx.gicp_clear()
            passes.append(ctx.match_reduce(poses[0], cfg))
            ndt = ctx.scan_ndt(0, poses, 1.0)
            return gicp, passes, knn, lin, ndt, ctx.ndt_cells(0), ctx.map_points().copy(), ctx.scan_get().copy()
        finally:
            ctx.close()
    a, b = run(True), run(False)
    same_bytes(a[0][0], a[0][1], "two passes of one model")
    assert a[0][0]["valid"][0] > 500 and b[0] == []
    for j, (x, y) in enumerate(zip(a[1], b[1])):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2], f"pass {j}"
    for x, y in zip(a[2], b[2]):
        assert x.tobytes() == y.tobytes(), "knn_k"
    same_bytes(a[3], b[3], "scan_linearize", ("valid", "H", "g", "cost"))
    same_bytes(a[4], b[4], "scan_ndt", ("valid", "cells", "H", "g", "score"))
    same_bytes(a[5], b[5], "the NDT model", ("ijk", "count", "mean", "evec", "wgt", "eval"))
    assert a[6].tobytes() == b[6].tobytes() and a[7].tobytes() == b[7].tobytes()


# ---- 5. the rejected arguments ------------------------------------------------------------------------------------------------------
def test_every_rejected_argument_leaves_the_outputs_untouched(hip):
    from fast_limo_amd import _abi
    n = hip.scan_size()
    good = np.ascontiguousarray(sf.standard_poses()[:3])
    out = dict(valid=np.full(3, -7, np.int32), H=np.full((3, 21), -7.0), g=np.full((3, 6), -7.0), cost=np.full(3, -7.0),
               pair_idx=np.full((3, n), -7, np.int32), pair_m=np.full((3, n), -7.0))
    p = {k: a.ctypes.data for k, a in out.items()}

    def raw(x=good, m=3, max_dist=GATE, h=hip._h, **null):
        q = dict(p, **{name: None for name in null})
        return hip._L.flimo_scan_gicp(h, None if x is None else x.ctypes.data, m, max_dist, *(q[k] for k in NAMES))
    assert raw(h=None) == ERR_INVALID and raw(x=None) == ERR_INVALID
    for name in NAMES[:4]:
        assert raw(**{name: True}) == ERR_INVALID, name
    for gate in (np.nan, -1.0, -np.inf):
        assert raw(max_dist=gate) == ERR_INVALID, gate
    x = good.copy()
    x[2, 5] = np.nan
    assert raw(x=x) == ERR_INVALID and raw(m=2 ** 31) == ERR_TOO_LARGE
    x[2, 5] = np.inf
    assert raw(x=x) == ERR_INVALID
    assert raw(m=0) == 0 and raw(x=None, m=0) == 0      # np == 0 touches nothing
    for a in out.values():
        assert np.all(a == -7)
    # the build's rejections leave *n_cov and the model alone
    model = hip.gicp_model()
    keep = C.c_size_t(77)
    for k, gate, mp, rule, eps, code in ((2, INF, 3, 0, EPS, ERR_UNSUPPORTED), (65, INF, 3, 0, EPS, ERR_UNSUPPORTED), (0, INF, 3, 0, EPS, ERR_UNSUPPORTED),
                                         (10, np.nan, 3, 0, EPS, ERR_INVALID), (10, -1.0, 3, 0, EPS, ERR_INVALID), (10, INF, -1, 0, EPS, ERR_INVALID),
                                         (10, INF, 3, 2, EPS, ERR_INVALID), (10, INF, 3, -1, EPS, ERR_INVALID), (10, INF, 3, 0, 0.0, ERR_INVALID),
                                         (10, INF, 3, 1, 1.5, ERR_INVALID), (10, INF, 3, 0, np.nan, ERR_INVALID), (10, INF, 3, 1, -0.5, ERR_INVALID)):
        cfg = _abi.GicpCfg(k, gate, mp, rule, eps)
        assert hip._L.flimo_gicp_build(hip._h, C.byref(cfg), C.byref(keep)) == code, (k, gate, mp, rule, eps)
    assert hip._L.flimo_gicp_build(hip._h, None, C.byref(keep)) == ERR_INVALID and keep.value == 77
    assert hip.gicp_model().tobytes() == model.tobytes() and hip.gicp_info()["stale"] == 0
    buf = np.full((4, 6), -7.0)
    N = hip.map_size()
    for first, cnt in ((N, 1), (N + 1, 0), (0, N + 1), (N - 1, 2)):
        assert hip._L.flimo_gicp_model(hip._h, first, cnt, buf.ctypes.data) == ERR_INVALID, (first, cnt)
    assert hip._L.flimo_gicp_model(hip._h, 0, 2, None) == ERR_INVALID and np.all(buf == -7)
    assert hip._L.flimo_gicp_info(hip._h, None) == ERR_INVALID
    assert hip._L.flimo_scan_cov_set(hip._h, hip.scov.ctypes.data, n - 1) == ERR_INVALID and hip.scan_cov_size() == n
    assert raw() == 0 and np.all(out["valid"] >= 0) and np.all(out["pair_idx"] >= -1)


# ---- 6. the alignment ---------------------------------------------------------------------------------------------------------------
def test_gicp_align_follows_the_restatement_bit_for_bit(hip):
    """Two starts, four steps: the restatement with brute-force neighbours gives the sums of every step byte for byte, so the
    host's solve sees the same bytes and the poses stay equal."""
    from fast_limo_amd import api
    start = sl.start_poses(((0.5, 0, 0), (-1, 1, -10)))
    lin = gc.linearizer(hip.scan_get(), hip.scov, hip.map_points(), hip.gicp_model(), GATE)
    got = api.gicp_align(hip, start, max_dist=GATE, iters=4)
    ref = api.scan_align(None, start, iters=4, linearize=lin)
    for name in ("x26", "valid", "cost", "iters", "status"):
        assert got[name].tobytes() == ref[name].tobytes(), name
    assert np.all(got["iters"] == 4)


def test_gicp_align_ends_where_the_restatement_ends(hip):
    """All nine starts, api.gicp_align's ten steps.  The restatement runs on the device's neighbours (scan_fitness' nn_idx, which
    test 2 pins to brute force) and so on the device's sums: the poses are equal byte for byte.  The end is held to twice the
    restatement's own recorded end on numpy's covariances (test_gicp_host.REF_END): the device's covariances are the same
    neighbourhoods' by another summation, which moves the minimum by rounding alone."""
    from fast_limo_amd import api
    start = sl.start_poses(sl.STARTS)
    lin = gc.linearizer(hip.scan_get(), hip.scov, hip.map_points(), hip.gicp_model(), GATE,
                        neighbours=lambda xs: hip.scan_fitness(xs, GATE, want_nn=True)[3])
    got = api.gicp_align(hip, start, max_dist=GATE)
    ref = api.scan_align(None, start, linearize=lin)
    for name in ("x26", "valid", "cost", "iters", "status"):
        assert got[name].tobytes() == ref[name].tobytes(), name
    errs = [sl.pose_error(x) for x in got["x26"]]
    for s, (dp, dr), it, v in zip(sl.STARTS, errs, got["iters"], got["valid"]):
        print(f"gicp_align start {s}: iterations {it}, valid {v}; {dp * 1e3:.3f} mm, {dr:.5f} deg")
    assert np.all(got["status"] == api.ALIGN_RUNNING) and np.all(got["iters"] == 10)
    for s, (dp, dr) in zip(sl.STARTS, errs):
        assert dp <= 2 * REF_END[0] and dr <= 2 * REF_END[1], (s, dp, dr)


def test_through_the_localizer(built):
    from fast_limo_amd import api
    mp, scan, imu = cfg1_scene()
    poses = np.stack([sf.displaced(), sf.displaced(dx=0.2), sf.displaced(dx=60.0)])
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        with pytest.raises(Exception, match="flimo_loc_scan_gicp failed \\(-4\\)"):
            loc.scan_gicp(poses)
        loc.set_async_insert(True)
        assert drive_two_scans(loc, mp, scan, imu)[1] == 0
        n_cov = loc.gicp_build(10, INF, 3, gc.PLANE, EPS)      # (an insert may still be running: the call waits)
        pc = loc.pc2match().copy()
        sctx = fresh([pc], downsample=False)
        try:
            cov = api.gicp_covs(sctx, k=10, rule=gc.PLANE, eps=EPS)
        finally:
            sctx.close()
        assert loc.scan_cov_size() == 0
        loc.scan_cov_set(cov)
        assert loc.scan_cov_size() == len(pc)
        found = loc.scan_gicp(poses, GATE, want_pairs=True)
        loc.sync()
        ctx = fresh([loc.hip.map_points().copy()], pc, downsample=False)
        try:
            assert np.array_equal(ctx.map_points(), loc.hip.map_points())
            assert ctx.gicp_build(10, INF, 3, gc.PLANE, EPS) == n_cov == loc.gicp_info()["n_cov"] > 50
            assert ctx.gicp_model().tobytes() == loc.gicp_model().tobytes() and ctx.gicp_info() == loc.gicp_info()
            ctx.scan_cov_set(cov)
            same_bytes(found, ctx.scan_gicp(poses, GATE, want_pairs=True), "Localizer against HipCtx")
            assert found["valid"][2] == 0 and found["valid"][0] > 100
            a, b = api.gicp_align(loc, poses[:2], iters=3), api.gicp_align(ctx, poses[:2], iters=3)
            assert a["x26"].tobytes() == b["x26"].tobytes()
        finally:
            ctx.close()
        loc.gicp_clear()
        with pytest.raises(Exception, match="flimo_loc_gicp_info failed \\(-4\\)"):
            loc.gicp_info()
    finally:
        loc.close()
