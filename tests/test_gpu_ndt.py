"""GPU: the resident NDT cell models (flimo_ndt_build / _cells / _info / _clear), flimo_scan_ndt and api.ndt_align over them.

The model is compared with the same context's ``map_voxels`` -- ijk, count and mean bit for bit; the eigen-solve against numpy eigh
of that cov by normals_common's U_EIG bounds; wgt exactly from the device's own eval.  The terms are compared with the numpy
restatement (tests/ndt_common.py) fed with the same context's downloaded model: term_cell and m with no tolerance, e within
ndt_common.EXP_ULPS spacings of np.exp(x), and valid, cells and all 28 sums bit for bit given the device's own e, summed in the
shape written out in numpy.  Wherever two calls must give the same result the arrays are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import ndt_common as nd
import normals_common as nc
import scan_fitness_common as sf
import scan_linearize_common as sl
import voxels_common as vc
from common import CAPS, cfg1_scene, drive_two_scans
from test_ndt_host import EIG_RATIO, KEPT, LEAVES, MIN_PTS, OUTLIER, REF_END, WIDE

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NOMAP, ERR_TOO_LARGE = -2, -4, -5
NAMES = ("valid", "cells", "H", "g", "score", "terms", "term_cell")


def fresh(batches, scan=None, cell_size=0.0, downsample=True):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device
    ctx.map_config(cell_size=cell_size, downsample=downsample)
    for b in batches:
        ctx.map_add(b)
    if scan is not None:
        ctx.scan_set(scan)
    return ctx


def model_of(ctx, slot):
    m = ctx.ndt_cells(slot)
    m["leaf"] = ctx.ndt_info(slot)["leaf"]
    return m


def d2_of(leaf):
    from fast_limo_amd import api
    return api.ndt_params(OUTLIER, leaf)[1]


def same_bytes(a, b, tag, names=NAMES):
    for name in names:
        if name in a or name in b:
            assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), f"{tag}: {name}"


def check_model(ctx, slot, leaf, min_pts=MIN_PTS, eig_ratio=EIG_RATIO, tag=""):
    """The model of `slot` against the same context's voxels: the exact parts, the eigen bounds, the exact weights.  Returns it."""
    vox = ctx.map_voxels(want=("ijk", "count", "centroid", "cov"), leaf=leaf)
    rows = nd.cell_rows(vox, min_pts)
    m = model_of(ctx, slot)
    info = ctx.ndt_info(slot)
    assert m["nc"] == len(rows) == info["cells"], f"{tag}: {m['nc']} cells, the rule gives {len(rows)}"
    assert info["leaf"] == np.float32(leaf) and info["min_pts"] == min_pts and info["eig_ratio"] == eig_ratio
    assert np.array_equal(m["ijk"], vox["ijk"][rows]) and np.array_equal(m["count"], vox["count"][rows]), tag
    assert m["mean"].tobytes() == vox["centroid"][rows].tobytes(), f"{tag}: mean"
    keys = nd.key_of(m["ijk"])
    assert np.all(keys[1:] > keys[:-1]), f"{tag}: the cells are listed in ascending key"
    assert m["wgt"].tobytes() == nd.weights(m["eval"], eig_ratio).tobytes(), f"{tag}: wgt from the device's own eval"
    worst = np.zeros(4)
    for t, v in enumerate(rows):
        Cm = nd.sym3(vox["cov"][v])
        fro = np.linalg.norm(Cm)
        l, V = m["eval"][t], m["evec"][t]
        assert l[0] <= l[1] <= l[2] and l[2] > 0.0
        ev = np.abs(l - np.linalg.eigvalsh(Cm)).max()
        res = max(np.linalg.norm(Cm @ V[k] - l[k] * V[k]) for k in range(3))
        unit = max(abs(np.linalg.norm(V[k]) - 1.0) for k in range(3))
        assert ev <= nc.U_EIG * fro and res <= nc.U_EIG * fro and unit <= nc.U_EIG, (tag, t, ev, res, unit, fro)
        orth = max(abs(V[0] @ V[1]), abs(V[0] @ V[2]), abs(V[1] @ V[2]))
        worst = np.maximum(worst, [ev / fro, res / fro, unit, orth])
    m["worst"] = worst
    m["cov"] = vox["cov"][rows]
    return m


@pytest.fixture(scope="module")
def hip(built):
    """The standard scene (20 000 map points in four batches, a 1024-point scan) with the models of leaf 2.0 / 1.0 / 0.5 / 0.25 in slots
    0..3."""
    ctx = fresh(sf.standard_batches(), sf.standard_scan())
    for slot, leaf in enumerate(LEAVES + (0.25,)):
        ctx.ndt_build(slot, leaf, MIN_PTS, EIG_RATIO)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def models(hip):
    return [model_of(hip, slot) for slot in range(3)]


@pytest.fixture(scope="module")
def lab(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(downsample=False)
    yield ctx
    ctx.close()


def compare(ctx, model, slot, poses, hood, d2, tag, plain=False):
    """scan_ndt(want_terms) against the restatement; returns the call's dict."""
    scan = ctx.scan_get()
    n = scan.shape[0]
    got = ctx.scan_ndt(slot, poses, d2, hood=hood, want_terms=True)
    assert got["terms"].shape == (len(poses), n, 7, 2) and got["cells"].dtype == np.int64
    for j, x in enumerate(poses):
        r = nd.restate(x, scan, model, hood, d2, e=got["terms"][j, :, :, 1])
        assert np.array_equal(got["term_cell"][j], r["cell"]), f"{tag}: term_cell of pose {j}"
        have = r["cell"] >= 0
        assert np.array_equal(np.isnan(got["terms"][j, :, :, 0]), ~have) and np.array_equal(np.isnan(got["terms"][j, :, :, 1]), ~have)
        assert got["terms"][j, :, :, 0][have].tobytes() == r["m"][have].tobytes(), f"{tag}: m of pose {j}"
        with np.errstate(under="ignore", over="ignore"):
            ref_e = np.exp(r["x"][have])
        assert np.all(np.abs(got["terms"][j, :, :, 1][have] - ref_e) <= nd.EXP_ULPS * np.spacing(ref_e)), f"{tag}: e of pose {j}"
        assert (got["valid"][j], got["cells"][j]) == (r["valid"], r["cells"]), f"{tag}: counts of pose {j}"
        S = nd.shape_sums(r["C"])
        mine = np.concatenate([got["H"][j], got["g"][j], got["score"][j:j + 1]])
        assert mine.tobytes() == S.tobytes(), f"{tag}: the 28 sums of pose {j} (worst {np.abs(mine - S).max()})"
        if plain:
            assert nd.shape_sums_plain(r["C"]).tobytes() == mine.tobytes(), f"{tag}: plain floats"
        F, A, terms = nd.fsum_sums(r["C"])
        assert np.all(np.abs(mine - F) <= sl.sum_bound(terms, A)), f"{tag}: against fsum"
        Hm = np.zeros((6, 6))
        Hm[np.triu_indices(6)] = got["H"][j]
        Hm = Hm + np.triu(Hm, 1).T
        assert np.linalg.eigvalsh(Hm).min() >= -sl.sum_bound(terms, A[:21].max()), f"{tag}: H is positive semidefinite"
    return got


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------
def test_the_models_of_the_scene_are_the_voxels_that_pass_the_rule(hip):
    """Orthogonality |v_i . v_j| is not among U_EIG's derived quantities.  Its bar is four times numpy eigh's own worst
    orthogonality error on the leaf-1.0 cells' covariances, the dot products taken in mpmath at 50 digits.  Measured on an MI355X
    over the scene's 551 cells: numpy eigh 7.58e-16, so the bar is 3.03e-15; the device's vectors 2.88e-16 (profiles/ndt/README.md)."""
    import mpmath
    mpmath.mp.dps = 50
    worst = np.zeros(4)
    for slot, leaf in enumerate(LEAVES + (0.25,)):
        m = check_model(hip, slot, leaf, tag=f"leaf {leaf}")
        worst = np.maximum(worst, m["worst"])
        assert m["nc"] > 50
        if leaf == 1.0:
            eigh = 0.0
            for Cv in m["cov"]:
                V = np.linalg.eigh(nd.sym3(Cv))[1].T
                rows = [[mpmath.mpf(float(c)) for c in V[k]] for k in range(3)]
                eigh = max(eigh, *[float(abs(mpmath.fdot(rows[a], rows[b]))) for a, b in ((0, 1), (0, 2), (1, 2))])
            print(f"orthogonality: device {m['worst'][3]:.3e}, numpy eigh {eigh:.3e}, bar {4 * eigh:.3e}")
            assert m["worst"][3] <= 4 * eigh
    print("worst eigenvalue / residual (of ||C||_F), unit norm, orthogonality:", worst.tolist(), "U_EIG", nc.U_EIG)


def hand_points(rng):
    """Voxels of leaf 1.0 made by hand: [0] 5 points (min_pts - 1), [1] 6 points, [2] a coplanar 8, [3] a collinear 7, [4] 9
    duplicates, [5] 300 duplicates and one more point."""
    def box(c, n):
        return np.float32(c) + rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32)
    flat = box((4, 0, 0), 8)
    flat[:, 2] = 0.5
    line = np.float32((6, 0, 0)) + np.outer(np.arange(1, 8) / 8.0, (1, 0.5, 0.25)).astype(np.float32)
    return [box((0, 0, 0), 5), box((2, 0, 0), 6), flat, line, np.tile(np.float32((8.5, 0.5, 0.5)), (9, 1)),
            np.concatenate([np.tile(np.float32((10.25, 0.5, 0.5)), (300, 1)), np.float32([[10.75, 0.25, 0.5]])])]


def test_hand_made_cells_counts_degenerate_shapes_and_the_clamp(lab):
    rng = np.random.default_rng(3)
    parts = hand_points(rng)
    lab.map_clear()
    lab.map_add(np.concatenate(parts))
    assert lab.ndt_build(0, 1.0, MIN_PTS, EIG_RATIO) == 4
    m = check_model(lab, 0, 1.0, tag="hand")
    assert [int(c) for c in m["ijk"][:, 0]] == [2, 4, 6, 10] and list(m["count"]) == [6, 8, 7, 301]
    flat, line, dup = m["eval"][1], m["eval"][2], m["eval"][3]
    assert flat[0] == 0.0 and flat[1] > 0 and m["wgt"][1][0] == 1.0 / (EIG_RATIO * flat[2])
    # (the line's points are dyadic, so its cov is a rank-one matrix up to the rounding of six divisions: two eigenvalues within the
    #  eigenvalue bound of 0, either sign, and both below the floor)
    zero = 2 * nc.U_EIG * np.linalg.norm(nd.sym3(m["cov"][2]))
    assert abs(line[0]) <= zero and abs(line[1]) <= zero and m["wgt"][2][0] == m["wgt"][2][1] == 1.0 / (EIG_RATIO * line[2])
    assert dup[2] > 0 and dup[0] == 0.0
    assert lab.ndt_build(1, 1.0, MIN_PTS, 1.0) == 4      # eig_ratio = 1: every weight is 1 / l2
    one = check_model(lab, 1, 1.0, eig_ratio=1.0, tag="eig_ratio 1")
    assert np.all(one["wgt"] == (1.0 / one["eval"][:, 2])[:, None])
    assert lab.ndt_build(2, 1.0, 5, EIG_RATIO) == 5 and lab.ndt_build(3, 1.0, 400, EIG_RATIO) == 0
    check_model(lab, 2, 1.0, min_pts=5, tag="min_pts 5")
    assert lab.ndt_cells(3)["nc"] == 0 and lab.ndt_cells(3)["evec"].shape == (0, 3, 3)
    lab.ndt_clear()


@pytest.mark.parametrize("n", [1, 2, 6, 63, 64, 65, 257])
def test_small_maps_and_a_map_ten_kilometres_away(lab, n):
    rng = np.random.default_rng(n)
    pts = rng.uniform(0.0, 1.5, (n, 3)).astype(np.float32)
    for shift, leaf in ((0.0, 0.5), (10000.0, 2.0)):
        lab.map_clear()
        lab.map_add(pts + np.float32(shift))
        lab.ndt_build(0, leaf, 3, EIG_RATIO)
        check_model(lab, 0, leaf, min_pts=3, tag=f"{n} points at {shift}")
    lab.map_clear()
    assert lab.ndt_info(0)["stale"] == 1 and lab.ndt_build(1, 1.0) == 0 and lab.ndt_info(1)["map_size_at_build"] == 0
    out = lab.scan_ndt(1, np.stack([sf.displaced()]), 1.0)
    assert out["valid"][0] == 0 and out["score"].tobytes() == np.zeros(1).tobytes()
    lab.ndt_clear()


def test_batches_index_cell_sizes_slots_rebuild_and_cap(hip, models):
    ref = models[1]
    names = ("ijk", "count", "mean", "evec", "wgt", "eval")
    stored = hip.map_points().copy()
    for cell, nb in ((0.0, 1), (0.3, 5), (1.7, 5)):      # the stored points, all kept: one batch against five, three index cell sizes
        ctx = fresh(np.array_split(stored, nb), cell_size=cell, downsample=False)
        try:
            assert np.array_equal(ctx.map_points(), stored)
            ctx.ndt_build(2, 1.0, MIN_PTS, EIG_RATIO)
            same_bytes(ref, ctx.ndt_cells(2), f"cell size {cell}, {nb} batches", names)
        finally:
            ctx.close()
    ctx = fresh(sf.standard_batches(), cell_size=0.3)
    try:
        assert np.array_equal(ctx.map_points(), hip.map_points())
        with pytest.raises(Exception, match="no map"):
            ctx.ndt_info(2)
        ctx.ndt_build(2, 2.0, MIN_PTS, EIG_RATIO)
        ctx.ndt_build(2, 1.0, MIN_PTS, EIG_RATIO)      # a rebuild replaces the slot's model
        same_bytes(ref, ctx.ndt_cells(2), "rebuilt, cell size 0.3", names)
        nc_ = ref["nc"]
        buf = np.full((nc_ + 1, 3), -7, np.int32)
        got = C.c_size_t(0)
        raw = ctx._L.flimo_ndt_cells
        assert raw(ctx._h, 2, nc_ - 1, C.byref(got), buf.ctypes.data, None, None, None, None, None) == ERR_TOO_LARGE
        assert got.value == nc_ and np.all(buf == -7)
        for cap in (nc_, nc_ + 1):
            assert raw(ctx._h, 2, cap, C.byref(got), buf.ctypes.data, None, None, None, None, None) == 0
            assert np.array_equal(buf[:nc_], ref["ijk"]) and np.all(buf[nc_:] == -7)
        ctx.ndt_clear(2)
        assert raw(ctx._h, 2, 0, C.byref(got), None, None, None, None, None, None) == ERR_NOMAP
    finally:
        ctx.close()
    assert [hip.ndt_info(s)["leaf"] for s in range(4)] == [2.0, 1.0, 0.5, 0.25] and all(hip.ndt_info(s)["stale"] == 0 for s in range(4))


# ---- 2. the terms and the sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m, hood", [(1, 1, 7), (255, 1, 7), (256, 1, 1), (257, 5, 7), (4095, 1, 7), (4096, 1, 1), (4097, 5, 7)])
def test_terms_and_sums_against_the_restatement(hip, models, n, m, hood):
    poses = np.stack([sf.displaced(), sf.displaced(dx=0.3, dyaw_deg=2), sf.displaced(dy=-0.2), sf.displaced(dx=-0.1, dyaw_deg=-1),
                      sf.displaced(dx=50.0)])[:m]
    keep = hip.scan_get()
    try:
        hip.scan_set(sf.standard_scan(n))
        got = compare(hip, models[1], 1, poses, hood, d2_of(1.0), f"n {n}", plain=(n == 257))
        assert got["valid"][0] > 0
        if m == 5:
            assert got["valid"][4] == 0 and got["cells"][4] == 0      # thrown clear of every cell: every sum is +0.0
            zero = np.concatenate([got["H"][4], got["g"][4], got["score"][4:]])
            assert zero.tobytes() == np.zeros(28).tobytes()
    finally:
        hip.scan_set(keep)


def test_hood_one_against_seven_borders_nan_points_and_underflow(hip, models):
    model, leaf = models[1], 1.0
    ident = sf.x26_of((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    inner = np.flatnonzero(np.all(np.abs(model["ijk"]) >= 2, axis=1))[0]      # (no border at 0: its lower neighbour is a denormal)
    base = model["mean"][inner].astype(np.float32)
    cell0 = np.floor(base)
    assert np.array_equal(cell0.astype(np.int32), model["ijk"][inner])
    pts = []
    for a in range(3):
        for b in (cell0[a], cell0[a] + 1):
            for v in (vc.down(b), np.float32(b), vc.up(b)):      # one float32 step either side of a border
                p = base.copy()
                p[a] = v
                pts.append(p)
    pts.append(np.float32([np.nan, 0, 0]))
    scan = np.concatenate([np.stack(pts), sf.standard_scan(100)])
    keep = hip.scan_get()
    try:
        hip.scan_set(scan)
        assert np.array_equal(hip.scan_to_world(ident)[:18], scan[:18]), "the identity pose leaves the points alone"
        poses = np.stack([ident, sf.displaced()])
        seven = compare(hip, model, 1, poses, 7, d2_of(leaf), "hood 7")
        one = compare(hip, model, 1, poses, 1, d2_of(leaf), "hood 1")
        assert np.array_equal(one["term_cell"][:, :, 0], seven["term_cell"][:, :, 0]) and np.all(one["term_cell"][:, :, 1:] == -1)
        assert np.all(seven["cells"] > one["cells"]) and np.all(seven["term_cell"][:, 18] == -1)
        own = seven["term_cell"][0, :18, 0].reshape(3, 2, 3)
        assert np.all(own[:, 0, 1] == own[:, 0, 2]) and np.all(own[:, 1, 0] == own[:, 0, 1]), "a point ON a border belongs to the upper cell"
        for d2 in (1e300,):
            dead = hip.scan_ndt(1, poses, d2, want_terms=True)
            assert np.all(dead["valid"] == 0) and np.all(dead["cells"] == 0)
            for name in ("H", "g", "score"):
                assert dead[name].tobytes() == np.zeros_like(dead[name]).tobytes(), f"d2 {d2}: {name}"
            have = dead["term_cell"] >= 0
            assert have.sum() > 100 and np.all(dead["terms"][have][:, 1] == 0.0) and not np.any(np.isnan(dead["terms"][have]))
    finally:
        hip.scan_set(keep)


def test_a_neighbour_beyond_the_lattice_edge_an_empty_model_and_an_empty_scan(lab):
    edge = np.float32(2 ** 20 - 1)      # the last cell along x at leaf 1.0: float32 steps of 1/8 there
    pts = np.float32([[edge + dx, 0.25 + 0.125 * (t % 5), 0.25 + 0.0625 * t] for t, dx in enumerate((0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 0.5))])
    lab.map_clear()
    lab.map_add(pts)
    assert lab.ndt_build(0, 1.0, 3, EIG_RATIO) == 1
    model = check_model(lab, 0, 1.0, min_pts=3, tag="lattice edge")
    assert model["ijk"][0, 0] == 2 ** 20 - 1
    lab.scan_set(pts[:3])
    ident = sf.x26_of((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    got = compare(lab, model, 0, np.stack([ident]), 7, 1.0, "lattice edge")
    assert np.all(got["term_cell"][0, :, 0] == 0) and np.all(got["term_cell"][0, :, 1:] == -1)
    lab.map_clear()
    assert lab.ndt_build(1, 1.0) == 0      # an empty model
    out = lab.scan_ndt(1, np.stack([ident, ident]), 1.0, want_terms=True)
    assert np.all(out["valid"] == 0) and np.all(np.isnan(out["terms"])) and np.all(out["term_cell"] == -1)
    lab.ndt_clear()
    ctx = fresh(sf.standard_batches())      # an empty scan
    try:
        ctx.ndt_build(0, 1.0)
        out = ctx.scan_ndt(0, np.stack([ident, ident]), 1.0, want_terms=True)
        assert out["terms"].shape == (2, 0, 7, 2) and np.all(out["valid"] == 0) and out["H"].tobytes() == np.zeros((2, 21)).tobytes()
    finally:
        ctx.close()


# ---- 3. invariance and side effects -------------------------------------------------------------------------------------------------
def test_batch_order_chunks_outputs_and_cell_size_move_no_byte(hip, models):
    poses = sf.standard_poses()[::9]      # 14 poses
    d2 = d2_of(1.0)
    whole = hip.scan_ndt(1, poses, d2, want_terms=True)
    n = hip.scan_size()
    order = np.random.default_rng(1).permutation(len(poses))
    shuffled = hip.scan_ndt(1, poses[order], d2, want_terms=True)
    same_bytes({k: v[order] for k, v in whole.items()}, shuffled, "pose order")
    for j in (0, 7):
        same_bytes({k: v[j:j + 1] for k, v in whole.items()}, hip.scan_ndt(1, poses[j:j + 1], d2, want_terms=True), f"pose {j} alone")
    try:
        for chunk in (1, 3 * n):
            hip.set_ndt_chunk(chunk)
            same_bytes(whole, hip.scan_ndt(1, poses, d2, want_terms=True), f"chunks of {chunk} pairs")
    finally:
        hip.set_ndt_chunk(0)
    same_bytes(whole, hip.scan_ndt(1, poses, d2), "without the terms", NAMES[:5])
    ctx = fresh(sf.standard_batches(), sf.standard_scan(), cell_size=1.3)
    try:
        ctx.ndt_build(0, 1.0, MIN_PTS, EIG_RATIO)
        same_bytes(whole, ctx.scan_ndt(0, poses, d2, want_terms=True), "index cell size 1.3")
    finally:
        ctx.close()


def test_a_model_is_a_snapshot_and_the_call_leaves_map_scan_and_a_pass_alone(models):
    from fast_limo_amd import _lib
    cfg = _lib.default_match_cfg(**CAPS)
    poses = sf.standard_poses()[[sf.TRUE_POSE, 30, 99]]
    d2 = d2_of(1.0)

    def run(call):
        ctx = fresh(sf.standard_batches()[:3], sf.standard_scan())
        try:
            out = []
            if call:
                ctx.ndt_build(0, 1.0, MIN_PTS, EIG_RATIO)
                out.append(ctx.scan_ndt(0, poses, d2, want_terms=True))
                assert ctx.ndt_info(0)["stale"] == 0
            passes = [ctx.match_reduce(poses[0], cfg)]
            ctx.map_add(sf.standard_batches()[3])
            if call:
                assert ctx.ndt_info(0)["stale"] == 1 and ctx.ndt_info(0)["map_size_at_build"] < ctx.map_size()
                out.append(ctx.scan_ndt(0, poses, d2, want_terms=True))
            passes.append(ctx.match_reduce(poses[0], cfg))
            assert ctx.map_crop_box(np.float32([-30, -4, -5]), np.float32([6, 30, 30])) > 500
            if call:
                out.append(ctx.scan_ndt(0, poses, d2, want_terms=True))
                assert ctx.ndt_info(0)["stale"] == 1
            passes.append(ctx.match_reduce(poses[0], cfg))
            return out, passes, ctx.map_points().copy(), ctx.scan_get().copy()
        finally:
            ctx.close()
    (ndt, with_calls, mp_a, scan_a), (_, twin, mp_b, scan_b) = run(True), run(False)
    same_bytes(ndt[0], ndt[1], "after an insert")
    same_bytes(ndt[0], ndt[2], "after a crop")
    assert ndt[0]["valid"][0] > 500
    assert mp_a.tobytes() == mp_b.tobytes() and scan_a.tobytes() == scan_b.tobytes()
    for j, (a, b) in enumerate(zip(with_calls, twin)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], f"pass {j}"


def test_every_rejected_argument_leaves_the_outputs_and_the_model_untouched(hip, models):
    from fast_limo_amd import _abi
    n = hip.scan_size()
    good = np.ascontiguousarray(sf.standard_poses()[:3])
    out = dict(valid=np.full(3, -7, np.int32), cells=np.full(3, -7, np.int64), H=np.full((3, 21), -7.0), g=np.full((3, 6), -7.0),
               score=np.full(3, -7.0), terms=np.full((3, n, 7, 2), -7.0), term_cell=np.full((3, n, 7), -7, np.int32))
    p = {k: a.ctypes.data for k, a in out.items()}

    def raw(x=good, m=3, slot=1, hood=7, d2=1.0, h=hip._h, **null):
        q = dict(p, **{name: None for name in null})
        return hip._L.flimo_scan_ndt(h, slot, None if x is None else x.ctypes.data, m, hood, d2, *(q[k] for k in NAMES))
    assert raw(h=None) == ERR_INVALID and raw(x=None) == ERR_INVALID
    for name in NAMES[:5]:
        assert raw(**{name: True}) == ERR_INVALID, name
    for hood in (0, 2, 6, 8, 27, -1):
        assert raw(hood=hood) == ERR_INVALID, hood
    for d2 in (np.nan, 0.0, -1.0, np.inf, -np.inf):
        assert raw(d2=d2) == ERR_INVALID, d2
    for slot in (-1, 4, 100):
        assert raw(slot=slot) == ERR_INVALID, slot
    x = good.copy()
    x[2, 5] = np.nan
    assert raw(x=x) == ERR_INVALID and raw(m=2 ** 31) == ERR_TOO_LARGE
    lone = fresh([sf.standard_batches()[0]], sf.standard_scan())
    try:
        assert raw(h=lone._h) == ERR_NOMAP      # nothing was built in that context
        with pytest.raises(Exception, match="no map"):
            lone.scan_ndt(0, good, 1.0)
    finally:
        lone.close()
    for a in out.values():
        assert np.all(a == -7)
    # the build's rejections leave *nc and the old model alone
    nc_ = C.c_size_t(77)
    for slot, leaf, mp, ratio in ((4, 1.0, 6, 0.01), (-1, 1.0, 6, 0.01), (1, 0.0, 6, 0.01), (1, np.nan, 6, 0.01), (1, 1e-39, 6, 0.01), (1, 1.0, 2, 0.01),
                                  (1, 1.0, 6, 0.0), (1, 1.0, 6, 1.5), (1, 1.0, 6, np.nan), (1, 1.0, 6, -0.1)):
        k = _abi.NdtCfg(leaf, mp, ratio)
        assert hip._L.flimo_ndt_build(hip._h, slot, C.byref(k), C.byref(nc_)) == ERR_INVALID, (slot, leaf, mp, ratio)
    assert nc_.value == 77 and hip._L.flimo_ndt_build(hip._h, 1, None, C.byref(nc_)) == ERR_INVALID
    same_bytes(models[1], hip.ndt_cells(1), "the old model", ("ijk", "count", "mean", "evec", "wgt", "eval"))
    assert raw() == 0 and np.all(out["valid"] >= 0)
    x = good.copy()
    x[:, 7:] = np.nan      # only pos and rot of a pose are read
    same_bytes(hip.scan_ndt(1, x, 1.0), hip.scan_ndt(1, good, 1.0), "the rest of a pose")


def test_through_the_localizer(built):
    from fast_limo_amd import api
    mp, scan, imu = cfg1_scene()
    poses = np.stack([sf.displaced(), sf.displaced(dx=0.2), sf.displaced(dx=60.0)])
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        with pytest.raises(Exception, match="flimo_loc_scan_ndt failed \\(-4\\)"):
            loc.scan_ndt(0, poses, 1.0)
        loc.set_async_insert(True)
        assert drive_two_scans(loc, mp, scan, imu)[1] == 0
        cells = loc.ndt_build(0, 1.0, MIN_PTS, EIG_RATIO)      # (an insert may still be running: the call waits)
        found = loc.scan_ndt(0, poses, d2_of(1.0), want_terms=True)
        loc.sync()
        ctx = fresh([loc.hip.map_points().copy()], loc.pc2match().copy(), downsample=False)
        try:
            assert np.array_equal(ctx.map_points(), loc.hip.map_points())
            assert ctx.ndt_build(0, 1.0, MIN_PTS, EIG_RATIO) == cells == loc.ndt_info(0)["cells"] > 50
            same_bytes(loc.ndt_cells(0), ctx.ndt_cells(0), "the model", ("ijk", "count", "mean", "evec", "wgt", "eval"))
            same_bytes(found, ctx.scan_ndt(0, poses, d2_of(1.0), want_terms=True), "Localizer against HipCtx")
            assert found["valid"][2] == 0 and found["valid"][0] > 100
        finally:
            ctx.close()
        loc.ndt_clear()
    finally:
        loc.close()


# ---- 4. the loop over the call ------------------------------------------------------------------------------------------------------
def test_ndt_align_ends_where_the_restatement_ends(hip):
    """The bar is twice the restatement's worst end error over the kept starts (test_ndt_host.py: REF_END, which starts were dropped
    and why); the margin covers the float64 differences of exp and of the eigenvectors across the iterations."""
    from fast_limo_amd import api
    start = sl.start_poses(KEPT + WIDE)
    res = api.ndt_align(hip, start, (0, 1, 2), hood=7, outlier_ratio=OUTLIER)
    again = api.ndt_align(hip, start, (0, 1, 2), hood=7, outlier_ratio=OUTLIER)
    errs = [sl.pose_error(x) for x in res["x26"]]
    plane = api.scan_align(hip, sl.start_poses(WIDE))
    for s, (dp, dr), it, v in zip(KEPT + WIDE, errs, res["iters"], res["valid"]):
        print(f"ndt_align start {s}: iterations {it}, valid {v}; {dp * 1e3:.2f} mm, {dr:.4f} deg")
    for s, x in zip(WIDE, plane["x26"]):
        print(f"scan_align (default gate) from the wide start {s}: {sl.pose_error(x)}")
    for name in ("x26", "valid", "cost", "iters", "status"):
        assert res[name].tobytes() == again[name].tobytes(), f"two runs: {name} differs"
    assert len(res["stages"]) == 3 and np.all(res["cost"][:len(KEPT)] < 0)
    for s, (dp, dr) in list(zip(KEPT + WIDE, errs))[:len(KEPT)]:
        assert dp <= 2 * REF_END[0] and dr <= 2 * REF_END[1], (s, dp, dr)
