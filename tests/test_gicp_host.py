"""CPU: what of GICP (flimo_gicp_build / flimo_scan_gicp, api.gicp_covs / gicp_align) can be checked without a device -- the two
host/device functions (flimo_gicp_regularize_host, flimo_gicp_term_host) against the numpy restatement (tests/gicp_common.py) and
against pairs worked by hand, the restatement against itself (the shape of the sums in numpy, in plain Python floats and by
math.fsum; g against finite differences of half the cost; H positive semidefinite), the bindings of both classes, and the
restatement's own Gauss-Newton, whose end error is recorded here and is what the GPU test's alignment is held to."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import gicp_common as gc
import normals_common as nc
import scan_fitness_common as sf
import scan_linearize_common as sl
from fast_limo_amd import _abi, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_COV, EPS, GATE = 20, 1e-3, 1.0
# Where the restatement's Gauss-Newton ends on the standard scene (20 000 map points fed in four batches, a 1 024-point scan;
# covariances of both clouds from their 20 nearest by numpy, FLIMO_GICP_PLANE at eps 1e-3, gate 1 m, api.gicp_align's 10 steps),
# from all nine starts of scan_linearize_common.STARTS: the worst distance [m] and angle [deg] to the true pose.  Measured, not
# chosen: every start ends at the same pose to 1e-7 (20 and 30 steps move it by less than 1e-8), all 1 024 pairs valid.
REF_END = (0.0033631, 0.0097276)


@pytest.fixture(scope="module")
def scene(built):
    """The stored points of the standard scene by the host's replay of the insert rule, the scan, and both clouds' covariances."""
    batches = sf.standard_batches()
    keeps, stored = _lib.insert_rule_replay(batches)
    mp = np.concatenate([b[k] for b, k in zip(batches, keeps)])
    assert mp.shape[0] == stored
    scan = sf.standard_scan()
    return dict(mp=mp, scan=scan, model=gc.regularize_numpy(gc.knn_covs(mp, mp, K_COV), gc.PLANE, EPS),
                scov=gc.regularize_numpy(gc.knn_covs(scan, scan, K_COV), gc.PLANE, EPS))


def test_the_rules_and_the_structs_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    rule = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FLIMO_GICP_([A-Z]+) (\d+)", txt)}
    assert rule == dict(PLANE=_lib.GICP_PLANE, CLAMP=_lib.GICP_CLAMP) == dict(PLANE=gc.PLANE, CLAMP=gc.CLAMP)
    assert C.sizeof(_abi.GicpCfg) == 24 and C.sizeof(_abi.GicpInfo) == 48


# ---- gicp_term ----

def _random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    b = (w + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
    p = rng.uniform(-15, 15, (n, 3)).astype(np.float32)
    q = rng.normal(size=4)
    R = sl.quat_R(q).astype(np.float32)
    covs = []
    for _ in range(2):
        pts = rng.normal(size=(n, 12, 3)) * rng.uniform(0.01, 1.0, (n, 1, 3))
        d = pts - pts.mean(1, keepdims=True)
        covs.append(np.stack([(d[:, :, i] * d[:, :, j]).mean(1) for i, j in nc.PAIRS], 1))
    return w, b, p, R, covs[0], covs[1]


def test_the_host_term_is_the_restatement_bit_for_bit_on_random_pairs(built):
    w, b, p, R, CA, CB = _random_pairs(400, 7)
    CA[::5] = gc.regularize_numpy(CA[::5], gc.PLANE, EPS)
    CB[::3] = gc.regularize_numpy(CB[::3], gc.CLAMP, 0.01)
    ref = gc.term(w, b, p, R, CA, CB)
    assert ref["live"].all()
    for i in range(w.shape[0]):
        live, m, det, sums = api.gicp_term_host(w[i], b[i], p[i], R, CA[i], CB[i])
        assert live and m == ref["m"][i] and det == ref["det"][i]
        assert sums.tobytes() == ref["C"][i].tobytes(), i
        assert sums[27] == m


def test_the_host_term_on_a_pair_worked_by_hand(built):
    """R = I, CA = diag(1, 1, 2^-10), CB = diag(1, 2^-10, 1): S = diag(2, s, s) with s = 1 + 2^-10, det = 2 s^2 (exact),
    M = diag(1/2, q, q) with q = fl(1 / s); r = (-1/8, 0, -1/4), p = (1/2, 1/4, 1/8).  Every product below is a scaling by a power
    of two, every sum rounds once."""
    s = 1.0 + 2.0 ** -10
    q = 1.0 / s
    live, m, det, sums = api.gicp_term_host([1.0, 2.0, 3.0], [1.125, 2.0, 3.25], [0.5, 0.25, 0.125], np.eye(3), [1, 0, 0, 1, 0, 2.0 ** -10],
                                            [1, 0, 0, 2.0 ** -10, 0, 1])
    H, g = api.sym6(sums[:21]), sums[21:27]
    assert live and det == 2.0 * (s * s) and m == 0.0078125 + 0.0625 * q == sums[27]
    assert np.array_equal(np.diag(H)[:3], [0.5, q, q]) and H[0, 1] == H[0, 2] == H[1, 2] == 0.0
    # J3 = (0, -pz, py), J4 = (pz, 0, -px), J5 = (-py, px, 0)
    assert H[3, 3] == 0.015625 * q + 0.0625 * q and H[4, 4] == 0.015625 * 0.5 + 0.25 * q and H[5, 5] == 0.0625 * 0.5 + 0.25 * q
    assert np.array_equal(g[:3], [-0.0625, 0.0, -0.25 * q]) and g[3] == 0.25 * (-0.25 * q) and g[4] == 0.125 * -0.0625 + 0.5 * (0.25 * q)
    assert g[5] == -0.25 * -0.0625


def test_axis_aligned_covariances_give_a_diagonal_M(built):
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, c = rng.uniform(1e-3, 2.0, 3), rng.uniform(1e-3, 2.0, 3)
        CA, CB = [a[0], 0, 0, a[1], 0, a[2]], [c[0], 0, 0, c[1], 0, c[2]]
        w = rng.uniform(-5, 5, 3).astype(np.float32)
        b = (w + rng.normal(0, 0.2, 3)).astype(np.float32)
        p = rng.uniform(-5, 5, 3).astype(np.float32)
        live, m, det, sums = api.gicp_term_host(w, b, p, np.eye(3), CA, CB)
        ref = gc.term(w[None], b[None], p[None], np.eye(3), [CA], [CB])
        assert live and sums.tobytes() == ref["C"][0].tobytes() and det == ref["det"][0]
        H = api.sym6(sums[:21])
        assert H[0, 1] == H[0, 2] == H[1, 2] == 0.0 and np.all(np.diag(H)[:3] > 0.0)
        r = w.astype(np.float64) - b.astype(np.float64)
        assert m == pytest.approx(float(np.sum(r * r / (a + c))), rel=1e-14)
        assert np.diag(H)[:3] == pytest.approx(1.0 / (a + c), rel=1e-14)


@pytest.mark.parametrize("CA, CB, why", [
    ([1, 0, 0, 1, 0, np.nan], [1, 0, 0, 1, 0, 1], "a NaN in the scan's covariance"),
    ([1, 0, 0, 1, 0, 1], [np.nan] * 6, "a NaN row of the model"),
    ([1, 0, 0, 1, 0, 1], [1, 0, np.inf, 1, 0, 1], "an infinity"),
    ([0] * 6, [0] * 6, "det == 0"),
    ([0] * 6, [-1, 0, 0, 1, 0, 1], "a negative det"),
    ([0] * 6, [1e-103, 0, 0, 1e-103, 0, 1e-103], "a det whose reciprocal overflows"),
])
def test_the_term_is_not_live(built, CA, CB, why):
    live, m, det, sums = api.gicp_term_host([1, 2, 3], [1.5, 2, 3], [1, 1, 1], np.eye(3), CA, CB)
    assert not live and m == 0.0 and det == 0.0 and not sums.any(), why
    ref = gc.term(np.float32([[1, 2, 3]]), np.float32([[1.5, 2, 3]]), np.float32([[1, 1, 1]]), np.eye(3), [CA], [CB])
    assert not ref["live"][0] and not ref["C"].any(), why


# ---- gicp_regularize ----

def test_both_rules_on_a_covariance_with_known_axes(built):
    cov = [4.0, 0, 0, 1.0, 0, 0.25]      # l = (1/4, 1, 4) along z, y, x: no rotation is needed
    l, v = api.gicp_eigen_host(cov)
    assert np.array_equal(l, [0.25, 1.0, 4.0]) and np.array_equal(v, [[0, 0, 1], [0, 1, 0], [1, 0, 0]])
    for rule, eps, want in ((gc.PLANE, 2.0 ** -10, [1, 0, 0, 1, 0, 2.0 ** -10]), (gc.CLAMP, 0.5, [4, 0, 0, 2, 0, 2]),
                            (gc.PLANE, 1.0, [1, 0, 0, 1, 0, 1]), (gc.CLAMP, 1.0, [4, 0, 0, 4, 0, 4]), (gc.CLAMP, 2.0 ** -10, cov)):
        has, out = api.gicp_regularize_host(cov, rule, eps)
        assert has and np.array_equal(out, want), (rule, eps)


def test_coplanar_collinear_and_zero_covariances(built):
    for cov, has_want in (([1.0, 0.25, 0, 1.0, 0, 0.0], True), ([2.0, 0, 0, 0, 0, 0], True), ([0.0] * 6, False),
                          ([1, 0, 0, np.nan, 0, 1], False), ([np.inf, 0, 0, 1, 0, 1], False), ([-1.0, 0, 0, -2.0, 0, -3.0], False)):
        for rule in (gc.PLANE, gc.CLAMP):
            has, out = api.gicp_regularize_host(cov, rule, EPS)
            assert has == has_want
            if not has:
                assert np.all(np.isnan(out))
                continue
            l, v = api.gicp_eigen_host(cov)
            assert out.tobytes() == gc.regularize(l, v, rule, EPS).tobytes()
            assert np.linalg.eigvalsh(gc.sym3(out)).min() > 0.0, "a regularised covariance is positive definite"
    has, out = api.gicp_regularize_host([1.0, 0.25, 0, 1.0, 0, 0.0], gc.PLANE, EPS)      # the plane z = 0: eps along z
    assert np.array_equal(out[[2, 4]], [0, 0]) and out[5] == EPS


def test_one_step_either_side_of_the_clamp(built):
    # l = (a, 2, 4) along x, y, z; eps = 1/4: floor = 1.0
    for a, want in ((np.nextafter(1.0, 0.0), 1.0), (1.0, 1.0), (np.nextafter(1.0, 2.0), np.nextafter(1.0, 2.0))):
        has, out = api.gicp_regularize_host([a, 0, 0, 2.0, 0, 4.0], gc.CLAMP, 0.25)
        assert has and np.array_equal(out, [want, 0, 0, 2.0, 0, 4.0]), a


def test_the_eigen_pairs_are_numpys_and_the_matrix_is_exactly_theirs(built):
    _, _, _, _, CA, CB = _random_pairs(300, 11)
    for cov in np.concatenate([CA, CB]):
        l, v = api.gicp_eigen_host(cov)
        M = gc.sym3(cov)
        fro = np.linalg.norm(M)
        assert l[0] <= l[1] <= l[2]
        assert np.all(np.abs(l - np.linalg.eigvalsh(M)) <= nc.U_EIG * fro)
        for k in range(3):
            assert np.linalg.norm(M @ v[k] - l[k] * v[k]) <= nc.U_EIG * fro and abs(np.linalg.norm(v[k]) - 1.0) <= nc.U_EIG
        for rule, eps in ((gc.PLANE, EPS), (gc.CLAMP, 0.01), (gc.CLAMP, 1.0)):
            has, out = api.gicp_regularize_host(cov, rule, eps)
            assert has and out.tobytes() == gc.regularize(l, v, rule, eps).tobytes()
    with pytest.raises(_lib.FlimoError):
        api.gicp_regularize_host(CA[0], 2, EPS)
    for eps in (0.0, -1.0, 1.5, np.nan):
        with pytest.raises(_lib.FlimoError):
            api.gicp_regularize_host(CA[0], gc.PLANE, eps)


# ---- the restatement against itself ----

def test_the_shape_in_numpy_is_the_shape_in_plain_floats_and_meets_fsum(scene):
    x26 = sl.start_poses(((0.1, 0.1, 1),))[0]
    for n in (257, 1024):
        r = gc.restate(x26, scene["scan"][:n], scene["scov"][:n], scene["mp"], scene["model"], GATE)
        assert r["valid"].sum() > 0.9 * n
        a, b = gc.shape_sums(r["C"]), gc.shape_sums_plain(r["C"])
        assert a.tobytes() == b.tobytes()
        S, A, cnt = gc.fsum_sums(r["C"])
        assert np.all(np.abs(a - S) <= sl.sum_bound(cnt, A))


def test_H_is_symmetric_positive_semidefinite_on_the_standard_scene(scene):
    for start in ((0, 0, 0), (0.5, -0.5, -5), (1, 1, 10)):
        r = gc.restate(sl.start_poses((start,))[0], scene["scan"], scene["scov"], scene["mp"], scene["model"], GATE)
        S, A, cnt = gc.fsum_sums(r["C"])
        H = api.sym6(gc.shape_sums(r["C"])[:21])
        assert np.array_equal(H, H.T) and r["valid"].sum() > 500
        assert np.all(np.linalg.eigvalsh(H) >= -sl.sum_bound(cnt, A[:21].max())), "H is positive semidefinite"
        assert np.linalg.eigvalsh(H).min() > 0.0, "and, with a thousand pairs on six walls, definite"


def test_g_is_the_gradient_of_half_the_cost_at_fixed_M(scene):
    """Central differences of F = 1/2 sum m over the body-frame perturbation, the neighbours and every M held, w moved in float64
    (the float32 rounding of w is a property of the call, not of the derivative).  r(h) = R Exp(h e) p + .. moves by at most
    rho = 1 + |p| per unit step, and so do its second and third derivatives; F''' of 1/2 r^T M r is r'''^T M r + 3 r'^T M r'', at most
    ||M|| rho (|r| + 3 rho).  A central difference with step h is off by h^2 / 6 of that (twice it covers the fifth-order
    remainder at h = 1e-5), plus the rounding 8 eps * sum m / h of the two costs."""
    scan, scov, mp, model = scene["scan"], scene["scov"], scene["mp"], scene["model"]
    x26 = sl.start_poses(((0.05, -0.05, 0.5),))[0]
    r0 = gc.restate(x26, scan, scov, mp, model, GATE)
    ok = r0["valid"]
    Mx = sf.pose_rt(x26).astype(np.float64)
    R, t = Mx[:, :3], Mx[:, 3]
    p = scan.astype(np.float64)[ok]
    b = mp[r0["idx"][ok]].astype(np.float64)
    S = gc.sym3(model[r0["idx"][ok]]) + R @ gc.sym3(scov[ok]) @ R.T
    Minv = np.linalg.inv(S)

    def half_cost(xi):
        th = float(np.linalg.norm(xi[3:]))
        K = np.array([[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]])
        E = np.eye(3) + (math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K if th > 0 else 0)
        r = (p @ E.T + xi[:3]) @ R.T + t - b
        return 0.5 * math.fsum(np.einsum("ia,iab,ib->i", r, Minv, r))
    t0 = gc.term(p @ R.T + t, mp[r0["idx"][ok]], scan[ok], Mx[:, :3], scov[ok], model[r0["idx"][ok]], wide_w=True)
    assert t0["live"].all()
    Ssum, A, _ = gc.fsum_sums(t0["C"])
    assert abs(2.0 * half_cost(np.zeros(6)) - Ssum[27]) <= 1e-9 * Ssum[27]
    h = 1e-5
    rho = 1.0 + np.linalg.norm(p, axis=1)
    rn = np.linalg.norm((p @ R.T + t) - b, axis=1)
    third = float(np.sum(np.linalg.norm(Minv, 2, axis=(1, 2)) * rho * (rn + 3.0 * rho)))
    bound = 2.0 * h * h / 6.0 * third + 8 * 2.0 ** -52 * Ssum[27] / h
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        fd = (half_cost(e) - half_cost(-e)) / (2 * h)
        print("g", a, fd, Ssum[21 + a], abs(fd - Ssum[21 + a]), bound)
        assert abs(fd - Ssum[21 + a]) <= bound, (a, fd, Ssum[21 + a])
    assert ok.sum() > 900 and np.abs(Ssum[21:27]).max() > 100 * bound


def test_the_restatement_converges_from_all_nine_starts_to_the_recorded_end(scene):
    lin = gc.linearizer(scene["scan"], scene["scov"], scene["mp"], scene["model"], GATE)
    out = api.scan_align(None, sl.start_poses(sl.STARTS), iters=10, min_valid=30, linearize=lin)
    errs = np.array([sl.pose_error(r) for r in out["x26"]])
    print("restatement ends", errs.tolist())
    assert np.all(out["status"] == api.ALIGN_RUNNING) and np.all(out["valid"] == scene["scan"].shape[0])
    assert errs[:, 0].max() <= REF_END[0] * 1.01 and errs[:, 1].max() <= REF_END[1] * 1.01
    assert errs[:, 0].max() >= REF_END[0] * 0.99 and errs[:, 1].max() >= REF_END[1] * 0.99, "REF_END is the measured worst, not a loose cap"


# ---- the bindings, on a recording stand-in for the libraries (test_bindings_host.py's) ----
from test_bindings_host import _hip_ctx, _localizer, _shape      # noqa: E402

_LIN = dict(valid="int32:1", H="float64:2", g="float64:2", cost="float64:1")
_GICP_CASES = [
    ("gicp_build", "flimo_gicp_build", "flimo_loc_gicp_build", (), dict(k=10, rule=1, eps=0.01), "int"),
    ("gicp_info", "flimo_gicp_info", "flimo_loc_gicp_info", (), {},
     dict(points="int", n_cov="int", eps="float", k="int", max_dist="float", min_pts="int", rule="int", stale="int")),
    ("gicp_model", "flimo_gicp_model", "flimo_loc_gicp_model", (0, 3), {}, "float64:2"),
    ("gicp_clear", "flimo_gicp_clear", "flimo_loc_gicp_clear", (), {}, "NoneType"),
    ("scan_cov_set", "flimo_scan_cov_set", "flimo_loc_scan_cov_set", (np.zeros((2, 6)),), {}, "NoneType"),
    ("scan_cov_set", "flimo_scan_cov_set", "flimo_loc_scan_cov_set", (None,), {}, "NoneType"),
    ("scan_gicp", "flimo_scan_gicp", "flimo_loc_scan_gicp", (np.zeros((2, 26)),), {}, _LIN),
    ("scan_gicp", "flimo_scan_gicp", "flimo_loc_scan_gicp", (np.zeros((2, 26)), 2.0), dict(want_pairs=True),
     dict(_LIN, pair_idx="int32:2", pair_m="float64:2")),
]


@pytest.mark.parametrize("case", _GICP_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(_GICP_CASES)])
def test_the_gicp_methods_are_shared_and_call_their_symbols(case):
    method, hip_sym, loc_sym, args, kw, shape = case
    assert getattr(_lib.HipCtx, method) is getattr(api.Localizer, method)
    for make, sym, msg in ((_hip_ctx, hip_sym, "invalid argument: said the library"), (_localizer, loc_sym, f"{loc_sym} failed (-2)")):
        obj = make(0)
        out = getattr(obj, method)(*args, **kw)
        calls = [(name, a) for name, a in obj._L.calls if not name.endswith("_size") and name != "flimo_loc_ctx"]
        assert calls and {name for name, _ in calls} == {sym} and all(a[0] is obj._h for _, a in calls)
        assert _shape(out) == shape
        with pytest.raises(_lib.FlimoError) as err:
            getattr(make(-2), method)(*args, **kw)
        assert str(err.value) == msg


def test_the_chunk_and_the_covariance_count_go_to_the_maps_context():
    for make in (_hip_ctx, _localizer):
        obj = make(0)
        assert _lib.HipCtx.set_gicp_chunk is api.Localizer.set_gicp_chunk and _lib.HipCtx.scan_cov_size is api.Localizer.scan_cov_size
        obj.set_gicp_chunk(4096)
        assert obj.scan_cov_size() == 0
        rec = getattr(obj, "hip", obj)._L
        assert [(name, a[1:]) for name, a in rec.calls if name != "flimo_loc_ctx"] == [("flimo_set_gicp_chunk", (4096,)), ("flimo_scan_cov_size", ())]


def test_the_gicp_rows_are_declared_on_both_libraries(built):
    L, H = _lib.load_hip(), api.load_host()
    assert len(_abi.PAIRED_GICP) == 6
    for hip, loc, args in _abi.PAIRED_GICP:
        assert list(getattr(L, hip).argtypes[1:]) == list(getattr(H, loc).argtypes[1:]) == list(args), hip
        assert _abi.LOC_OF[hip] == loc
    for name in ("flimo_set_gicp_chunk", "flimo_scan_cov_size", "flimo_gicp_eigen_host", "flimo_gicp_regularize_host", "flimo_gicp_term_host"):
        assert getattr(L, name).argtypes is not None


def test_gicp_covs_regularises_the_scan_contexts_covariances_and_keeps_nan_rows(built):
    rng = np.random.default_rng(5)
    cov = rng.normal(size=(6, 4, 3))
    cov = np.stack([(cov[:, :, i] * cov[:, :, j]).mean(1) for i, j in nc.PAIRS], 1)
    cov[2] = np.nan

    class Obj:
        def __init__(self):
            self.calls = []

        def map_size(self):
            return 6

        def normals(self, q, k, max_dist, min_pts, want):
            self.calls.append(("normals", len(q), k, max_dist, min_pts, want))
            return dict(cov=cov.copy())

        def normals_range(self, first, n, k, max_dist, min_pts, want):
            self.calls.append(("range", first, n, k, max_dist, min_pts, want))
            return dict(cov=cov.copy())
    obj = Obj()
    a = api.gicp_covs(obj, np.zeros((6, 3)), k=7, max_dist=2.0, min_pts=4, rule=gc.CLAMP, eps=0.01)
    b = api.gicp_covs(obj, k=7, max_dist=2.0, min_pts=4, rule=gc.CLAMP, eps=0.01)
    assert obj.calls == [("normals", 6, 7, 2.0, 4, ("cov",)), ("range", 0, 6, 7, 2.0, 4, ("cov",))]
    assert a.tobytes() == b.tobytes() and np.all(np.isnan(a[2])) and np.all(np.isfinite(np.delete(a, 2, 0)))
    for i in (0, 1, 3, 4, 5):
        assert a[i].tobytes() == api.gicp_regularize_host(cov[i], gc.CLAMP, 0.01)[1].tobytes()


from test_corr_graph_host import canned      # noqa: E402,F401  (relocalize's stages replaced by recorders)


def test_relocalize_ends_in_gicp_align_only_when_asked(canned, monkeypatch):      # noqa: F811
    map_obj, scan_obj, log, qi, rj = canned
    calls = []

    def gicp_align(obj, x, **kw):
        calls.append((obj, np.array(x), kw))
        return dict(x26=np.array(x) + 1.0)
    monkeypatch.setattr(api, "gicp_align", gicp_align)
    plain = api.relocalize(map_obj, scan_obj, nh=64)      # the default stays point-to-plane
    assert calls == [] and np.array_equal(plain["x26"], plain["fitness"]["x26"][0])
    out = api.relocalize(map_obj, scan_obj, nh=64, refine="gicp", gicp=dict(max_dist=2.0, iters=5))
    assert len(calls) == 1 and calls[0][0] is map_obj and calls[0][2] == dict(max_dist=2.0, iters=5)
    assert np.array_equal(calls[0][1], out["fitness"]["x26"][:1]) and np.array_equal(out["x26"], out["fitness"]["x26"][0] + 1.0)
    with pytest.raises(ValueError, match="refine"):
        api.relocalize(map_obj, scan_obj, refine="icp")


def test_gicp_align_is_scan_align_on_scan_gicp():
    class Obj:
        def __init__(self):
            self.calls = []

        def scan_gicp(self, xs, max_dist):
            self.calls.append((len(xs), max_dist))
            m = len(xs)
            H = np.zeros((m, 21))
            H[:, [0, 6, 11, 15, 18, 20]] = 1.0      # the identity
            return dict(valid=np.full(m, 100, np.int32), H=H, g=np.zeros((m, 6)), cost=np.full(m, 3.0))
    obj = Obj()
    x = np.zeros((2, 26))
    x[:, 6] = 1.0
    out = api.gicp_align(obj, x, max_dist=0.5, iters=3)
    assert obj.calls == [(2, 0.5)] * 3 and np.all(out["cost"] == 3.0) and np.array_equal(out["x26"], x) and np.all(out["iters"] == 3)
