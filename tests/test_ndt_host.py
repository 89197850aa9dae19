"""CPU: what of NDT (flimo_ndt_build / flimo_scan_ndt, api.ndt_params / ndt_align) can be checked without a device -- the one
host/device function of a term (flimo_ndt_term_host) against the numpy restatement (tests/ndt_common.py), the restatement against
itself (the shape of the sums in numpy, in plain Python floats and by math.fsum; g against finite differences of -score), PCL's
(d1, d2), the bindings of both classes, and the restatement's own coarse-to-fine Gauss-Newton, whose end error is the source of the
GPU test's bar."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ndt_common as nd
import scan_fitness_common as sf
import scan_linearize_common as sl
from fast_limo_amd import _abi, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES = (2.0, 1.0, 0.5)
MIN_PTS, EIG_RATIO, OUTLIER = 6, 0.01, 0.55
# The starts of the convergence tests: scan_linearize_common.STARTS and two wider ones, (2, 2, 20 deg) and (-2, 1, -20 deg).  The
# restatement's Gauss-Newton (leaves 2.0 / 1.0 / 0.5, api.ndt_align's default of 30 steps each; measured once over all eleven, 69 s)
# converges from all nine of STARTS = KEPT: every one ends at the same pose to 1e-7, REF_END off the true one -- the minimum of the
# leaf-0.5 objective over this sparse map, whose cells hold 6 to 10 points each.  It converges from neither wide start: they end
# 2.26 m / 13.2 deg and 1.67 m / 11.8 deg off.  The scene is a box of flat walls; a wall's cell is clamped to
# sigma = sqrt(eig_ratio * l2) = 6 cm across the wall at leaf 2.0, so a scan 2 m and 20 degrees off leaves most points many
# sigma from every cell and the step has nothing to pull on.  Both are dropped.  (With 10 steps a leaf only the four starts within
# 0.5 m / 5 deg arrive.)  The CPU test below runs CPU_STARTS, three of the nine.
KEPT = sl.STARTS
CPU_STARTS = ((0.5, 0, 0), (1, 1, 10), (-1, 1, -10))
WIDE = ((2, 2, 20), (-2, 1, -20))
REF_END = (0.048517, 0.97995)      # the restatement's worst end error over KEPT: position [m], rotation [deg]


@pytest.fixture(scope="module")
def scene(built):
    """The stored points of the standard scene by the host's replay of the insert rule, the scan, and the three numpy models."""
    batches = sf.standard_batches()
    keeps, stored = _lib.insert_rule_replay(batches)
    mp = np.concatenate([b[k] for b, k in zip(batches, keeps)])
    assert mp.shape[0] == stored
    return dict(mp=mp, scan=sf.standard_scan(), models=[nd.model_numpy(mp, leaf, MIN_PTS, EIG_RATIO) for leaf in LEAVES])


def test_the_error_codes_and_the_slot_count_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    code = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FLIMO_(ERR_[A-Z_]+|NDT_SLOTS) \(?(-?\d+)\)?", txt)}
    assert (code["ERR_INVALID"], code["ERR_NOMAP"], code["ERR_TOO_LARGE"]) == (-2, -4, -5)
    assert code["NDT_SLOTS"] == _lib.NDT_SLOTS == 4
    assert C.sizeof(_abi.NdtCfg) == 16 and C.sizeof(_abi.NdtInfo) == 40


@pytest.mark.parametrize("o, leaf", [(0.55, 1.0), (0.55, 2.0), (0.1, 0.5)])
def test_ndt_params_are_pcls_formulas(o, leaf):
    c1, c2 = 10 * (1 - o), o / leaf ** 3
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    got = api.ndt_params(o, leaf)
    assert got == pytest.approx((d1, d2), rel=1e-14, abs=0) and got[0] < 0 < got[1]


def test_the_host_term_is_the_restatement_exact_given_its_e(scene):
    """m with no tolerance, e within EXP_ULPS spacings of np.exp(x), the 28 contributions bit for bit given the function's own e;
    a d2 that underflows every e: not live, all sums +0.0."""
    model, scan = scene["models"][1], scene["scan"]
    x26 = sl.start_poses(((0.2, -0.1, 2),))[0]
    R = sf.pose_rt(x26)[:, :3]
    seen = 0
    for d2 in (api.ndt_params(OUTLIER, 1.0)[1], 1e6):
        r = nd.restate(x26, scan, model, 7, d2)
        for i, s in np.argwhere(r["cell"] >= 0)[::17]:
            c = r["cell"][i, s]
            live, m, e, sums = api.ndt_term_host(r["w"][i], scan[i], R, model["mean"][c], model["evec"][c], model["wgt"][c], d2)
            assert m == r["m"][i, s]
            assert abs(e - np.exp(r["x"][i, s])) <= nd.EXP_ULPS * np.spacing(np.exp(r["x"][i, s]))
            assert live == (e > 0.0)
            one = np.full((1, 7), -1, np.int32)
            one[0, s] = c
            _, _, d = nd.terms(r["w"][i:i + 1], model, one, d2)
            Cc, lv = nd.contributions(x26, scan[i:i + 1], model, one, d, np.full((1, 7), e), d2)
            want = (Cc[0, s, 0] + Cc[0, s, 1]) + Cc[0, s, 2]      # (from +0.0, k ascending)
            assert bool(lv[0, s]) == live and sums.tobytes() == (want + 0.0).tobytes()
            seen += 1
        if d2 == 1e6:
            assert not np.any(r["live"][r["m"] > 1e-2]) and np.all(np.isfinite(r["C"]))
    assert seen > 50


def test_the_shape_in_numpy_is_the_shape_in_plain_floats_and_meets_fsum(scene):
    model, scan = scene["models"][1], scene["scan"][:257]
    r = nd.restate(sl.start_poses(((0.1, 0.1, 1),))[0], scan, model, 7, api.ndt_params(OUTLIER, 1.0)[1])
    assert r["cells"] > 300
    a, b = nd.shape_sums(r["C"]), nd.shape_sums_plain(r["C"])
    assert a.tobytes() == b.tobytes()
    S, A, n = nd.fsum_sums(r["C"])
    assert np.all(np.abs(a - S) <= sl.sum_bound(n, A))
    H = api.sym6(a[:21])
    assert np.all(np.linalg.eigvalsh(H) >= -sl.sum_bound(n, A[:21].max())), "H is positive semidefinite"


def test_g_is_the_gradient_of_minus_score(scene):
    """Central differences of F = -sum e over the body-frame perturbation, the cells held, w moved in float64 (the float32 rounding
    of w is a property of the call, not of the derivative).  With L = max d2 * w_k * |d_k| * (1 + |p|) the rate at which an exponent
    moves per unit step, the step is h = 1e-3 / L; a central difference is then off by at most (h L)^2 = 1e-6 of the terms' absolute
    sum (third derivatives of exp(c m): at most a few L^3 each, over 6) plus the rounding 8 eps * sum e / h of the two scores."""
    model, scan = scene["models"][1], scene["scan"]
    d2 = api.ndt_params(OUTLIER, 1.0)[1]
    x26 = sl.start_poses(((0.05, -0.05, 0.5),))[0]
    M = sf.pose_rt(x26).astype(np.float64)
    R, t = M[:, :3], M[:, 3]
    p = scan.astype(np.float64)
    cell = nd.lookup(sf.world_points(x26, scan), model["leaf"], model["ijk"], 7)

    def world(xi):
        th = float(np.linalg.norm(xi[3:]))
        K = np.array([[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]])
        E = np.eye(3) + (math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K if th > 0 else 0)
        return (p @ E.T + xi[:3]) @ R.T + t

    def score(xi):
        _, x, _ = nd.terms(world(xi), model, cell, d2)
        return math.fsum(np.exp(x[cell >= 0]))
    w0 = world(np.zeros(6))
    m, x, d = nd.terms(w0, model, cell, d2)
    Cc, live = nd.contributions(x26, scan, model, cell, d, np.exp(x), d2)
    S, A, _ = nd.fsum_sums(Cc)
    at = np.where(cell >= 0, cell, 0)
    L = float(np.max(np.where((cell >= 0)[:, :, None], d2 * model["wgt"][at] * np.abs(d), 0.0) * (1 + np.abs(p).max())))
    h = 1e-3 / L
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        fd = -(score(e) - score(-e)) / (2 * h)
        assert abs(fd - S[21 + a]) <= 1e-6 * A[21 + a] + 8 * 2.0 ** -52 * S[27] / h, (a, fd, S[21 + a])
    assert live.sum() > 1000 and np.abs(S[21:27]).max() > 1.0


def test_the_restatement_converges_from_the_kept_starts_to_the_recorded_end(scene):
    x = nd.gauss_newton(sl.start_poses(CPU_STARTS), scene["scan"], scene["models"], outlier_ratio=OUTLIER)
    errs = np.array([sl.pose_error(r) for r in x])
    print("restatement ends", errs.tolist())
    assert errs[:, 0].max() <= REF_END[0] * 1.01 and errs[:, 1].max() <= REF_END[1] * 1.01
    assert errs[:, 0].max() >= REF_END[0] * 0.99 and errs[:, 1].max() >= REF_END[1] * 0.99, "REF_END is the measured worst, not a loose cap"


# ---- the bindings, on a recording stand-in for the libraries (test_bindings_host.py's) ----
from test_bindings_host import _hip_ctx, _localizer, _shape      # noqa: E402

_NDT_CASES = [
    ("ndt_build", "flimo_ndt_build", "flimo_loc_ndt_build", (0, 1.0), {}, "int"),
    ("ndt_info", "flimo_ndt_info", "flimo_loc_ndt_info", (1,), {},
     dict(cells="int", map_size_at_build="int", eig_ratio="float", leaf="float", min_pts="int", stale="int")),
    ("ndt_cells", "flimo_ndt_cells", "flimo_loc_ndt_cells", (2,), {},
     dict(ijk="int32:2", count="int32:1", mean="float64:2", evec="float64:3", wgt="float64:2", eval="float64:2", nc="int")),
    ("ndt_clear", "flimo_ndt_clear", "flimo_loc_ndt_clear", (), {}, "NoneType"),
    ("scan_ndt", "flimo_scan_ndt", "flimo_loc_scan_ndt", (0, np.zeros((2, 26)), 1.0), {},
     dict(valid="int32:1", cells="int64:1", H="float64:2", g="float64:2", score="float64:1")),
    ("scan_ndt", "flimo_scan_ndt", "flimo_loc_scan_ndt", (0, np.zeros((2, 26)), 1.0), dict(hood=1, want_terms=True),
     dict(valid="int32:1", cells="int64:1", H="float64:2", g="float64:2", score="float64:1", terms="float64:4", term_cell="int32:3")),
]


@pytest.mark.parametrize("case", _NDT_CASES, ids=[c[0] + ("-terms" if c[4] else "") for c in _NDT_CASES])
def test_the_ndt_methods_are_shared_and_call_their_symbols(case):
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


def test_the_ndt_rows_are_declared_on_both_libraries(built):
    L, H = _lib.load_hip(), api.load_host()
    assert len(_abi.PAIRED_NDT) == 5
    for hip, loc, args in _abi.PAIRED_NDT:
        assert list(getattr(L, hip).argtypes[1:]) == list(getattr(H, loc).argtypes[1:]) == list(args), hip
        assert _abi.LOC_OF[hip] == loc
    assert L.flimo_set_ndt_chunk.argtypes is not None and L.flimo_ndt_term_host.argtypes is not None


from test_corr_graph_host import canned      # noqa: E402,F401  (relocalize's stages replaced by recorders)


def test_relocalize_ends_in_ndt_align_only_when_asked(canned, monkeypatch):      # noqa: F811
    map_obj, scan_obj, log, qi, rj = canned
    calls = []

    def ndt_align(obj, x, **kw):
        calls.append((obj, np.array(x), kw))
        return dict(x26=np.array(x) + 1.0)
    monkeypatch.setattr(api, "ndt_align", ndt_align)
    plain = api.relocalize(map_obj, scan_obj, nh=64)      # the default stays point-to-plane
    assert calls == [] and np.array_equal(plain["x26"], plain["fitness"]["x26"][0])
    out = api.relocalize(map_obj, scan_obj, nh=64, refine="ndt", ndt=dict(slots=(0, 1, 2), hood=1))
    assert len(calls) == 1 and calls[0][0] is map_obj and calls[0][2] == dict(slots=(0, 1, 2), hood=1)
    assert np.array_equal(calls[0][1], out["fitness"]["x26"][:1]) and np.array_equal(out["x26"], out["fitness"]["x26"][0] + 1.0)
    with pytest.raises(ValueError, match="refine"):
        api.relocalize(map_obj, scan_obj, refine="icp")


def test_ndt_align_runs_scan_align_once_per_slot_at_that_leafs_d2(monkeypatch):
    class Obj:
        def __init__(self):
            self.calls = []

        def ndt_info(self, slot):
            return dict(leaf=(2.0, 1.0, 0.5)[slot])

        def scan_ndt(self, slot, xs, d2, hood=7):
            self.calls.append((slot, d2, hood, len(xs)))
            m = len(xs)
            H = np.zeros((m, 21))
            H[:, [0, 6, 11, 15, 18, 20]] = 1.0      # the identity
            return dict(valid=np.full(m, 100, np.int32), cells=np.zeros(m, np.int64), H=H, g=np.zeros((m, 6)), score=np.full(m, 3.0))
    obj = Obj()
    x = np.zeros((2, 26))
    x[:, 6] = 1.0
    out = api.ndt_align(obj, x, (0, 1, 2), hood=1, iters=2)
    assert [c[0] for c in obj.calls] == [0, 0, 1, 1, 2, 2] and all(c[2:] == (1, 2) for c in obj.calls)
    assert [c[1] for c in obj.calls[::2]] == [api.ndt_params(0.55, leaf)[1] for leaf in (2.0, 1.0, 0.5)]
    assert len(out["stages"]) == 3 and np.all(out["cost"] == -3.0) and np.array_equal(out["x26"], x)
    with pytest.raises(ValueError, match="no slots"):
        api.ndt_align(obj, x, ())
