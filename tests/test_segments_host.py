"""CPU suite: map segments as far as they can be checked without a device -- the move on the host (flimo_seg_move_host: the
function the kernel calls) against the numpy restatement and against hand values, api.segment_corrections against T_new T_old^-1
formed on its own, api.pose_graph_solve on graphs whose answer is known, and the new symbols in the headers and the tables."""
import math
import os
import re

import numpy as np
import pytest

import segments_common as sg
from fast_limo_amd import _abi, _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the move ------------------------------------------------------------------------------------------------------------------
def test_seg_find_is_the_largest_start_not_beyond_the_index():
    begin = [0, 0, 3, 3, 3, 10]                      # segments 0, 2 and 3 are empty
    assert sg.seg_find(begin, [0, 1, 2, 3, 9, 10, 11]).tolist() == [1, 1, 1, 4, 4, 5, 5]
    assert sg.seg_find([0], [0, 5]).tolist() == [0, 0]


def test_the_host_move_is_the_restatement_bit_for_bit(built):
    rng = np.random.default_rng(11)
    mats = [sg.IDENTITY, sg.rigid((3.0, -2.0, 40.0), (1.5, -0.25, 0.125)), sg.rigid((0.01, 0.02, -0.03), (1e4, -1e4, 3.0)),
            rng.normal(0, 1, 12), rng.normal(0, 1e3, 12), np.array([1e-30, 1e30, -1e30, 1.0] * 3)]
    pts = np.concatenate([rng.uniform(-50, 50, (64, 3)), rng.normal(0, 1e4, (32, 3)), rng.normal(0, 1e-20, (8, 3)),
                          [[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [3.4e38, -3.4e38, 1.0], [1e-45, -1e-45, 0.0]]]).astype(F)
    for T in mats:
        want = sg.seg_move(np.tile(T, (len(pts), 1)), pts)
        got = np.array([api.seg_move_host(T, p) for p in pts])
        assert _bits(got).tobytes() == _bits(want).tobytes()


def test_the_host_move_by_hand(built):
    T = [2, 0, 0, 1, 0, 3, 0, -1, 0, 0, 0.5, 0.25]
    assert api.seg_move_host(T, [1, 2, 4]).tolist() == [3.0, 5.0, 2.25]
    # float64 holds 1 + 2^-30, float32 does not: one rounding at the end
    assert api.seg_move_host([1, 0, 0, 2.0 ** -30] + [0] * 8, [1, 0, 0])[0] == F(1.0)
    assert api.seg_move_host([1, 0, 0, 2.0 ** -23] + [0] * 8, [1, 0, 0])[0] == F(1.0) + F(2.0 ** -23)
    # the sum is formed from the right: 2^60 + 1 is 2^60 in float64, so x = -2^60 leaves 0 where a sum from the left would leave 1
    assert api.seg_move_host([1, 0, 1, 1.0] + [0] * 8, [-2.0 ** 60, 0, 2.0 ** 60])[0] == F(0.0)
    assert api.seg_move_host([1, 0, 1, 1.0] + [0] * 8, [2.0 ** 60, 0, -2.0 ** 60])[0] == F(0.0)
    # identity: every component goes through "+ 0.0" and comes back, except -0.0, which becomes +0.0
    out = api.seg_move_host(sg.IDENTITY, F([-0.0, 5.5, 0.0]))
    assert _bits(out).tolist() == _bits(F([0.0, 5.5, 0.0])).tolist() and _bits(out)[0] != _bits(F([-0.0]))[0]
    # float32 overflow is reported as it is
    assert np.isinf(api.seg_move_host([1e30, 0, 0, 0] + [0] * 8, [1e30, 0, 0])[0])
    L = _lib.load_hip()
    z = np.zeros(12)
    assert L.flimo_seg_move_host(None, z.ctypes.data, z.ctypes.data) == -2


# ---- segment_corrections -------------------------------------------------------------------------------------------------------
def _random_poses(rng, n, spread=30.0):
    return np.array([sg.mat4(synth.rpy_to_R(*rng.uniform(-math.pi, math.pi, 3) * [1, 0.49, 1]), rng.uniform(-spread, spread, 3)) for _ in range(n)])


def test_segment_corrections_are_t_new_times_t_old_inverse():
    try:
        import mpmath
    except ImportError:
        mpmath = None
    rng = np.random.default_rng(5)
    old, new = _random_poses(rng, 12), _random_poses(rng, 12)
    xo, xn = np.array([sg.x26_of(M) for M in old]), np.array([sg.x26_of(M) for M in new])
    xo[:, 3:7] *= 1.7                                 # (rot is normalised before it is used)
    xo[:, 7:] = rng.normal(0, 1, (12, 19))            # (nothing but pos and rot is read)
    got = api.segment_corrections(xo, xn)
    assert got.shape == (12, 12) and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    for s in range(12):
        A, B = sg.mat_of_x26(xo[s]), sg.mat_of_x26(xn[s])       # built on their own, from the same rows
        if mpmath is not None:
            mpmath.mp.dps = 50
            want = np.array((mpmath.matrix(B.tolist()) * mpmath.matrix(A.tolist()) ** -1).tolist(), dtype=np.float64)
        else:
            want = B @ np.linalg.inv(A)
        # entries of R are below 1 and of t below 100 here: 1e-12 is thousands of float64 roundings of either
        np.testing.assert_allclose(got[s].reshape(3, 4), want[:3], rtol=0, atol=1e-12)
    # the same pose before and after: the identity to within the rounding of R R^T, and it moves a point by less than a float32 ulp
    same = api.segment_corrections(xn, xn)
    np.testing.assert_allclose(same, np.tile(sg.IDENTITY, (12, 1)), rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        api.segment_corrections(xo, xn[:5])


# ---- pose_graph_solve ----------------------------------------------------------------------------------------------------------
def _x26s(mats):
    return np.array([sg.x26_of(M) for M in mats])


def _pos_err(x26, truth, k):
    return float(np.linalg.norm(x26[k, 0:3] - truth[k][:3, 3]))


def test_the_jacobians_are_the_residuals_derivatives():
    """The normal equations' gradient against central differences of the cost along pose_retract's perturbation."""
    rng = np.random.default_rng(3)
    truth = _random_poses(rng, 5, 5.0)
    edges = [(0, 1, np.linalg.inv(truth[0]) @ truth[1]), (1, 2, np.linalg.inv(truth[1]) @ truth[2], [1, 2, 3, 4, 5, 6]),
             (3, 2, np.linalg.inv(truth[3]) @ truth[2]), (4, 0, np.linalg.inv(truth[4]) @ truth[0]), (1, 4, np.linalg.inv(truth[1]) @ truth[4])]
    x = _x26s(truth)
    for k in range(5):
        x[k] = api.pose_retract(x[k], rng.normal(0, 0.2, 6))

    def cost(x):
        E = api._pg_edges(edges, 5)
        return sum(float(np.dot(w, r * r)) for (_, _, _, w), (r, _, _, _) in zip(E, api.pose_graph_residuals(api._pose_mats(x), E)))

    # one step of length zero cannot be asked for; the gradient the solver starts from is what it reports first
    g0 = api.pose_graph_solve(x, edges, fixed=0, iters=0)["grad"][0]
    num, h = [], 1e-6
    for k in range(1, 5):
        for a in range(6):
            e = np.zeros(6)
            e[a] = h
            xp, xm = np.array(x), np.array(x)
            xp[k], xm[k] = api.pose_retract(x[k], e), api.pose_retract(x[k], -e)
            num.append((cost(xp) - cost(xm)) / (2 * h))
    # the solver's g is J^T W r, half the cost's gradient
    assert abs(0.5 * np.linalg.norm(num) - g0) <= 1e-6 * g0


def test_a_consistent_graph_comes_back_to_the_truth():
    rng = np.random.default_rng(8)
    truth = _random_poses(rng, 8, 10.0)
    pairs = [(k, k + 1) for k in range(7)] + [(7, 0), (2, 6), (5, 1)]
    edges = [(i, j, np.linalg.inv(truth[i]) @ truth[j]) for i, j in pairs]
    x0 = _x26s(truth)
    for k in range(1, 8):
        x0[k] = api.pose_retract(x0[k], np.concatenate([rng.normal(0, 0.1, 3), rng.normal(0, math.radians(2.0), 3)]))
    x0[:, 7:] = rng.normal(0, 1, (8, 19))
    sol = api.pose_graph_solve(x0, edges, fixed=0)
    print("consistent graph: %d steps, cost %.3e -> %.3e, gradient %.3e -> %.3e" % (sol["iters"], sol["cost"][0], sol["cost"][-1],
                                                                                   sol["grad"][0], sol["grad"][-1]))
    for k in range(8):
        np.testing.assert_allclose(sg.mat_of_x26(sol["x26"][k]), truth[k], rtol=0, atol=1e-9)
    assert sol["grad"][-1] < 1e-8 * sol["grad"][0]
    assert np.all(np.diff(sol["cost"]) <= 0.0)
    assert sol["x26"][:, 7:].tobytes() == x0[:, 7:].tobytes() and sol["x26"][0].tobytes() == x0[0].tobytes()
    # another node held: the same shape, moved rigidly so that node 3 stays where the start put it
    sol3 = api.pose_graph_solve(x0, edges, fixed=3)
    assert sol3["x26"][3].tobytes() == x0[3].tobytes()
    rel = np.linalg.inv(sg.mat_of_x26(sol3["x26"][3])) @ sg.mat_of_x26(sol3["x26"][6])
    np.testing.assert_allclose(rel, np.linalg.inv(truth[3]) @ truth[6], rtol=0, atol=1e-9)


@pytest.mark.parametrize("err_t,err_deg", [(0.02, 0.1), (0.05, 0.3)])
def test_a_loop_edge_pulls_the_end_of_the_ring_back(err_t, err_deg):
    truth, drift, edges = sg.ring_case(24, 10.0, err_t, err_deg)
    x0 = _x26s(drift)
    sol = api.pose_graph_solve(x0, edges, fixed=0)
    before, after = _pos_err(x0, truth, 23), _pos_err(sol["x26"], truth, 23)
    mid_b, mid_a = _pos_err(x0, truth, 12), _pos_err(sol["x26"], truth, 12)
    print("ring %.2f m / %.1f deg: loop end %.4f -> %.4f m (ratio %.4f), mid loop %.4f -> %.4f m, %d steps, gradient %.2e -> %.2e"
          % (err_t, err_deg, before, after, after / before, mid_b, mid_a, sol["iters"], sol["grad"][0], sol["grad"][-1]))
    assert np.all(np.diff(sol["cost"]) <= 0.0)
    assert after <= 0.1 * before


def test_the_solver_refuses_what_is_no_graph():
    x = _x26s(sg.ring_truth(3))
    with pytest.raises(ValueError):
        api.pose_graph_solve(x, [(0, 3, np.eye(4))])
    with pytest.raises(ValueError):
        api.pose_graph_solve(x, [(1, 1, np.eye(4))])
    with pytest.raises(ValueError):
        api.pose_graph_solve(x, [(0, 1, np.eye(4))], fixed=3)
    sol = api.pose_graph_solve(x, [])
    assert sol["iters"] == 0 and sol["x26"].tobytes() == x.tobytes()


# ---- headers and bindings ------------------------------------------------------------------------------------------------------
HIP_NEW = ["flimo_map_segment_mark", "flimo_map_segments", "flimo_map_segments_reset", "flimo_map_corrected", "flimo_map_correct",
           "flimo_map_transform", "flimo_map_remove_range"]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_new_symbols_are_in_the_headers_and_in_the_tables(built):
    c_h, loc_h, dev_h = _header("flimo_c.h"), _header("flimo_localizer_c.h"), _header("flimo_dev.h")
    assert re.search(r"#define\s+FLIMO_SEG_MAX\s+\(\(size_t\)1\s*<<\s*20\)", c_h)
    assert [row[0] for row in _abi.PAIRED_SEG] == HIP_NEW
    for hip, loc, args in _abi.PAIRED_SEG:
        assert loc == hip.replace("flimo_map_", "flimo_loc_map_")
        assert re.search(r"\bint\s+%s\s*\(" % hip, c_h) and re.search(r"\bint\s+%s\s*\(" % loc, loc_h), hip
        assert hip in _lib.HIP_SYMBOLS and loc in api.HOST_SYMBOLS and _abi.LOC_OF[hip] == loc
    assert all(row in _abi.PAIRED_ALL for row in _abi.PAIRED_SEG) and not any(row in _abi.PAIRED for row in _abi.PAIRED_SEG)
    assert re.search(r"\bint\s+flimo_seg_move_host\s*\(", c_h) and "flimo_seg_move_host" in _lib.HIP_SYMBOLS
    assert re.search(r"\bint\s+flimo_set_segment_plan\s*\(", dev_h) and "flimo_set_segment_plan" in _lib.HIP_SYMBOLS
    L, H = _lib.load_hip(), api.load_host()
    for hip, loc, args in _abi.PAIRED_SEG:
        assert list(getattr(L, hip).argtypes[1:]) == list(getattr(H, loc).argtypes[1:]) == list(args), hip
    for name in ("map_segment_mark", "map_segments", "map_segments_reset", "map_corrected", "map_correct", "map_transform", "map_remove_range"):
        assert getattr(_lib.HipCtx, name) is getattr(api.Localizer, name), name
