"""CPU tests: the host twins of the filter's device algebra (flimo_ieskf.h compiled for the host, the host filter's own
elimination, flimo_host::Esekf) against the mpmath reference of tests/ieskf_common.py, on the inputs the GPU tests use
(tests/test_gpu_ieskf.py).  This is where the error constants K_HOST are measured: every test prints its worst error in units of
the scale ieskf_common derives, then asserts it at four times the recorded value."""
import numpy as np
import pytest

import ieskf_common as C


def _host(op, items):
    from fast_limo_amd import _lib
    return _lib.ieskf_eval_host(op, items)


@pytest.mark.parametrize("name", list(C.HELPERS))
def test_host_helper_against_mpmath(built, name):
    op, inputs = C.HELPERS[name][0], C.HELPERS[name][1]()
    out, _ = _host(op, inputs)
    worst, k = C.helper_units(name, out)
    print(f"ieskf host {name}: {worst:.3f} units at item {k} {inputs[k]} (recorded {C.K_HOST[name]})")
    assert worst <= 4.0 * C.K_HOST[name], (worst, k, inputs[k], out[k])


@pytest.mark.parametrize("name", list(C.HELPERS))
def test_every_branch_of_a_helper_is_reached_ten_times(built, name):
    """What the deskew's coverage check does for the front end: the branch each input takes, as the host evaluation reports it."""
    _, br = _host(C.HELPERS[name][0], C.HELPERS[name][1]())
    for mask, value in C.BRANCHES[name]:
        assert int(np.sum((br & mask) == value)) >= 10, (name, mask, value, np.bincount(br))


def test_branch_codes_agree_with_the_reference(built):
    """... and the reference takes the same branches on these inputs (none sits where a last bit decides)."""
    _, br = _host(5, C.in_s2_boxminus())
    ref = [C.mp_s2_boxminus(C.vec(p[0:3]), C.vec(p[3:6]))[1] + 4 * C.mp_s2_chart(C.vec(p[3:6])) for p in C.in_s2_boxminus()]
    assert list(br) == ref
    _, br = _host(4, C.in_s2_Bx())
    assert list(br) == [C.mp_s2_chart(C.vec(g)) for g in C.in_s2_Bx()]
    _, br = _host(1, C.in_A_T())
    assert list(br) == [int(C.mp_norm(C.vec(v)) < C.TOL) for v in C.in_A_T()]
    _, br = _host(3, C.in_cos_sinc_sqrt())
    assert list(br) == [int(not C.mp.mpf(float(a[0])) >= C.TAYLOR_N_BOUND) for a in C.in_cos_sinc_sqrt()]


def test_antipodal_and_equal_pairs_give_the_literals(built):
    pairs = C.in_s2_boxminus()
    out, br = _host(5, pairs)
    assert np.all(out[(br & 3) == 2] == [3.1415926, 0.0]) and np.all(out[(br & 3) == 1] == 0.0)


# ---- Gauss-Jordan ----
def _gj_items(solve):
    T = np.array([t.reshape(-1) for _, t in C.gj_systems()])
    return np.concatenate([T, C.gj_rhs()], axis=1) if solve else T


def test_host_gauss_jordan_twins_take_the_stated_steps(built):
    """ik_inverse_gj12_serial, the host filter's inverse_gj and solve_gj, and a plain float64 elimination by the stated rule
    (largest magnitude among the unused rows, the lowest row among equals) agree bit for bit; a zero pivot is reported at
    every step it can occur at; and on the tied systems the other tie rule gives other bits (the comparison can tell)."""
    from fast_limo_amd import _lib, api
    ser, _ = _host(_lib.IK_GJ12_INVERSE, _gj_items(False))
    inv = api.ieskf_gj12_host(_lib.IK_GJ12_INVERSE, _gj_items(False))
    sol = api.ieskf_gj12_host(_lib.IK_GJ12_SOLVE, _gj_items(True))
    other_rule_differs = {"tie2": 0, "tie3": 0, "tie_pm": 0}
    for i, ((kind, T), v) in enumerate(zip(C.gj_systems(), C.gj_rhs())):
        X, u, ok, tied = C.gj_plain(T, v)
        assert ser[i, 144] == inv[i, 144] == sol[i, 12] == float(ok), (i, kind)
        assert ok == (not kind.startswith("zero")), (i, kind)
        if not ok:
            continue
        assert tied == kind.startswith("tie"), (i, kind)
        assert ser[i, :144].tobytes() == X.tobytes() == inv[i, :144].tobytes(), (i, kind)
        assert sol[i, :12].tobytes() == u.tobytes(), (i, kind)
        if tied:
            Xh, uh, _, _ = C.gj_plain(T, v, highest=True)
            other_rule_differs[kind] += int(Xh.tobytes() != X.tobytes() and uh.tobytes() != u.tobytes())
    assert all(n >= 5 for n in other_rule_differs.values()), other_rule_differs


def test_host_gauss_jordan_against_mpmath(built):
    from fast_limo_amd import _lib, api
    ser, _ = _host(_lib.IK_GJ12_INVERSE, _gj_items(False))
    sol = api.ieskf_gj12_host(_lib.IK_GJ12_SOLVE, _gj_items(True))
    wi, ws = C.gj_units(ser, sol)
    print(f"ieskf host gj_inverse: {wi:.3f} units, gj_solve: {ws:.3f} units (recorded {C.K_HOST['gj_inverse']}, {C.K_HOST['gj_solve']})")
    assert wi <= 4.0 * C.K_HOST["gj_inverse"] and ws <= 4.0 * C.K_HOST["gj_solve"]


# ---- the measurement-independent half ----
def test_host_pre_half_against_mpmath(built):
    from fast_limo_amd import _lib
    out, _ = _host(_lib.IK_PRE, np.array([it for _, it in C.pre_cases()]))
    w = C.pre_units(out)
    print("ieskf host pre: " + ", ".join(f"{k} {v[0]:.3f} units at {v[1]}" for k, v in w.items()), {k: C.K_HOST[k] for k in w})
    for k, (units, where) in w.items():
        assert units <= 4.0 * C.K_HOST[k], (k, units, where)


# ---- the whole algebra ----
@pytest.mark.parametrize("case", list(C.algebra_cases()))
def test_host_filter_iterations_against_mpmath(built, case):
    """flimo_host::Esekf on fixed per-iteration sums: every logged pass against one outer iteration of the reference in its
    literal two-inverse form, from the state the host itself was at; the ladder's rungs are reached."""
    c = C.algebra_cases()[case]
    h = C.host_run(case)
    assert h["passes"] == len(h["log"]) >= 2
    w = C.iteration_units(c, h["log"])
    print(f"ieskf host iterations {case}: dx {w[0]:.3f} units, x_after {w[1]:.3f} units (recorded {C.K_HOST['iter_dx']}, {C.K_HOST['iter_x']})")
    assert w[0] <= 4.0 * C.K_HOST["iter_dx"] and w[1] <= 4.0 * C.K_HOST["iter_x"]
    if c.get("rungs"):
        C.assert_rungs_reached(c, h["log"])


def test_host_loop_counts_a_step_on_its_limit_as_within_it(built):
    """The host loop's own counter t, pass by pass (esekfom.hpp:1749-1764: `>` a limit is over, two passes within end the loop)."""
    t = {name: [p["t"] for p in C._host_of(c)["log"]] for name, c in C.loop_cases().items()}
    assert t == {"t2_early": [1, 2], "limit_on": [1, 1, 1, 1, 1], "limit_one_ulp_above": [0] * 5, "ends_at_max_iter": [0] * 5}


@pytest.mark.parametrize("who", ["host", "oracle"])
def test_filter_from_dense_rows_on_a_general_state_against_mpmath(built, oracle, who):
    """The oracle's eskf_update_fixed applies where dense rows reproduce the sums: one set for every iteration.  The rows are
    dyadic, so their sums are exact whoever adds them; the filter is run with max_iters = 0, 1, .. and the state after every
    pass is held against one iteration of the reference from the filter's own state before it -- the quantity, the scale and
    the constant of the per-iteration tests above."""
    from fast_limo_amd import api
    u = C.passes_from_rows_units(api.eskf_update_fixed if who == "host" else oracle.eskf_update_fixed)
    print(f"ieskf {who} from dense rows: x_after {u:.3f} units (recorded {C.K_HOST['iter_x']})")
    assert u <= 4.0 * C.K_HOST["iter_x"], (who, u)
