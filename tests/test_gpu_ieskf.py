"""GPU tests: the filter's device algebra (csrc/hip/flimo_ieskf.h) away from the identity state -- its helpers, the one-wave
Gauss-Jordan routines, ik_pre_block and the whole algebra on fixed sums (the two one-workgroup launches of flimo_ieskf.hip), each
against its host twin and against the mpmath reference of tests/ieskf_common.py, which is written from the reference
implementation's own files.  No scene, no map, no search: nothing here waits for another workgroup, and no comparison hangs on a
discrete decision.  Bounds: bit equality where no transcendental function is involved, the existing 1e-13 for the near-identity
baseline, and otherwise the host twin's measured error (ieskf_common.K_HOST, in units of a derived scale) times four against
mpmath and times eight between device and host.  Every test prints what it measured."""
import numpy as np
import pytest

import ieskf_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built):
    from fast_limo_amd import _lib
    c = _lib.HipCtx(0)
    yield c
    c.close()


def _gj_items(solve):
    T = np.array([t.reshape(-1) for _, t in C.gj_systems()])
    return np.concatenate([T, C.gj_rhs()], axis=1) if solve else T


# ---- helpers ----
@pytest.mark.parametrize("name", list(C.HELPERS))
def test_device_helper_against_host_twin_and_mpmath(ctx, name):
    from fast_limo_amd import _lib
    op, inputs = C.HELPERS[name][0], C.HELPERS[name][1]()
    dev = ctx.ieskf_eval(op, inputs)
    host, br = _lib.ieskf_eval_host(op, inputs)
    for mask, value in C.BRANCHES[name]:
        assert int(np.sum((br & mask) == value)) >= 10, (name, mask, value)
    worst, k = C.helper_units(name, dev)
    between = C.units_between(name, dev, host)
    print(f"ieskf device {name}: {worst:.3f} units against mpmath at item {k}, {between:.3f} against the host twin (host: {C.K_HOST[name]})")
    assert worst <= 4.0 * C.K_HOST[name], (worst, k, inputs[k], dev[k], host[k])
    assert between <= 8.0 * C.K_HOST[name]
    if name in ("s2_Bx",):                                  # no transcendental function: the same bits
        assert dev.tobytes() == host.tobytes()


# ---- Gauss-Jordan on one wave ----
def test_wave_gauss_jordan_takes_the_hosts_steps_bit_for_bit(ctx):
    """flimo_ieskf.h: "the steps of the host's inverse_gj, element for element" -- SPD systems up to cond 1e12, (signed)
    permutations, pivot ties of two and three rows and of opposite signs met at several steps, negative pivots, a pivot order
    that reverses the rows; a zero column at step 0, 5 and 11 is reported and the call returns."""
    from fast_limo_amd import _lib, api
    dev_i = ctx.ieskf_eval(_lib.IK_GJ12_INVERSE, _gj_items(False))
    dev_s = ctx.ieskf_eval(_lib.IK_GJ12_SOLVE, _gj_items(True))
    ser, _ = _lib.ieskf_eval_host(_lib.IK_GJ12_INVERSE, _gj_items(False))
    hst_i = api.ieskf_gj12_host(_lib.IK_GJ12_INVERSE, _gj_items(False))
    hst_s = api.ieskf_gj12_host(_lib.IK_GJ12_SOLVE, _gj_items(True))
    kinds = [k for k, _ in C.gj_systems()]
    for i, kind in enumerate(kinds):
        ok = not kind.startswith("zero")
        assert dev_i[i, 144] == dev_s[i, 12] == ser[i, 144] == hst_i[i, 144] == hst_s[i, 12] == float(ok), (i, kind)
        if ok:                                              # (nothing is read from the outputs of a system with a zero pivot)
            assert dev_i[i, :144].tobytes() == ser[i, :144].tobytes() == hst_i[i, :144].tobytes(), (i, kind)
            assert dev_s[i, :12].tobytes() == hst_s[i, :12].tobytes(), (i, kind)
    wi, ws = C.gj_units(dev_i, dev_s)
    print(f"ieskf device gj_inverse: {wi:.3f} units, gj_solve: {ws:.3f} units against mpmath (host: {C.K_HOST['gj_inverse']}, {C.K_HOST['gj_solve']})")
    assert wi <= 4.0 * C.K_HOST["gj_inverse"] and ws <= 4.0 * C.K_HOST["gj_solve"]


# ---- the measurement-independent half ----
def test_pre_block_against_serial_twin_and_mpmath(ctx):
    """ik_pre_block at general states and covariances with x a rung of the ladder from x_prop; with x == x_prop it equals
    ik_pre_serial bit for bit -- what flimo_update_chain rests on when it forms iteration -1's half on the host."""
    from fast_limo_amd import _lib
    items = np.array([it for _, it in C.pre_cases()])
    dev = ctx.ieskf_eval(_lib.IK_PRE, items)
    host, _ = _lib.ieskf_eval_host(_lib.IK_PRE, items)
    w = C.pre_units(dev)
    same = 0
    btw = {"pre_dxn": 0.0, "pre_AI": 0.0, "pre_G2": 0.0}
    for i, (name, it) in enumerate(C.pre_cases()):
        if np.array_equal(it[0:26], it[26:52]):
            assert dev[i].tobytes() == host[i].tobytes(), name
            same += 1
        for key, sl, sc in zip(btw, (slice(0, 23), slice(23, 167), slice(167, 299)), C.pre_scales(i)):
            btw[key] = max(btw[key], float(np.max(np.abs(dev[i, sl] - host[i, sl]))) / sc)
    assert same >= 12
    print("ieskf device pre: " + ", ".join(f"{k} {v[0]:.3f} units at {v[1]} ({btw[k]:.3f} against the host twin)" for k, v in w.items()))
    for k, (units, where) in w.items():
        assert units <= 4.0 * C.K_HOST[k], (k, units, where)
        assert btw[k] <= 8.0 * C.K_HOST[k], (k, btw[k])


# ---- the whole algebra ----
def _run(ctx, c, **kw):
    return ctx.ieskf_run_fixed(c["x"], c["P"], c["limits"], c["partials"], R=c["R"], D=c["D"], max_iter=c["max_iter"], **kw)


def _check_head_and_sums(c, its, fin):
    """after every iteration that went on: the logged sums are the partials added in slot order, PoseMats is pose_from_x26 of
    the device's own x_after, prev_RT the RT the iteration ran with, status 0; after the hand-back status 2"""
    rt = C.pose_f32(c["x"])[0:16]
    ns = len(c["partials"])
    for i, it in enumerate(its):
        if not it["went_on"]:
            assert i == len(its) - 1 and it["status"] == 2
            break
        HTH, HTh, _ = C.unpack_sums(C.slot_order_sum(c["partials"][min(i, ns - 1)]))
        assert it["HTH"].tobytes() == HTH.tobytes() and it["HTh"].tobytes() == HTh.tobytes(), i
        assert it["status"] == 0 and it["passes"] == i + 1 and it["it"] == i
        assert it["pose"].tobytes() == C.pose_f32(it["x_after"]).tobytes(), i
        assert it["prev_RT"].tobytes() == rt.tobytes(), i
        rt = it["pose"][0:16]
    assert fin["status"] == 2 and not its[-1]["went_on"]
    assert fin["sums"].tobytes() == C.slot_order_sum(c["partials"][min(len(its) - 1, ns - 1)]).tobytes()


def _check_loop_against_host(c, its, fin, h):
    """the chain hands back at the iteration whose covariance update is due: reason 5, and passes, it, t as the host loop has
    them there; the handed-back state is the one that iteration measured at"""
    n = len(h["log"])
    assert (fin["reason"], fin["passes"], fin["it"]) == (5, n - 1, n - 2) and len(its) == n
    assert fin["t"] == (h["log"][n - 2]["t"] if n >= 2 else 0)          # the host loop's own count before the pass handed back
    assert fin["x"].tobytes() == (its[n - 2]["x_after"] if n >= 2 else c["x"]).tobytes()
    assert np.all(fin["passinfo"][:n, 0] == [p["M"] for p in h["log"]])


@pytest.mark.parametrize("case", list(C.algebra_cases()))
def test_whole_algebra_against_host_filter_and_mpmath(ctx, case):
    """The two launches per iteration on fixed sums, at every state x covariance of ieskf_common.algebra_cases(): each pass's dx
    and x_after against the host filter's log and against one iteration of the reference from the device's own state; sums,
    head, loop variables and the half each iteration's first launch leaves, bit for bit."""
    c = C.algebra_cases()[case]
    h = C.host_run(case)
    its, fin = _run(ctx, c)
    _check_head_and_sums(c, its, fin)
    _check_loop_against_host(c, its, fin, h)
    log = [it for it in its if it["went_on"]]
    if c["rungs"]:
        C.assert_rungs_reached(c, h["log"])
        C.assert_rungs_reached(c, log)
    if case == "tool/tool/baseline":
        for a, b in zip(log, h["log"]):
            np.testing.assert_allclose(a["dx"], b["dx"], rtol=0, atol=1e-13)
            np.testing.assert_allclose(a["x_after"], b["x_after"], rtol=0, atol=1e-13)
    wd, wx, bd, bx = C.iteration_units2(c, log, h["log"])
    print(f"ieskf device iterations {case}: dx {wd:.3f}, x_after {wx:.3f} units against mpmath; {bd:.3f}, {bx:.3f} against the host filter "
          f"(host: {C.K_HOST['iter_dx']}, {C.K_HOST['iter_x']})")
    assert wd <= 4.0 * C.K_HOST["iter_dx"] and wx <= 4.0 * C.K_HOST["iter_x"]
    assert bd <= 8.0 * C.K_HOST["iter_dx"] and bx <= 8.0 * C.K_HOST["iter_x"]
    # the first launch of iteration i + 1 leaves the half ik_pre_block forms from the state iteration i left
    from fast_limo_amd import _lib
    for i in range(1, len(its)):
        item = np.concatenate([its[i - 1]["x_after"], c["x"], c["P"].reshape(-1), [c["R"]]])
        pre = ctx.ieskf_eval(_lib.IK_PRE, item[None, :])[0]
        assert its[i]["pre_dxn"].tobytes() == pre[0:23].tobytes() and its[i]["pre_AG"].tobytes() == pre[23:299].tobytes(), i


@pytest.mark.parametrize("case", ["t2_early", "limit_on", "limit_one_ulp_above", "ends_at_max_iter"])
def test_loop_logic(ctx, case):
    """a component of dx exactly on its limit does not count as over, one ulp above it does; t reaches 2 before max_iter; the
    loop ends at it == max_iter - 1"""
    c = C.loop_cases()[case]
    h = C._host_of(c)
    its, fin = _run(ctx, c)
    _check_head_and_sums(c, its, fin)
    _check_loop_against_host(c, its, fin, h)
    assert its[0]["dx"].tobytes() == h["log"][0]["dx"].tobytes()          # x == x_prop: no transcendental in the first step
    want = {"t2_early": (2, 1), "limit_on": (5, 1), "limit_one_ulp_above": (5, 0), "ends_at_max_iter": (5, 0)}[case]
    assert (len(h["log"]), fin["t"]) == want


def test_hand_backs(ctx):
    H = C.handback_cases()
    # M = 22 in iteration 0, and in iteration 2 only: reason 1, the state before that iteration, the input's sums
    its, fin = _run(ctx, H["few_at_0"])
    assert (fin["reason"], fin["passes"], fin["it"], fin["t"], len(its)) == (1, 0, -1, 0, 1)
    assert fin["x"].tobytes() == H["few_at_0"]["x"].tobytes() and fin["passinfo"][0, 0] == 22
    _check_head_and_sums(H["few_at_0"], its, fin)
    c = H["few_at_2"]
    h = C._host_of(c)
    its, fin = _run(ctx, c)
    assert (fin["reason"], fin["passes"], fin["it"], len(its)) == (1, 2, 1, 3)
    assert fin["x"].tobytes() == its[1]["x_after"].tobytes()
    _check_head_and_sums(c, its, fin)
    _, _, bd, bx = C.iteration_units2(c, its[:2], h["log"][:2])
    assert bd <= 8.0 * C.K_HOST["iter_dx"] and bx <= 8.0 * C.K_HOST["iter_x"]
    # the smallest eigenvalue of H^T H's pose block below and above D
    its, fin = _run(ctx, H["eig_0.9D"])
    assert (fin["reason"], fin["passes"], len(its)) == (3, 0, 1)
    _check_head_and_sums(H["eig_0.9D"], its, fin)
    its, fin = _run(ctx, H["eig_1.1D"])
    assert fin["reason"] == 5 and fin["passes"] == 3 and all(it["went_on"] for it in its[:3])
    # a zero pivot: P with a zero row and column, H^T H with the same column zero
    its, fin = _run(ctx, H["zero_pivot"])
    assert (fin["reason"], fin["passes"], len(its)) == (3, 0, 1)
    assert np.all(np.isfinite(fin["x"])) and fin["x"].tobytes() == H["zero_pivot"]["x"].tobytes()
    # sums that carry another pass's number
    its, fin = _run(ctx, H["bad_tags"], tag_ok=[0])
    assert (fin["reason"], fin["passes"], len(its)) == (4, 0, 1) and its[0]["status"] == 2


def test_same_call_from_fresh_contexts_gives_the_same_bytes(built):
    from fast_limo_amd import _lib
    c = C.algebra_cases()["general/corr/ladder11"]
    got = []
    for _ in range(2):
        k = _lib.HipCtx(0)
        its, fin = _run(k, c)
        helpers = k.ieskf_eval(_lib.IK_S2_J, C.in_s2_J())
        k.close()
        got.append(b"".join(np.concatenate([v.reshape(-1).astype(np.float64) for v in it.values() if isinstance(v, np.ndarray)]).tobytes()
                            for it in its) + fin["x"].tobytes() + fin["sums"].tobytes() + helpers.tobytes())
    assert got[0] == got[1]
