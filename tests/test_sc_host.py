"""CPU suite: Scan Context's host entries (flimo_sc_bin_host, flimo_sc_dist_host: the functions the kernels call) against the numpy
restatement (tests/sc_common.py) and against values worked by hand, bit for bit; and the method itself on the restatement alone."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import fpfh_common as fpc
import sc_common as sc
from desc_common import bits, fmaf

F = np.float32
INF = float("inf")


@pytest.fixture(autouse=True)
def feature(built):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    for name in ("flimo_sc_bin_host", "flimo_sc_dist_host"):
        getattr(L, name)


def bins_host(pts, c, frame12=None):
    """flimo_sc_bin_host of every point: the arrays of sc.bins."""
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    p = np.ascontiguousarray(pts, F).reshape(-1, 3)
    k = _lib.sc_cfg(**c)
    f = None if frame12 is None else np.ascontiguousarray(frame12, F).reshape(12)
    ring, sector, h = C.c_int(0), C.c_int(0), C.c_float(0)
    out = (np.zeros(len(p), bool), np.full(len(p), -1, np.int32), np.full(len(p), -1, np.int32), np.zeros(len(p), F))
    for i in range(len(p)):
        rc = L.flimo_sc_bin_host(p.ctypes.data + 12 * i, C.byref(k), None if f is None else f.ctypes.data, C.byref(ring), C.byref(sector), C.byref(h))
        assert rc in (0, 1)
        if rc:
            out[0][i], out[1][i], out[2][i], out[3][i] = True, ring.value, sector.value, h.value
    return out


def same_bins(got, want, tag):
    for name, a, b in zip(("has", "ring", "sector"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=f"{tag}: {name}")
    np.testing.assert_array_equal(bits(got[3]), bits(want[3]), err_msg=f"{tag}: h bits")


def step(v, up):
    return np.nextafter(F(v), F(INF) if up else F(-INF))


# ---- flimo_sc_bin_host ---------------------------------------------------------------------------------------------------------------
def test_the_hosts_libm_and_the_host_entry_agree_on_every_point_the_suite_uses():
    """The sector comes from libm_atan2f (csrc/hip/flimo_math.h), the restatement's from this host's libm: every cloud of
    tests/test_gpu_sc.py and every sweep of the scene, with no exception."""
    clouds = [(sc.random_cloud(5, 4097), sc.cfg(min_range=1.0, max_range=40.0), sc.yaw_frame12(0.7, (0.3, -0.2, 0.4))),
              (sc.random_cloud(3, 300), sc.cfg(), sc.yaw_frame12(0.1)), (sc.random_cloud(9, 3000), sc.cfg(), None),
              (sc.random_cloud(4, 2000), sc.cfg(), None), (sc.random_cloud(0, 65536, reach=60.0)[::16], sc.cfg(), None)]
    for i, (pts, c, frame) in enumerate(clouds):
        for f in (None, frame):
            same_bins(bins_host(pts, c, f), sc.bins(pts, c, f), f"cloud {i}")
    s = sc.scene()
    for i, pts in enumerate(s["kf_sweep"] + s["q_sweep"]):
        same_bins(bins_host(pts, sc.SCENE_CFG), sc.bins(pts, sc.SCENE_CFG), f"sweep {i}")


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_ranges_one_step_either_side_of_every_boundary(shape):
    """r one float32 step either side of every ring boundary, of min_range and of max_range, along +x (r = x exactly)."""
    c = sc.cfg(rings=shape[0], sectors=shape[1], min_range=1.5, max_range=80.0)
    edges = [c["max_range"] * t / shape[0] for t in range(shape[0] + 1)] + [c["min_range"], c["max_range"]]
    xs = np.array([v for e in edges for v in (step(e, False), F(e), step(e, True))], F)
    pts = np.stack([xs, np.zeros_like(xs), np.ones_like(xs)], axis=1)
    got, want = bins_host(pts, c), sc.bins(pts, c)
    same_bins(got, want, "ring edges")
    rscale = sc.scales(c)[0]
    for x, has, ring in zip(xs, got[0], got[1]):
        assert has == (x >= F(1.5) and x < F(80.0))
        if has:
            assert ring == min(shape[0] - 1, int(F(x * rscale))) and 0 <= ring < shape[0]
    assert got[0][-3:].tolist() == [True, False, False] and got[1][-3] == shape[0] - 1      # below max_range: the last ring
    lo = [i for i, x in enumerate(xs) if x == step(1.5, False)][0]
    assert not got[0][lo] and got[0][lo + 1]


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_angles_one_step_either_side_of_every_sector_boundary(shape):
    """Directions at every sector boundary and one float32 step of the angle's argument either side, the four axes and both zeros."""
    c = sc.cfg(rings=shape[0], sectors=shape[1], max_range=100.0)
    S = shape[1]
    pts = []
    for j in range(S + 1):
        a = 2.0 * math.pi * j / S
        x, y = F(10.0 * math.cos(a)), F(10.0 * math.sin(a))
        pts += [(x, y), (x, step(y, True)), (x, step(y, False)), (step(x, True), y), (step(x, False), y)]
    pts += [(5.0, 0.0), (5.0, -0.0), (-5.0, 0.0), (-5.0, -0.0), (0.0, 5.0), (-0.0, 5.0), (0.0, -5.0), (-0.0, -5.0), (0.0, 0.0), (-0.0, 0.0)]
    p = np.array([(x, y, 1.0) for x, y in pts], F)
    got, want = bins_host(p, c), sc.bins(p, c)
    same_bins(got, want, "sector edges")
    assert got[0][:-2].all() and not got[0][-2:].any()      # (r = 0 has no bin)
    k = len(pts) - 10
    assert got[2][k] == 0 and got[2][k + 1] == 0                                   # +x with y = +0 and -0: angle 0
    assert got[2][k + 2] == S // 2 and got[2][k + 3] == S // 2                     # -x: pi and -pi + 2 pi
    assert got[2][k + 4] == S // 4 and got[2][k + 6] == (3 * S) // 4
    assert got[2].max() == S - 1 and got[2][got[0]].min() == 0


def test_heights_non_finite_components_and_a_yaw_frame():
    c = sc.cfg(z_offset=2.0)
    zs = [step(-2.0, False), F(-2.0), step(-2.0, True), F(0.0), F(-0.0), F(3.5)]
    p = np.array([(3.0, 4.0, z) for z in zs], F)
    got = bins_host(p, c)
    same_bins(got, sc.bins(p, c), "heights")
    assert got[0].tolist() == [False, False, True, True, True, True] and got[3][2] == step(-2.0, True) + F(2.0) and got[3][5] == F(5.5)
    bad = np.array([(np.nan, 1, 1), (1, np.nan, 1), (1, 1, np.nan), (np.inf, 1, 1), (1, -np.inf, 1), (1, 1, np.inf), (1, 1, -np.inf)], F)
    for f in (None, sc.yaw_frame12(0.3)):
        got = bins_host(bad, c, f)
        assert not got[0].any()
        same_bins(got, sc.bins(bad, c, f), "non-finite")
    # a quarter turn about z, worked by hand: (x, y) -> (-y, x); 60 sectors of 6 degrees, 20 rings of 4 m
    quarter = np.array([0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0], F)
    p = np.array([(10.0, 1.0, 0.0), (1.0, 10.0, 1.0), (-10.0, -1.0, 2.0), (3.0, -30.0, -1.0)], F)
    got = bins_host(p, c, quarter)
    assert got[0].all() and got[1].tolist() == [2, 2, 2, 7] and got[3].tolist() == [2.0, 3.0, 4.0, 1.0]
    # rotated: (-1, 10) at 95.7 deg, (-10, 1) at 174.3, (1, -10) at 275.7, (30, 3) at 5.7
    assert got[2].tolist() == [15, 29, 45, 0]
    same_bins(got, sc.bins(p, c, quarter), "quarter turn")
    assert bins_host(p, c)[2].tolist() == [0, 14, 30, 45]


def test_rejected_bin_calls():
    from fast_limo_amd import _lib, api
    for kw in (dict(rings=0), dict(sectors=65), dict(max_range=INF), dict(min_range=-1.0), dict(z_offset=float("nan"))):
        with pytest.raises(api.FlimoError):
            api.sc_bin_host((1, 1, 1), **kw)
    with pytest.raises(api.FlimoError):
        api.sc_bin_host((1, 1, 1), frame12=np.full(12, np.nan, F))
    has, ring, sector, h = api.sc_bin_host((10.0, 0.5, 1.0), _lib.sc_cfg())
    assert (has, ring, sector, float(h)) == (True, 2, 0, 3.0)


# ---- flimo_sc_dist_host --------------------------------------------------------------------------------------------------------------
def rf32(x):
    """A Fraction rounded to the nearest float32, ties to even (normal range), as a Fraction."""
    if x == 0:
        return Fraction(0)
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = 0
    while x >= 1 << 24:
        x /= 2; e += 1
    while x < 1 << 23:
        x *= 2; e -= 1
    n, r = divmod(x.numerator, x.denominator)
    half = Fraction(r, x.denominator)
    if half > Fraction(1, 2) or (half == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * Fraction(n) * Fraction(2) ** e


def rsqrt32(x):
    """The correctly rounded float32 square root of a Fraction that is a float32."""
    g = Fraction(F(math.sqrt(float(x))).item())
    for cand in sorted((g, Fraction(step(float(g), True).item()), Fraction(step(float(g), False).item())), key=lambda v: abs(v * v - x)):
        return cand


def hand_distance(A, B, s):
    """d(s) of two small descriptors in exact rational arithmetic with one float32 rounding per written operation."""
    R, S = len(A), len(A[0])

    def unit(D):
        out, valid = [[Fraction(0)] * S for _ in range(R)], [False] * S
        for j in range(S):
            c = Fraction(0)
            for t in range(R):
                c = rf32(Fraction(D[t][j]) * Fraction(D[t][j]) + c)
            n = rsqrt32(c)
            valid[j] = n > 0
            for t in range(R):
                out[t][j] = rf32(Fraction(D[t][j]) / n) if valid[j] else Fraction(0)
        return out, valid
    ua, va = unit(A)
    ub, vb = unit(B)
    slots, m = [Fraction(0)] * 64, 0
    for j in range(S):
        jq = (j + s) % S
        if va[jq] and vb[j]:
            c = Fraction(0)
            for t in range(R):
                c = rf32(ua[t][jq] * ub[t][j] + c)
            slots[j], m = c, m + 1
    while len(slots) > 1:
        slots = [rf32(slots[i] + slots[i + 1]) for i in range(0, len(slots), 2)]
    if m == 0:
        return None, 0
    d = rf32(1 - rf32(slots[0] / m))
    return max(d, Fraction(0)), m


def test_a_three_by_four_pair_worked_by_hand():
    from fast_limo_amd import api
    A = [[1.5, 0.0, 2.25, 0.7], [0.3, 0.0, 1.0, 2.5], [2.0, 0.0, 0.1, 1.1]]
    B = [[0.9, 2.0, 0.0, 1.3], [1.7, 0.4, 0.0, 0.2], [0.6, 1.9, 0.0, 3.0]]
    A, B = np.array(A, F), np.array(B, F)
    hand = [hand_distance(A.tolist(), B.tolist(), s) for s in range(4)]
    assert [m for _, m in hand] == [2, 2, 2, 3]      # (A's column 1 and B's column 2 are empty: only shift 3 lets three pairs meet)
    have, dist, shift, prof = api.sc_dist_host(A, B, want_profile=True)
    assert have and [Fraction(float(v)) for v in prof] == [d for d, _ in hand]
    best = min(range(4), key=lambda s: (hand[s][0], s))
    assert shift == best and Fraction(float(dist)) == hand[best][0]
    P = sc.profiles(A, B)[0, 0]
    assert bits(prof).tolist() == bits(P).tolist()
    # min_cols at m(s) - 1, m(s), m(s) + 1 of the best shift and of the three-column shift
    for mc, open_ in ((1, [0, 1, 2, 3]), (2, [0, 1, 2, 3]), (3, [3]), (4, [])):
        have, dist, shift, prof = api.sc_dist_host(A, B, min_cols=mc, want_profile=True)
        assert np.flatnonzero(~np.isnan(prof)).tolist() == open_ and have == bool(open_)
        assert bits(prof).tolist() == bits(sc.profiles(A, B, mc)[0, 0]).tolist()
        if not open_:
            assert shift == -1 and dist == 0


def test_fmaf_quick_is_fmaf_and_the_tree_is_the_tree():
    rs = np.random.RandomState(0)
    a, b, c = (rs.standard_normal(200000).astype(F) for _ in range(3))
    c[::7] = (-(a[::7].astype(np.float64) * b[::7])).astype(F)      # (cancellation)
    assert bits(sc.fmaf_quick(a, b, c)).tolist() == bits(fmaf(a, b, c)).tolist()
    v = rs.rand(3, 64).astype(F)
    for row, got, wide in zip(v, sc.slot_tree32(v), fpc.slot_tree(v)):
        t = [F(x) for x in row]
        while len(t) > 1:
            t = [F(t[i] + t[i + 1]) for i in range(0, len(t), 2)]
        assert bits(got) == bits(t[0]) and abs(float(got) - wide) < 1e-4


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_a_descriptor_against_its_own_roll_and_against_the_restatement(shape):
    from fast_limo_amd import api
    R, S = shape
    D = sc.random_descs(3, 4, R, S, empty=0.1 if S > 2 else 0.0)
    if S == 2:      # (one ring: every valid column normalises to 1, so only an empty column tells the two shifts apart)
        D[:, :, 0] += 1
        D[0, :, 1] = 0
    for s in range(S):
        q = np.roll(D[0], s, axis=1)
        have, dist, shift, prof = api.sc_dist_host(q, D[0], want_profile=True)
        want = sc.profiles(q, D[0])[0, 0]
        assert have and shift == s and bits(prof).tolist() == bits(want).tolist()
        assert bits(dist) == bits(sc.pair_best(want)[1]) and float(dist) < 1e-6
    for i in range(1, 4):
        for mc in (1, max(S // 2, 1), S):
            have, dist, shift, prof = api.sc_dist_host(D[0], D[i], min_cols=mc, want_profile=True)
            want = sc.profiles(D[0], D[i], mc)[0, 0]
            w_have, w_dist, w_shift = sc.pair_best(want)
            assert np.array_equal(np.isnan(prof), np.isnan(want)) and bits(np.nan_to_num(prof)).tolist() == bits(np.nan_to_num(want)).tolist()
            assert (have, shift) == (bool(w_have), int(w_shift)) and bits(dist) == bits(w_dist)


def test_exclusions_and_ties_between_shifts():
    from fast_limo_amd import api
    D = sc.random_descs(8, 2, 20, 60, empty=0.0)
    zero = np.zeros((20, 60), F)
    for a, b in ((zero, D[0]), (D[0], zero), (zero, zero)):
        have, dist, shift, prof = api.sc_dist_host(a, b, want_profile=True)
        assert not have and dist == 0 and shift == -1 and np.isnan(prof).all()
    for bad in (np.nan, np.inf, -np.inf):
        E = D[1].copy()
        E[19, 59] = bad
        assert not api.sc_dist_host(D[0], E)[0] and not api.sc_dist_host(E, D[0])[0] and not sc.pair_best(sc.profiles(D[0], E)[0, 0])[0]
    # period sectors / 2: shifts s and s + 30 tie bit for bit, the smaller wins
    half = sc.random_descs(9, 1, 20, 30, empty=0.0)[0]
    per = np.concatenate([half, half], axis=1)
    for s in (0, 7, 29):
        have, dist, shift, prof = api.sc_dist_host(np.roll(per, s, axis=1), per, want_profile=True)
        assert have and shift == s and bits(prof[s]) == bits(prof[s + 30]) == bits(dist)
        assert bits(prof).tolist() == bits(sc.profiles(np.roll(per, s, axis=1), per)[0, 0]).tolist()
    for args in ((D[0], D[1], 0), (D[0], D[1], 61)):
        with pytest.raises(api.FlimoError):
            api.sc_dist_host(*args)
    with pytest.raises(ValueError):
        api.sc_dist_host(D[0], D[1][:, :30])


# ---- the method, on the restatement alone --------------------------------------------------------------------------------------------
def test_every_query_of_the_scene_finds_its_keyframe_and_its_yaw():
    """A ground plane and 150 random boxes along a 190 m strip (sc.scene, seed 3); 20 keyframes 10 m apart, 20 queries up to 1 m off
    a keyframe, every yaw random; 20 x 60 out to 25 m.  Every query's first entry is its keyframe and the yaw of sc_guesses is within
    one sector (6 degrees) of the truth.  With this seed: the worst distance to the right keyframe is 0.2076, the best runner-up
    0.3218; the worst yaw error 2.88 degrees."""
    from fast_limo_amd import api
    s = sc.scene()
    assert len(s["kf_sweep"]) == 20 and min(len(p) for p in s["kf_sweep"]) > 3000
    K, Q = sc.scene_descs()
    m = sc.match(Q, K, 2)
    print(f"worst distance {m['dist'][:, 0].max():.4f}, best runner-up {m['dist'][:, 1].min():.4f}")
    assert np.array_equal(m["idx"][:, 0], s["truth"]) and np.all(m["cnt"] == 2)
    assert m["dist"][:, 0].max() < m["dist"][:, 1].min()
    g = api.sc_guesses(s["kf_x26"], m["idx"][:, 0], m["shift"][:, 0], 60)
    err = np.array([abs(sc.wrap(sc.yaw_of(g[i]) - sc.yaw_of(s["q_x26"][i]))) for i in range(20)])
    print(f"worst yaw error {math.degrees(err.max()):.2f} degrees")
    assert np.all(err <= 2.0 * math.pi / 60)
    assert np.array_equal(g[:, 0:3], s["kf_x26"][:, 0:3]) and np.allclose(np.linalg.norm(g[:, 3:7], axis=1), 1.0)
    assert np.allclose(g[:, 3:5], 0.0)      # (roll and pitch are the keyframe's: none)
    with pytest.raises(ValueError):
        api.sc_guesses(s["kf_x26"], [20], [0], 60)
