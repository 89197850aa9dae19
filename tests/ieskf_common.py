"""An independent reference for the filter's 23-dof algebra, and the fixed inputs the CPU and GPU tests of it share.

The reference is written from the reference implementation's own files -- IKFoM_toolkit/esekfom/esekfom.hpp:1652-1764,
mtk/src/mtkmath.hpp (tolerance, cos_sinc_sqrt, hat, A_matrix, exp, log), mtk/types/SOn.hpp (SO3 boxplus / boxminus / exp / log) and
mtk/types/S2.hpp (S2<double, 98090, 10000, 1>: Bx, Nx_yy, Mx, boxminus, boxplus) -- in mpmath at 50 digits, not from the product's
restatement of them.  What the reference does in double precision ON PURPOSE is kept: its branch conditions are evaluated on the double
inputs with its double constants (the tolerance 1e-11, the literal 3.1415926, length = 98090.0 / 10000.0, the Taylor bound
eps^(1/4)), `scalar(1/2)` in S2_Mx is the integer division 0, and cos_sinc_sqrt below its bound is the reference's three-term
polynomial, not cos and sinc.  Everything else is exact to 50 digits: the difference to a double implementation is that
implementation's rounding.

Error scales (section 5 of the issue; `eps` = 2^-52), per item, `|.|` the largest magnitude among the item's outputs:
  A_matrix            eps (1 + 1 / |v|) per entry: (1 - cos |v|) / |v|^2 cancels -- the reference's own formula, kept;
  a 12 x 12 solve     eps cond_2(T) |solution|;
  S2 boxminus         eps (1 + |out|): hat(a) o and hat(o) a cancel to L^2 sin(theta) with an absolute error of eps L^2, and
                      theta / v_sin ~ 1 / L^2 turns that into eps radians whatever the angle -- again the reference's own formula;
  the other helpers   eps |out|;
  the pre half        dx_new: eps (1 + |dx_new|) (a product of unit quaternions is good to eps absolutely, and the S2 term above);
                      A11^-1, G2: eps cond_2(A11) amp |out| with amp = 1 + sum over the two rotation blocks of 1 / |v| (their
                      A_matrix entries carry eps / |v| into P_);
  one iteration       dx_: eps (cond_2(N) amp (|dx_| + |dx_new|) + 1 + |dx_new|), N = A11^-1 + H^T H: the solve, and dx_new's own
                      error, which dx_ = K_h + (K_x - I) dx_new carries over one to one; x_after: that + eps |x_after|.
The HOST twins' worst error over the fixed inputs below, in units of these scales, is measured by tests/test_ieskf_host.py (it
prints them) and recorded in K_HOST; host and device are asserted against mpmath at 4 K_HOST, device against host at 8 K_HOST."""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = 2.0 ** -52
TOL = mp.mpf(1e-11)                       # MTK::tolerance<double>()
L_S2 = mp.mpf(98090.0 / 10000.0)          # S2::length = scalar(den) / scalar(num)
PI_LIT = mp.mpf(3.1415926)                # S2.hpp:152
L_F = 98090.0 / 10000.0

# the host twins' worst error over the inputs of this module in units of the scales above, as tests/test_ieskf_host.py measures
# it on an x86-64 host with glibc; DESIGN.md section 6 has the table with the device's values beside them
K_HOST = {
    "so3_log": 1.49, "A_T": 0.52, "exp_quat": 1.35, "cos_sinc_sqrt": 0.67, "s2_Bx": 1.16, "s2_boxminus": 1.37, "s2_J": 2.04,
    "gj_inverse": 0.95, "gj_solve": 0.69, "pre_dxn": 0.99, "pre_AI": 1.23, "pre_G2": 1.39, "iter_dx": 1.17, "iter_x": 2.13,
}


# --------------------------------------------------------------------------------------------------------------------------------
# mpmath: mtkmath.hpp
# --------------------------------------------------------------------------------------------------------------------------------
def M(rows):
    return mp.matrix(rows)


def vec(v):
    return [mp.mpf(float(t)) for t in v]


def mp_hat(v):
    return M([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def mp_norm(v):
    return mp.sqrt(sum(t * t for t in v))


def mp_A_matrix(v):
    """mtkmath.hpp:236-247"""
    sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    n = mp.sqrt(sq)
    if n < TOL:
        return mp.eye(3)
    H = mp_hat(v)
    return mp.eye(3) + (1 - mp.cos(n)) / sq * H + (1 - mp.sin(n) / n) / sq * (H * H)


TAYLOR_N_BOUND = mp.mpf(float(np.sqrt(np.sqrt(np.float64(2.220446049250313e-16)))))


def mp_cos_sinc_sqrt(x2):
    """mtkmath.hpp:143-174"""
    if x2 >= TAYLOR_N_BOUND:
        x = mp.sqrt(x2)
        return mp.cos(x), mp.sin(x) / x
    inv = [mp.mpf(1) / k for k in (3, 4, 5, 6, 7, 8, 9)]
    cosi, sinc = mp.mpf(1), mp.mpf(1)
    term = -x2 / 2
    for i in range(3):
        cosi += term
        term *= inv[2 * i]
        sinc += term
        term *= -inv[2 * i + 1] * x2
    return cosi, sinc


def mp_exp(v, scale):
    """mtkmath.hpp:249-256: (w, vec)"""
    c, s = mp_cos_sinc_sqrt(scale * scale * sum(t * t for t in v))
    return c, [s * scale * t for t in v]


def mp_log(w, v, scale=2):
    """mtkmath.hpp:268-288 with plus_minus_periodicity = true (SOn.hpp:293-297)"""
    nv = mp_norm(v)
    if nv < TOL:
        nv = TOL
    s = scale / nv * mp.atan(nv / w)
    return [s * t for t in v]


# quaternions: x y z w (Eigen's coefficient order, and the flat state's)
def mp_qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def mp_q2r(q):
    x, y, z, w = q
    return M([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
              [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
              [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def mp_so3_exp(v, scale=1):
    """SOn.hpp:284-288"""
    w, u = mp_exp(v, mp.mpf(scale) / 2)
    return [u[0], u[1], u[2], w]


def mp_so3_log(q):
    return mp_log(q[3], q[0:3])


def mp_so3_boxminus(a, other):
    """SOn.hpp:237-239: log(other.conjugate() * this)"""
    oc = [-other[0], -other[1], -other[2], other[3]]
    return mp_so3_log(mp_qmul(oc, a))


# --------------------------------------------------------------------------------------------------------------------------------
# mpmath: S2.hpp, S2_typ == 1
# --------------------------------------------------------------------------------------------------------------------------------
def mp_s2_chart(v):
    return 0 if v[0] + L_S2 > TOL else 1


def mp_s2_Bx(v):
    """S2.hpp:215-231"""
    Lg = L_S2
    if v[0] + Lg > TOL:
        d = Lg + v[0]
        B = M([[-v[1], -v[2]], [Lg - v[1] * v[1] / d, -v[2] * v[1] / d], [-v[2] * v[1] / d, Lg - v[2] * v[2] / d]])
        return B / Lg
    B = mp.zeros(3, 2)
    B[1, 1] = -1
    B[2, 0] = 1
    return B


def mp_s2_boxminus(a, other):
    """S2.hpp:144-167; returns (res, branch): 0 general, 1 equal, 2 antipodal"""
    av, ov = M(a), M(other)
    v_sin = mp_norm(list(mp_hat(a) * ov))
    v_cos = sum(s * t for s, t in zip(a, other))
    theta = mp.atan2(v_sin, v_cos)
    if v_sin < TOL:
        if abs(theta) > TOL:
            return [PI_LIT, mp.mpf(0)], 2
        return [mp.mpf(0), mp.mpf(0)], 1
    r = theta / v_sin * (mp_s2_Bx(other).T * (mp_hat(other) * av))
    return [r[0], r[1]], 0


def mp_s2_Nx_yy(v):
    """S2.hpp:259-264"""
    return 1 / L_S2 / L_S2 * (mp_s2_Bx(v).T * mp_hat(v))


def mp_s2_Mx(v, delta):
    """S2.hpp:266-280; exp(.., scalar(1/2)) is exp(.., 0): the identity rotation"""
    B = mp_s2_Bx(v)
    if mp_norm(delta) < TOL:
        return -1 * (mp_hat(v) * B)
    Bu = list(B * M(delta))
    w, u = mp_exp(Bu, mp.mpf(0))
    E = mp_q2r([u[0], u[1], u[2], w])
    return -1 * (E * mp_hat(v) * mp_A_matrix(Bu).T * B)


def mp_s2_J(now, prop, delta):
    return mp_s2_Nx_yy(now) * mp_s2_Mx(prop, delta)


def mp_s2_boxplus(v, delta):
    """S2.hpp:136-142"""
    Bu = list(mp_s2_Bx(v) * M(delta))
    w, u = mp_exp(Bu, mp.mpf(1) / 2)
    return list(mp_q2r([u[0], u[1], u[2], w]) * M(v))


# --------------------------------------------------------------------------------------------------------------------------------
# mpmath: one outer iteration, esekfom.hpp:1652-1764 (n <= dof_Measurement branch, every eigenvalue >= D)
# flat state: pos 3, rot 4, offset_R_L_I 4, offset_T_L_I 3, vel 3, bg 3, ba 3, grav 3; tangent: 3 3 3 3 3 3 3 2
# --------------------------------------------------------------------------------------------------------------------------------
VECT = ((0, 0), (11, 9), (14, 12), (17, 15), (20, 18))      # (offset in x26, offset in dx) of the five vect<3> members
SO3 = ((3, 3), (7, 6))


def mp_state_boxminus(x, xp):
    dx = [mp.mpf(0)] * 23
    for xo, do in VECT:
        for i in range(3):
            dx[do + i] = x[xo + i] - xp[xo + i]
    for xo, do in SO3:
        dx[do:do + 3] = mp_so3_boxminus(x[xo:xo + 4], xp[xo:xo + 4])
    dx[21:23], _ = mp_s2_boxminus(x[23:26], xp[23:26])
    return dx


def mp_state_boxplus(x, d):
    y = list(x)
    for xo, do in VECT:
        for i in range(3):
            y[xo + i] = x[xo + i] + d[do + i]
    for xo, do in SO3:
        y[xo:xo + 4] = mp_qmul(x[xo:xo + 4], mp_so3_exp(d[do:do + 3]))
    y[23:26] = mp_s2_boxplus(x[23:26], d[21:23])
    return y


def mp_pre(x, xp, P):
    """:1652-1697: (dx_new, P_ through the manifold blocks, [|v_rot|, |v_offR|])"""
    dx = mp_state_boxminus(x, xp)
    dxn = M(dx)
    P_ = P.copy()
    vn = []
    for _, idx in SO3:
        seg = dx[idx:idx + 3]
        vn.append(mp_norm(seg))
        J = mp_A_matrix(seg).T
        dxn[idx:idx + 3, 0] = J * dxn[idx:idx + 3, 0]
        P_[idx:idx + 3, :] = J * P_[idx:idx + 3, :]
        P_[:, idx:idx + 3] = P_[:, idx:idx + 3] * J.T
    J = mp_s2_J(x[23:26], xp[23:26], dx[21:23])
    dxn[21:23, 0] = J * dxn[21:23, 0]
    P_[21:23, :] = J * P_[21:23, :]
    P_[:, 21:23] = P_[:, 21:23] * J.T
    return dxn, P_, vn


def mp_iteration(x, xp, P, R, HTH, HTh):
    """:1652-1747 in the literal two-inverse form of :1722-1733: (dx_, x after boxplus, dx_new, N = A11^-1 + H^T H)"""
    dxn, P_, _ = mp_pre(x, xp, P)
    P_temp = mp.inverse(P_ / R)
    Ai = mp.inverse((P_ / R)[0:12, 0:12])
    P_temp[0:12, 0:12] = P_temp[0:12, 0:12] + HTH
    P_inv = mp.inverse(P_temp)
    K_h = P_inv[:, 0:12] * HTh
    K_x = mp.zeros(23, 23)
    K_x[:, 0:12] = P_inv[:, 0:12] * HTH
    dx_ = K_h + (K_x - mp.eye(23)) * dxn
    return list(dx_), mp_state_boxplus(x, list(dx_)), list(dxn), Ai + HTH


def to_mp_matrix(a):
    a = np.asarray(a, dtype=np.float64)
    return M([[mp.mpf(float(t)) for t in row] for row in a.reshape(a.shape[0], -1)])


def to_np(m):
    if isinstance(m, mp.matrix):
        return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])
    return np.array([float(t) for t in m])


def err_units(got, ref_mp, scale):
    """max |got - ref| / scale over the item's entries; ref_mp: list / mp.matrix in the entries' order"""
    ref = list(ref_mp) if not isinstance(ref_mp, mp.matrix) else [ref_mp[i, j] for i in range(ref_mp.rows) for j in range(ref_mp.cols)]
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    assert len(ref) == got.size
    worst = mp.mpf(0)
    for g, r in zip(got, ref):
        assert np.isfinite(g), got
        worst = max(worst, abs(mp.mpf(float(g)) - r))
    return float(worst / mp.mpf(scale)) if worst > 0 else 0.0


def mp_maxabs(ref):
    ref = list(ref) if not isinstance(ref, mp.matrix) else [ref[i, j] for i in range(ref.rows) for j in range(ref.cols)]
    return float(max(abs(t) for t in ref))


# --------------------------------------------------------------------------------------------------------------------------------
# numpy: the float32 pose constants of a pass (State.cpp:38-55,136-172, Localizer.cpp:554-555) as pose_from_x26 forms them
# --------------------------------------------------------------------------------------------------------------------------------
def _q2r(q, one, two):
    tx, ty, tz = two * q[0], two * q[1], two * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def pose_f32(x26):
    """[RT 16, RT_inv 16, TLI_inv 16, R_inv 9, RLI_inv 9] float32"""
    f = np.float32
    x = np.asarray(x26, dtype=np.float64)
    one, two, zero = f(1), f(2), f(0)

    def se3(q, p):
        Rm = _q2r(q, one, two)
        return [Rm[0], Rm[1], Rm[2], p[0], Rm[3], Rm[4], Rm[5], p[1], Rm[6], Rm[7], Rm[8], p[2], zero, zero, zero, one]

    def se3_inv(q, p):
        Rm = _q2r(q, one, two)
        Rt = [Rm[0], Rm[3], Rm[6], Rm[1], Rm[4], Rm[7], Rm[2], Rm[5], Rm[8]]
        t = [(-Rt[3 * i]) * p[0] + ((-Rt[3 * i + 1]) * p[1] + (-Rt[3 * i + 2]) * p[2]) for i in range(3)]
        return [Rt[0], Rt[1], Rt[2], t[0], Rt[3], Rt[4], Rt[5], t[1], Rt[6], Rt[7], Rt[8], t[2], zero, zero, zero, one]

    with np.errstate(all="ignore"):
        p = [f(t) for t in x[0:3]]
        q = [f(t) for t in x[3:7]]
        qLI = [f(t) for t in x[7:11]]
        pLI = [f(t) for t in x[11:14]]
        d1, d2 = np.float64(1), np.float64(2)
        Rd = _q2r([-x[3], -x[4], -x[5], x[6]], d1, d2)
        Ld = _q2r([-x[7], -x[8], -x[9], x[10]], d1, d2)
        out = se3(q, p) + se3_inv(q, p) + se3_inv(qLI, pLI) + [f(t) for t in Rd] + [f(t) for t in Ld]
    return np.array(out, dtype=np.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# fixed inputs
# --------------------------------------------------------------------------------------------------------------------------------
V_LADDER = (0.0, 0.9e-11, 1.1e-11, 1e-9, 1e-8, 1e-6, 1e-3, 0.0220, 0.0222, 0.5, 1.5, 3.0, float(np.pi) - 1e-9)
STEP_LADDER = (1e-12, 1e-9, 1e-6, 0.0220, 0.0222, 0.5, 1.5, 3.0)


def axes(n_tilted=6, seed=11):
    """unit axes: n_tilted tilted ones, then the six pure ones"""
    r = np.random.default_rng(seed)
    a = r.normal(size=(n_tilted, 3))
    a /= np.linalg.norm(a, axis=1)[:, None]
    pure = np.concatenate([np.eye(3), -np.eye(3)])
    return np.concatenate([a, pure])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_of(v):
    """a unit quaternion x y z w turning by |v| about v (float64; only used to make inputs)"""
    v = np.asarray(v, dtype=np.float64)
    n = np.linalg.norm(v)
    if n == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(n / 2) * v / n, [np.cos(n / 2)]])


def rotate(g, axis, ang):
    """g turned by ang about axis (Rodrigues, float64; only used to make inputs)"""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    return g * np.cos(ang) + np.cross(k, g) * np.sin(ang) + k * np.dot(k, g) * (1 - np.cos(ang))


def perp(g, phi):
    """a unit vector perpendicular to g, turned by phi about it"""
    g = g / np.linalg.norm(g)
    e = np.eye(3)[int(np.argmin(np.abs(g)))]
    u = np.cross(g, e)
    u /= np.linalg.norm(u)
    return rotate(u, g, phi)


@functools.lru_cache(None)
def in_A_T():
    return np.array([m * a for m in V_LADDER for a in axes()])


@functools.lru_cache(None)
def in_exp_quat():
    v = in_A_T()
    half = np.concatenate([v, np.full((len(v), 1), 0.5)], axis=1)
    one = np.concatenate([v[::2], np.full((len(v[::2]), 1), 1.0)], axis=1)
    return np.concatenate([half, one])


@functools.lru_cache(None)
def in_cos_sinc_sqrt():
    bn = float(TAYLOR_N_BOUND)
    x2 = [0.25 * m * m for m in V_LADDER] + [bn, np.nextafter(bn, 0.0), np.nextafter(bn, 1.0), 0.5 * bn, 2.0 * bn]
    x2 += list(np.random.default_rng(12).uniform(0.0, bn, 12)) + list(np.random.default_rng(13).uniform(bn, 9.0, 12))
    return np.array(x2).reshape(-1, 1)


@functools.lru_cache(None)
def in_so3_log():
    ax = axes()
    q = [quat_of(m * a) for m in V_LADDER for a in ax]                                   # w > 0
    q += [-quat_of(m * a) for m in V_LADDER[3:] for a in ax[::2]]                        # w < 0
    for s in (1.0, -1.0):                                                                # |w| = 1e-9: atan(nv / w) at +-1e9
        q += [np.concatenate([a * np.sqrt(1.0 - 1e-18), [s * 1e-9]]) for a in ax]
        for nv in (0.9e-11, 1.1e-11):                                                    # nv itself either side of the tolerance
            q += [np.concatenate([a * nv, [s * np.sqrt(1.0 - nv * nv)]]) for a in ax[::2]]
    return np.array(q)


def _g_dirs():
    """(name, g) with |g| = 9.809"""
    down = np.array([0.0, 0.0, -L_F])
    out = [("down", down)]
    for k, a in enumerate(axes(4, 21)[:4]):
        out.append(("tilt20", rotate(down, perp(down, 1.3 * k), np.deg2rad(20.0))))
        out.append(("tilt90", rotate(down, perp(down, 0.7 + 1.3 * k), np.deg2rad(90.0))))
    for d in (1e-3, 1e-6, 1e-10):
        for k in range(5):
            phi = 0.4 + 1.25 * k
            out.append((f"near{d:g}", L_F * np.array([-np.cos(d), np.sin(d) * np.cos(phi), np.sin(d) * np.sin(phi)])))
    out.append(("on", np.array([-L_F, 0.0, 0.0])))
    return out


@functools.lru_cache(None)
def in_s2_Bx():
    return np.array([g for _, g in _g_dirs()])


@functools.lru_cache(None)
def in_s2_boxminus():
    """pairs (a, other): equal, antipodal, and 1e-12, 1e-6, 0.0442, 1 and 3 rad apart, `other` on both charts"""
    pairs = []
    for k, (_, o) in enumerate(_g_dirs()):
        pairs.append((o, o))
        pairs.append((-o, o))
        for j, ang in enumerate((1e-12, 1e-6, 0.0221 * 2, 1.0, 3.0)):
            pairs.append((rotate(o, perp(o, 0.9 * k + 2.1 * j), ang), o))
    return np.array([np.concatenate(p) for p in pairs])


@functools.lru_cache(None)
def in_s2_J():
    """(now, prop, delta = now boxminus prop as the reference computes it, rounded to double) -- the way :1687-1689 calls it"""
    rows = []
    for p in in_s2_boxminus():
        d, _ = mp_s2_boxminus(vec(p[0:3]), vec(p[3:6]))
        rows.append(np.concatenate([p, [float(d[0]), float(d[1])]]))
    return np.array(rows)


# ---- 12 x 12 systems ----
def _spd(rng, cond, scale):
    Q, _ = np.linalg.qr(rng.normal(size=(12, 12)))
    w = scale * np.logspace(0, -np.log10(cond), 12)
    A = (Q * w) @ Q.T
    return 0.5 * (A + A.T)


def _blockdiag(k, B):
    A = np.eye(12)
    A[k:, k:] = B
    return A


@functools.lru_cache(None)
def gj_systems():
    """[(kind, T)]: kinds spd / perm / tie2 / tie3 / tie_pm / neg / reverse are regular, zero0 / zero5 / zero11 have a zero pivot"""
    r = np.random.default_rng(31)
    out = []
    for cond in (1e2, 1e7, 1e12):
        for scale in (1.0, 1e4, 1e-3):
            for _ in range(3):
                out.append(("spd", _spd(r, cond, scale)))
    for s in range(10):
        Pm = np.eye(12)[r.permutation(12)]
        out.append(("perm", Pm if s < 5 else Pm * r.choice([-1.0, 1.0], size=(12, 1))))
    for kind, rows_n in (("tie2", 2), ("tie3", 3), ("tie_pm", 2)):
        for k in (0, 0, 0, 3, 3, 7, 7, 9, 9, 10):              # the tie is met at elimination step k: rows 0 .. k-1 are the identity's
            n = 12 - k
            if n < rows_n:
                continue
            B = r.uniform(-1.0, 1.0, size=(n, n)) + 3.0 * np.eye(n)
            rows = np.sort(r.choice(n, size=rows_n, replace=False))
            B[:, 0] = r.uniform(-1.0, 1.0, size=n)
            sign = np.ones(rows_n) if kind != "tie_pm" else np.array([1.0, -1.0])[:: (1 if r.random() < 0.5 else -1)]
            B[rows, 0] = 4.0 * sign
            out.append((kind, _blockdiag(k, B)))
    for _ in range(10):
        out.append(("neg", -_spd(r, 1e3, 10.0)))
    for _ in range(10):
        A = r.uniform(-0.1, 0.1, size=(12, 12))
        for k in range(12):
            A[11 - k, k] = (10.0 + k) * (1.0 if k % 3 else -1.0)
        out.append(("reverse", A))
    for k in (0, 5, 11):
        for _ in range(4):
            n = 12 - k
            B = r.uniform(-1.0, 1.0, size=(n, n)) + 3.0 * np.eye(n)
            B[:, 0] = 0.0
            out.append((f"zero{k}", _blockdiag(k, B)))
    return out


@functools.lru_cache(None)
def gj_rhs():
    return np.random.default_rng(32).normal(size=(len(gj_systems()), 12))




@functools.lru_cache(None)
def gj_refs():
    """per regular system: (cond_2, T^-1, T^-1 v) in mpmath; None for the singular ones"""
    out = []
    for (kind, T), v in zip(gj_systems(), gj_rhs()):
        if kind.startswith("zero"):
            out.append(None)
            continue
        Tm = to_mp_matrix(T)
        Xi = mp.inverse(Tm)
        out.append((float(np.linalg.cond(T)), Xi, mp.lu_solve(Tm, M(vec(v)))))
    return out


# ---- filter states ----
def state_tool():
    """the near-identity state of tools/ieskf_bench.hip"""
    x = np.zeros(26)
    x[0:3] = [0.3, -0.2, 0.1]
    x[3:7] = [0.0, 0.0, np.sin(0.01), np.cos(0.01)]
    x[10] = 1.0
    g = np.array([0.05, -0.03, -9.8088])
    x[23:26] = g * (9.809 / np.linalg.norm(g))
    return x


def state_general(w_negative=False, grav="tilt20"):
    r = np.random.default_rng(41)
    a1, a2 = axes(2, 42)[:2]
    x = np.zeros(26)
    x[0:3] = [120.0, -340.0, 15.0]
    x[3:7] = quat_of(2.5 * a1) * (-1.0 if w_negative else 1.0)
    x[7:11] = quat_of(2.5 * a2)
    x[11:14] = [0.4, -0.1, 0.25]
    v = r.normal(size=3)
    x[14:17] = 12.0 * v / np.linalg.norm(v)
    x[17:20] = [0.05, -0.05, 0.05]
    x[20:23] = [-0.05, 0.05, 0.05]
    down = np.array([0.0, 0.0, -L_F])
    if grav == "tilt20":
        x[23:26] = rotate(down, perp(down, 0.8), np.deg2rad(20.0))
    else:                                                       # 1e-6 rad from (-L, 0, 0): the other chart
        x[23:26] = L_F * np.array([-np.cos(1e-6), np.sin(1e-6) * np.cos(0.7), np.sin(1e-6) * np.sin(0.7)])
    return x


def states():
    return [("tool", state_tool()), ("general", state_general()), ("general_wneg", state_general(True)), ("grav_chart", state_general(False, "near"))]


def cov_tool():
    """the dense SPD P of tools/ieskf_bench.hip (its shape: 1e-3 A A^T + 1e-4 I, A ~ 0.02 N(0, 1)); seeded here"""
    A = 0.02 * np.random.default_rng(51).normal(size=(23, 23))
    return 1e-3 * (A @ A.T) + 1e-4 * np.eye(23)


def cov_diag():
    return np.diag(np.logspace(-8, 2, 23))


def cov_corr():
    """|rho| = 0.99 between pose (0:6) and gravity (21:23) and between pose and the extrinsics (6:12): G2 z moves them with the pose"""
    s = np.sqrt(np.concatenate([np.full(3, 1e-2), np.full(3, 1e-3), np.full(3, 1e-3), np.full(3, 1e-2), np.full(9, 1e-3), np.full(2, 1e-3)]))
    C = np.eye(23)
    for i, j, rho in ((0, 21, 0.99), (4, 22, -0.99), (3, 6, 0.99), (5, 8, -0.99), (1, 9, 0.99)):
        C[i, j] = C[j, i] = rho
    return C * np.outer(s, s)


def covs():
    return [("tool", cov_tool()), ("diag", cov_diag()), ("corr", cov_corr())]


def step_state(xp, step, k=0):
    """x with rot, offset_R_L_I and gravity `step` radians from xp's (and the vect members moved a little): x != x_prop"""
    a1, a2 = axes(2, 60 + k)[:2]
    x = xp.copy()
    x[3:7] = qmul(xp[3:7], quat_of(step * a1))
    x[7:11] = qmul(xp[7:11], quat_of(step * a2))
    x[23:26] = rotate(xp[23:26], perp(xp[23:26], 0.5 + k), step)
    x[0:3] += [0.03, -0.02, 0.01]
    x[14:17] += 0.01
    return x


@functools.lru_cache(None)
def pre_cases():
    """[(name, item [582])]: every state x every P, x == x_prop and x a rung of the ladder away"""
    out = []
    k = 0
    for sn, xp in states():
        for pn, P in covs():
            rungs = (0.0,) + STEP_LADDER if pn == "tool" else (0.0, STEP_LADDER[k % 8], STEP_LADDER[(k + 3) % 8])
            for step in rungs:
                k += 1
                x = xp.copy() if step == 0.0 else step_state(xp, step, k)
                out.append((f"{sn}/{pn}/{step:g}", np.concatenate([x, xp, P.reshape(-1), [0.001]])))
    return out


@functools.lru_cache(None)
def pre_refs():
    """per case: (dx_new [23], A11^-1, G2, cond_2(A11), amp) in mpmath"""
    out = []
    for _, it in pre_cases():
        x, xp, P, R = vec(it[0:26]), vec(it[26:52]), to_mp_matrix(it[52:581].reshape(23, 23)), mp.mpf(float(it[581]))
        dxn, P_, vn = mp_pre(x, xp, P)
        A = P_ / R
        Ai = mp.inverse(A[0:12, 0:12])
        G2 = A[12:23, 0:12] * Ai
        amp = 1.0 + sum(1.0 / float(v) for v in vn if v >= TOL)
        out.append((list(dxn), Ai, G2, float(np.linalg.cond(to_np(A[0:12, 0:12]))), amp))
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# the helpers: op, inputs, mpmath outputs, error scale per item
# --------------------------------------------------------------------------------------------------------------------------------
def _flat(m):
    return [m[i, j] for i in range(m.rows) for j in range(m.cols)] if isinstance(m, mp.matrix) else list(m)


def _ref_so3_log(a):
    return mp_so3_log(vec(a))


def _ref_A_T(a):
    return _flat(mp_A_matrix(vec(a)).T)


def _ref_exp_quat(a):
    w, u = mp_exp(vec(a[0:3]), mp.mpf(float(a[3])))
    return [u[0], u[1], u[2], w]


def _ref_cos_sinc(a):
    return list(mp_cos_sinc_sqrt(mp.mpf(float(a[0]))))


def _ref_Bx(a):
    return _flat(mp_s2_Bx(vec(a)))


def _ref_boxminus(a):
    return mp_s2_boxminus(vec(a[0:3]), vec(a[3:6]))[0]


def _ref_J(a):
    return _flat(mp_s2_J(vec(a[0:3]), vec(a[3:6]), vec(a[6:8])))


def _inv_or_0(n):
    return 1.0 / n if n >= 1e-11 else 0.0


# name: (op, inputs, reference, scale(item, |reference|) in units of eps)
HELPERS = {
    "so3_log": (0, in_so3_log, _ref_so3_log, lambda a, m: m),
    "A_T": (1, in_A_T, _ref_A_T, lambda a, m: 1.0 + _inv_or_0(float(np.linalg.norm(a[0:3])))),
    "exp_quat": (2, in_exp_quat, _ref_exp_quat, lambda a, m: m),
    "cos_sinc_sqrt": (3, in_cos_sinc_sqrt, _ref_cos_sinc, lambda a, m: m),
    "s2_Bx": (4, in_s2_Bx, _ref_Bx, lambda a, m: m),
    "s2_boxminus": (5, in_s2_boxminus, _ref_boxminus, lambda a, m: 1.0 + m),
    # (Mx holds A_matrix(Bx delta)^T, |Bx delta| = |delta|: its eps / |delta| per entry comes through hat(g) / L^2 ~ 1 / L ... L)
    "s2_J": (6, in_s2_J, _ref_J, lambda a, m: m * (1.0 + _inv_or_0(float(np.linalg.norm(a[6:8]))))),
}


@functools.lru_cache(None)
def helper_refs(name):
    """[(reference outputs in mpmath, scale)] per input item"""
    _, inputs, ref, scale = HELPERS[name]
    out = []
    for a in inputs():
        r = ref(a)
        out.append((r, EPS * scale(a, mp_maxabs(r))))
    return out


def helper_units(name, got):
    """the worst error of `got` [n, n_out] against mpmath in units of the helper's scale, and the item it occurs at"""
    refs = helper_refs(name)
    assert len(refs) == len(got)
    u = [err_units(g, r, s) if s > 0 else (0.0 if err_units(g, r, 1.0) == 0.0 else float("inf")) for g, (r, s) in zip(got, refs)]
    k = int(np.argmax(u))
    return u[k], k


def units_between(name, a, b):
    """the worst difference of two evaluations [n, n_out] in units of the helper's scale"""
    refs = helper_refs(name)
    worst = 0.0
    for x, y, (_, s) in zip(np.asarray(a), np.asarray(b), refs):
        d = float(np.max(np.abs(x - y)))
        worst = max(worst, d / s if s > 0 else (0.0 if d == 0.0 else float("inf")))
    return worst


# which branches the inputs of a helper must reach at least ten times each: {name: [(mask, value)]} on flimo_ieskf_eval_host's code
BRANCHES = {
    "so3_log": [(1, 0), (1, 1)], "A_T": [(1, 0), (1, 1)], "exp_quat": [(1, 0), (1, 1)], "cos_sinc_sqrt": [(1, 0), (1, 1)],
    "s2_Bx": [(1, 0), (1, 1)],
    "s2_boxminus": [(3, 0), (3, 1), (3, 2), (4, 0), (4, 4), (7, 4)],      # general, equal, antipodal; other chart; general ON the other chart
    "s2_J": [(1, 0), (1, 1), (2, 0), (2, 2), (4, 0), (4, 4)],
}


# ---- plain float64 Gauss-Jordan by the stated rule: the largest magnitude among the rows not yet used, the LOWEST row among equals
def gj_plain(T, v=None, highest=False):
    """(inverse or None, solution or None, ok, an exact tie was met) -- T [12, 12]; row_r -= (A[r][k] * (1 / A[p][k])) * row_p"""
    A = np.array(T, dtype=np.float64)
    X = np.eye(12)
    b = None if v is None else np.array(v, dtype=np.float64)
    used = np.zeros(12, bool)
    prow, dk, tied = [], [], False
    for k in range(12):
        mag = np.where(used, -1.0, np.abs(A[:, k]))
        top = mag.max()
        if not top > 0.0:
            return None, None, False, tied
        cand = np.flatnonzero(mag == top)
        tied = tied or len(cand) > 1
        p = int(cand[-1] if highest else cand[0])
        rinv = 1.0 / A[p, k]
        for r in range(12):
            if r == p:
                continue
            f = A[r, k] * rinv
            A[r] = A[r] - f * A[p]
            X[r] = X[r] - f * X[p]
            if b is not None:
                b[r] = b[r] - f * b[p]
        used[p] = True
        prow.append(p)
        dk.append(rinv)
    inv = np.array([X[prow[k]] * dk[k] for k in range(12)])
    sol = None if b is None else np.array([b[prow[k]] * dk[k] for k in range(12)])
    return inv, sol, True, tied


def gj_units(inv, sol):
    """worst error of inverses [n, 145] and solutions [n, 13] of gj_systems() against mpmath, in units of eps cond |solution|"""
    wi = ws = 0.0
    for i, ref in enumerate(gj_refs()):
        if ref is None:
            continue
        cond, Xi, u = ref
        assert inv[i, 144] == 1.0 and sol[i, 12] == 1.0, i
        wi = max(wi, err_units(inv[i, :144], Xi, EPS * cond * mp_maxabs(Xi)))
        ws = max(ws, err_units(sol[i, :12], u, EPS * cond * mp_maxabs(u)))
    return wi, ws


def pre_scales(i):
    dxn, Ai, G2, cond, amp = pre_refs()[i]
    return EPS * (1.0 + mp_maxabs(dxn)), EPS * cond * amp * mp_maxabs(Ai), EPS * cond * amp * max(mp_maxabs(G2), 1e-300)


def pre_units(out):
    """{pre_dxn, pre_AI, pre_G2: (worst units, case name)} of ik_pre outputs [n, 299] on pre_cases()"""
    w = {"pre_dxn": (0.0, ""), "pre_AI": (0.0, ""), "pre_G2": (0.0, "")}
    for i, ((name, _), (dxn, Ai, G2, _, _)) in enumerate(zip(pre_cases(), pre_refs())):
        s = pre_scales(i)
        for key, got, ref, sc in (("pre_dxn", out[i, 0:23], dxn, s[0]), ("pre_AI", out[i, 23:167], Ai, s[1]), ("pre_G2", out[i, 167:299], G2, s[2])):
            u = err_units(got, ref, sc)
            if u > w[key][0]:
                w[key] = (u, name)
    return w


# --------------------------------------------------------------------------------------------------------------------------------
# the whole algebra on fixed sums
# --------------------------------------------------------------------------------------------------------------------------------
def pack_sums(HTH, HTh, M):
    s = np.zeros(91)
    k = 0
    for i in range(12):
        for j in range(i, 12):
            s[k] = HTH[i, j]
            k += 1
    s[78:90] = HTh
    s[90] = M
    return s


def unpack_sums(s):
    HTH = np.zeros((12, 12))
    k = 0
    for i in range(12):
        for j in range(i, 12):
            HTH[i, j] = HTH[j, i] = s[k]
            k += 1
    return HTH, s[78:90].copy(), int(round(s[90]))


def one_group(s):
    g = np.zeros((8, 91))
    g[0] = s
    return g


def slot_order_sum(g):
    r = g[0].copy()
    for q in range(1, 8):
        r = r + g[q]
    return r


def mixed_groups(s, seed):
    """the sums spread over the eight groups with partials of magnitude 1e12, 1 and 1e-12 (relative) mixed: another order of
    addition gives other bits.  M stays whole."""
    r = np.random.default_rng(seed)
    a = r.uniform(0.5, 1.0, 91) * np.abs(s) * 1e12
    c = r.uniform(-1.0, 1.0, (2, 91)) * np.abs(s) * 1e-12
    b = s / 4.0
    g = np.array([a, b, c[0], -a, b, b, c[1], b])
    g[:, 90] = 0.0
    g[0, 90] = s[90]
    return g


@functools.lru_cache(None)
def _W():
    """a fixed SPD 12 x 12 shape with eigenvalues in [1, 10]"""
    Q, _ = np.linalg.qr(np.random.default_rng(71).normal(size=(12, 12)))
    A = (Q * np.linspace(1.0, 10.0, 12)) @ Q.T
    return 0.5 * (A + A.T)


def sums_for_step(d12, s=1e9, M=5000):
    """H^T H = s W much larger than A11^-1 and H^T h = H^T H d: the iteration's step comes out as d in pos, rot, offset_R, offset_T"""
    HTH = s * _W()
    return pack_sums(HTH, HTH @ np.asarray(d12, dtype=np.float64), M)


GRAV_AXIS = np.array([0.25, 1.0, -0.2]) / np.linalg.norm([0.25, 1.0, -0.2])


def ladder_sets(rungs, n_pass, seed, with_gravity=False):
    """per pass the sums that take rot and offset_R_L_I from one rung to the next about fixed axes (rotations about one axis add);
    passes beyond the ladder move the position by a millimetre, so that no pass meets the limits.  with_gravity (for cov_corr):
    the rot axis is tilted but mainly y, the component that P ties to gravity's second tangent coordinate with a regression
    coefficient of -0.99 -- G2 z then moves gravity by 0.94 of the rot step, rung by rung"""
    a1, a2 = axes(2, seed)[:2]
    if with_gravity:
        a1 = GRAV_AXIS
    sets, prev = [], 0.0
    for i in range(n_pass):
        d = np.zeros(12)
        if i < len(rungs):
            d[3:6] = (rungs[i] - prev) * a1
            d[6:9] = (rungs[i] - prev) * a2
            prev = rungs[i]
        else:
            d[0:3] = [1e-3 * (-1) ** i, 2e-3, -1e-3]
        sets.append(sums_for_step(d))
    return sets


def _case(x, P, sets, max_iter, limits=1e-12, R=0.001, D=5.0, rungs=None, mixed=None, grav_moves=False):
    part = np.array([mixed_groups(s, 80 + i) if mixed is not None and i in mixed else one_group(s) for i, s in enumerate(sets)])
    return dict(x=np.asarray(x, dtype=np.float64), P=np.asarray(P, dtype=np.float64), partials=part, max_iter=max_iter,
                limits=np.full(23, limits) if np.isscalar(limits) else np.asarray(limits, dtype=np.float64), R=R, D=D, rungs=rungs,
                grav_moves=grav_moves)


def tool_sums(seed=7, M=5000):
    """synthetic rows as tools/ieskf_bench.hip draws them: the same H^T H / H^T h in every iteration"""
    r = np.random.default_rng(seed)
    n = r.normal(size=(M, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    H = np.concatenate([n, 3.0 * r.normal(size=(M, 9))], axis=1)
    res = 0.02 * r.normal(size=M) + 0.05 * H[:, 0]
    return pack_sums(H.T @ H, H.T @ res, M), H, res


SHORT_RUNGS = (1e-6, 0.0222, 0.5, 3.0)


@functools.lru_cache(None)
def algebra_cases():
    out = {}
    st, cv = dict(states()), dict(covs())
    out["tool/tool/baseline"] = _case(st["tool"], cv["tool"], [tool_sums()[0]], 3, limits=1e-4)
    k = 0
    for sn in ("tool", "general", "general_wneg", "grav_chart"):
        for pn in ("tool", "diag", "corr"):
            k += 1
            if sn == "general_wneg" and pn != "corr":
                continue
            out[f"{sn}/{pn}/ladder4"] = _case(st[sn], cv[pn], ladder_sets(SHORT_RUNGS, 5, 90 + k, pn == "corr"), 4, rungs=SHORT_RUNGS,
                                              grav_moves=pn == "corr")
    out["general/corr/ladder11"] = _case(st["general"], cv["corr"], ladder_sets(STEP_LADDER, 12, 77, True), 11, rungs=STEP_LADDER, mixed=(0, 5),
                                         grav_moves=True)
    out["grav_chart/tool/ladder11"] = _case(st["grav_chart"], cv["tool"], ladder_sets(STEP_LADDER, 12, 78), 11, rungs=STEP_LADDER, mixed=(3,))
    out["general/corr/same_sums"] = _case(st["general"], cv["corr"], [dyadic_rows()[0]], 4)
    return out


@functools.lru_cache(None)
def dyadic_rows(seed=8, M=400):
    """(sums, H [M, 12], h [M]) with entries that are small multiples of 1/8 (H) and 1/512 (h): every product and every partial
    sum of H^T H and H^T h is exact in float64, so whoever adds the rows, in whatever order, has the bits of these sums"""
    r = np.random.default_rng(seed)
    H = np.concatenate([r.integers(-8, 9, size=(M, 3)), r.integers(-32, 33, size=(M, 9))], axis=1) / 8.0
    h = r.integers(-32, 33, size=M) / 512.0
    return pack_sums(H.T @ H, H.T @ h, M), H, h


def passes_from_rows_units(update_fixed):
    """A filter that takes dense rows and returns its final state only (api.eskf_update_fixed, the oracle's), run with max_iters =
    0, 1, ..: the state after each pass, each against one iteration of the reference from that filter's own state before it.
    Returns the worst x_after error in iteration_ref's scale -- the quantity K_HOST["iter_x"] is measured for."""
    c = algebra_cases()["general/corr/same_sums"]
    sums, H, h = dyadic_rows()
    HTH, HTh, _ = unpack_sums(sums)
    worst, xb = 0.0, c["x"]
    for p in range(c["max_iter"] + 1):
        x, _, n = update_fixed(c["x"], c["P"], H, h, max_iters=p, limits=c["limits"], R=c["R"], D=c["D"])
        assert n == p + 1
        _, xa, _, sx = iteration_ref(c, xb, HTH, HTh)
        worst = max(worst, err_units(x, xa, sx))
        xb = x
    return worst


@functools.lru_cache(None)
def host_run(name):
    from fast_limo_amd import api
    c = algebra_cases()[name]
    return api.ieskf_run_fixed_host(c["x"], c["P"], c["limits"], c["partials"], R=c["R"], D=c["D"], max_iter=c["max_iter"])


def iteration_ref(c, x_before, HTH, HTh):
    """one outer iteration of the reference from x_before: (dx_, x_after, scale of dx_, scale of x_after)"""
    xb, xp = vec(x_before), vec(c["x"])
    dx, xa, dxn, N = mp_iteration(xb, xp, to_mp_matrix(c["P"]), mp.mpf(float(c["R"])), to_mp_matrix(HTH), M(vec(HTh)))
    vn = [mp_norm(mp_so3_boxminus(xb[o:o + 4], xp[o:o + 4])) for o, _ in SO3]
    amp = 1.0 + sum(1.0 / float(v) for v in vn if v >= TOL)
    s = EPS * (float(np.linalg.cond(to_np(N))) * amp * (mp_maxabs(dx) + mp_maxabs(dxn)) + 1.0 + mp_maxabs(dxn))
    return dx, xa, s, s + EPS * mp_maxabs(xa)


def iteration_units(c, log, x_first=None):
    """worst error of the logged passes' dx and x_after against iteration_ref from the state each pass started at"""
    return iteration_units2(c, log, None, x_first)[0:2]


def iteration_units2(c, log, other, x_first=None):
    """... and, in the same scales, the worst difference to another evaluation's log of the same passes (device against host)"""
    wd = wx = bd = bx = 0.0
    xb = c["x"] if x_first is None else x_first
    for i, p in enumerate(log):
        dx, xa, sd, sx = iteration_ref(c, xb, p["HTH"], p["HTh"])
        wd = max(wd, err_units(p["dx"], dx, sd))
        wx = max(wx, err_units(p["x_after"], xa, sx))
        if other is not None:
            bd = max(bd, float(np.max(np.abs(p["dx"] - other[i]["dx"]))) / sd)
            bx = max(bx, float(np.max(np.abs(p["x_after"] - other[i]["x_after"]))) / sx)
        xb = p["x_after"]
    return wd, wx, bd, bx


def np_so3_angle(q, qp):
    d = qmul(np.array([-qp[0], -qp[1], -qp[2], qp[3]]), q)
    return 2.0 * np.arctan2(np.linalg.norm(d[0:3]), abs(d[3]))


def assert_rungs_reached(c, log):
    """after pass i, rot and offset_R_L_I are rung i from the propagated state within a factor of two -- and, in the cases with the
    correlated P, where G2 z moves it with the pose, so is the gravity direction.  (With the other covariances gravity is not
    on the ladder: the dense P moves it by 1e-2 of a rung, the diagonal P not at all.)"""
    for i, r in enumerate(c["rungs"]):
        for o in (3, 7):
            a = np_so3_angle(log[i]["x_after"][o:o + 4], c["x"][o:o + 4])
            assert 0.5 * r <= a <= 2.0 * r, (i, o, r, a)
        if c["grav_moves"]:
            a = grav_angle(log[i]["x_after"], c["x"])
            assert 0.5 * r <= a <= 2.0 * r, (i, "gravity", r, a)


def grav_angle(x, xp):
    g, gp = np.asarray(x[23:26]), np.asarray(xp[23:26])
    return float(np.arctan2(np.linalg.norm(np.cross(g, gp)), np.dot(g, gp)))


# ---- loop logic and hand-backs ----
def _host_of(c):
    from fast_limo_amd import api
    return api.ieskf_run_fixed_host(c["x"], c["P"], c["limits"], c["partials"], R=c["R"], D=c["D"], max_iter=c["max_iter"])


@functools.lru_cache(None)
def loop_cases():
    """{name: case}: a component of the first step exactly on its limit and one ulp above it (iteration -1 has x == x_prop: its step
    holds no transcendental, host and device form the same bits), every pass within the limits, no pass within them"""
    st, cv = dict(states()), dict(covs())
    base = dict(x=st["general"], P=cv["tool"], sets=[tool_sums(9)[0]], max_iter=4)
    wide = _case(limits=1e3, **base)
    dx0 = _host_of(wide)["log"][0]["dx"]
    k = 4
    on, above = np.full(23, 1e3), np.full(23, 1e3)
    on[k] = abs(dx0[k])
    above[k] = np.nextafter(abs(dx0[k]), 0.0)
    return {"t2_early": wide, "limit_on": _case(limits=on, **base), "limit_one_ulp_above": _case(limits=above, **base),
            "ends_at_max_iter": _case(limits=1e-12, **base)}


def _pose_block_sums(lam_min, D):
    Q, _ = np.linalg.qr(np.random.default_rng(91).normal(size=(6, 6)))
    HTH = np.zeros((12, 12))
    A = (Q * np.array([lam_min, 50.0, 60.0, 70.0, 80.0, 90.0])) @ Q.T
    HTH[0:6, 0:6] = 0.5 * (A + A.T)
    HTH[6:12, 6:12] = 1e3 * np.eye(6)
    return pack_sums(HTH, HTH @ np.full(12, 1e-3), 5000)


@functools.lru_cache(None)
def handback_cases():
    st, cv = dict(states()), dict(covs())
    lad = ladder_sets(SHORT_RUNGS, 5, 95)
    few = tool_sums(9)[0].copy()
    few[90] = 22.0
    few2 = [lad[0], lad[1], lad[2].copy(), lad[3], lad[4]]
    few2[2][90] = 22.0
    Pz = cv["tool"].copy()
    Pz[0, :] = 0.0
    Pz[:, 0] = 0.0
    Hz, hz, _ = unpack_sums(tool_sums(9)[0])
    Hz[0, :] = 0.0
    Hz[:, 0] = 0.0
    D = 5.0
    return {
        "few_at_0": _case(st["general"], cv["tool"], [few], 3, mixed=(0,)),
        "few_at_2": _case(st["general"], cv["corr"], few2, 4, mixed=(2,)),
        "eig_0.9D": _case(st["general"], cv["tool"], [_pose_block_sums(0.9 * D, D)], 3, D=D),
        "eig_1.1D": _case(st["general"], cv["tool"], [_pose_block_sums(1.1 * D, D)], 3, D=D),
        "zero_pivot": _case(st["general"], Pz, [pack_sums(Hz, hz, 5000)], 3),
        "bad_tags": _case(st["general"], cv["tool"], [tool_sums(9)[0]], 3),
    }


