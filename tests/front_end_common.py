"""Shared helpers of the sweep front end's tests (input filter, time order, deskew, voxel grid): input builders and plain references.

References
  filter_reference   numpy restatement of the reference's input stage (Localizer.cpp:262-302: NaN removal, negative crop box, rank
                     among the survivors % rate, FoV, min distance; :741-805: the four stamp decodings, the time sort, the stamp of
                     the point sorted last).
  deskew_f64         float64 restatement of one point of deskewPointCloud (Localizer.cpp:825-839) from the formulas of
                     State::update (State.cpp:76-119): Rodrigues rotation, quaternion product, p + v dt + a0 dt^2 / 2.  Independent of
                     the oracle's float32 restatement; DESKEW_F64_RATIO is the oracle's measured distance from it.
  voxel_reference    pcl::VoxelGrid with an int64 lattice and per-voxel float32 sums in ascending point index.
"""
import ctypes
import ctypes.util

import numpy as np

from fast_limo_amd._lib import FRAME_DTYPE

F32 = np.float32
INT_MAX = 2**31 - 1
TILE = 2048                      # points per tile of the one-launch filter (flimo_map.hip: FILT_TILE)
N_MAX = 266277                   # 130 full tiles + one of 37 points: three look-back rounds, the last one partly filled

# Worst |oracle float32 - float64 reference| of a deskewed point over every input of deskew_case(), in units of
# 2^-24 * (|p| + |frame p| + |v| |dt| + |a0| dt^2 / 2 + |L2B t| + |last p|), as test_front_end_host measures it (it asserts 4x
# this value; the inputs are fixed seeds, the margin only lets a seed change).  The GPU inherits the bound through bit equality
# with the oracle.
DESKEW_F64_RATIO = 7.95


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# input filter + stamps
# ---------------------------------------------------------------------------------------------------------------------------------
_LIBM = None


def atan2f_host(y, x):
    """atan2f of THIS host's libm, element by element (the FoV filter's verdict is defined by it, Localizer.cpp:873-876)."""
    global _LIBM
    if _LIBM is None:
        _LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _LIBM.atan2f.restype = ctypes.c_float
        _LIBM.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
    y = np.asarray(y, F32).reshape(-1)
    x = np.asarray(x, F32).reshape(-1)
    return np.array([_LIBM.atan2f(float(a), float(b)) for a, b in zip(y, x)], F32)


def filter_cfg(**kw):
    """A flimo_filter_cfg as a dict (the keyword arguments of HipCtx.raw_scan_filter_order_set), every filter off by default."""
    cfg = dict(crop_active=0, crop_min=(-1.0, -1.0, -1.0), crop_max=(1.0, 1.0, 1.0), dist_active=0, min_dist=0.0, rate_active=0,
               rate_value=1, time_kind=1, end_of_sweep=0, sweep_ref_time=0.0, fov_active=0, fov_angle=3.14159265)
    unknown = set(kw) - set(cfg)
    assert not unknown, unknown
    cfg.update(kw)
    return cfg


def filter_reference(xyz, tw, cfg):
    """The input stage on the host.  ``xyz`` [n, 3] float32; ``tw`` the time field of the configured sensor: uint32 (time_kind 0,
    OUSTER ns), float32 (1, VELODYNE s) or float64 (2 HESAI s, 3 LIVOX ns).  Returns a dict: keep (mask over the input), xyz and
    stamps of the kept points in arrival order, order (time rank -> position among the kept points: the stable sort of the sort
    key), n_kept, last_stamp (extract(sorted.back()); 0.0 when nothing is kept or a stamp is NaN, as the call reports it),
    nan_stamp, tied."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    kind, eos, ref = int(cfg["time_kind"]), bool(cfg["end_of_sweep"]), float(cfg["sweep_ref_time"])
    tw = np.asarray(tw, (np.uint32, F32, np.float64, np.float64)[kind]).reshape(-1)
    assert tw.shape[0] == xyz.shape[0]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    alive = np.isfinite(xyz).all(axis=1)                                            # removeNaNFromPointCloud
    if cfg["crop_active"]:                                                          # negative crop box: on a face is inside
        mn, mx = np.asarray(cfg["crop_min"], F32), np.asarray(cfg["crop_max"], F32)
        with np.errstate(invalid="ignore"):
            outside = (xyz < mn).any(axis=1) | (xyz > mx).any(axis=1)
        alive &= outside
    keep = alive.copy()
    if cfg["rate_active"]:                                                          # index among the survivors of the crop
        rank = np.cumsum(alive) - 1
        keep &= (rank % int(cfg["rate_value"])) == 0
    if cfg["fov_active"]:
        idx = np.flatnonzero(keep)
        keep[idx] = np.abs(atan2f_host(y[idx], x[idx])) < F32(cfg["fov_angle"])
    if cfg["dist_active"]:
        with np.errstate(invalid="ignore", over="ignore"):
            keep &= np.sqrt(x * x + (y * y + z * z)) > F32(cfg["min_dist"])           # float32, strict
    kt = tw[keep]
    # the four stamp decodings (Localizer.cpp:745-781) and the key the time sort compares
    if kind == 0:
        rel = (kt.astype(F32) * F32(1e-9)).astype(np.float64)                       # pt.t * 1e-9f: a float product
        stamps = ref - rel if eos else ref + rel
        key = -kt.astype(np.int64) if eos else kt.astype(np.int64)
    elif kind == 1:
        rel = kt.astype(np.float64)
        stamps = ref - rel if eos else ref + rel
        key = -kt if eos else kt
    else:
        stamps = kt.copy() if kind == 2 else kt * np.float64(F32(1e-9))             # pt.timestamp * 1e-9f: a double product
        key = kt
    n_kept = int(keep.sum())
    nan_stamp = int(kind != 0 and bool(np.isnan(kt).any()))
    out = dict(keep=keep, xyz=xyz[keep], stamps=stamps, n_kept=n_kept, nan_stamp=nan_stamp, tied=0, last_stamp=0.0,
               order=np.zeros(0, np.uint32))
    if n_kept == 0 or nan_stamp:
        return out
    order = np.argsort(key, kind="stable")
    ks = key[order]
    out["order"] = order.astype(np.uint32)
    out["tied"] = int(bool((ks[1:] == ks[:-1]).any()))
    out["last_stamp"] = float(stamps[order[-1]])
    return out


def records32(xyz, tw, kind):
    """The sweep as the reference's 32-byte PointType records."""
    import oracle_py
    if kind == 0:
        return oracle_py.make_points(xyz, 1.0, t_ns=np.asarray(tw, np.uint32))
    if kind == 1:
        return oracle_py.make_points(xyz, 1.0, time_s=np.asarray(tw, F32))
    return oracle_py.make_points(xyz, 1.0, timestamp=np.asarray(tw, np.float64))


def records16(xyz, tw, kind):
    """The sweep as 16-byte {x, y, z, 32-bit time word} records (time_order bit 2; OUSTER and VELODYNE only)."""
    assert kind in (0, 1)
    rec = np.zeros((np.asarray(xyz).shape[0], 4), F32)
    rec[:, :3] = xyz
    rec.view(np.uint32)[:, 3] = np.asarray(tw, np.uint32) if kind == 0 else bits(np.asarray(tw, F32))
    return rec


def sweep(n, seed, scale=30.0):
    """n sensor-like points (a flat box of +-scale m) and pairwise different VELODYNE stamps in arrival-shuffled order."""
    rs = np.random.RandomState(seed)
    xyz = (rs.uniform(-scale, scale, (n, 3)) * [1, 1, 0.1]).astype(F32)
    rel = ((rs.permutation(n) + 0.25) * (0.1 / max(n, 1))).astype(F32)
    return xyz, rel


def big_sweep(variant):
    """The 266 277-point sweep of the look-back test: tiles 5, 64 and 129 entirely NaN, tile 70 entirely inside the crop box
    (+-2 m); variant "last" / "first": only points of the last / the first tile lie beyond the min distance of 5 m."""
    xyz, rel = sweep(N_MAX, 17)
    rs = np.random.RandomState(18)
    if variant in ("last", "first"):
        near = (rs.uniform(-2.5, 2.5, (N_MAX, 3))).astype(F32)                      # |p| <= 4.34 < 5: dropped by the distance
        sl = slice(130 * TILE, N_MAX) if variant == "last" else slice(0, TILE)
        near[sl] = xyz[sl]
        xyz = near
    for t in (5, 64, 129):
        xyz[np.arange(t * TILE, (t + 1) * TILE), rs.randint(0, 3, TILE)] = np.nan
        xyz[t * TILE, :] = np.inf
    xyz[70 * TILE:71 * TILE] = rs.uniform(-2.0, 2.0, (TILE, 3)).astype(F32)
    return xyz, rel


REST_X26 = np.zeros(26)
REST_X26[6] = REST_X26[10] = 1.0
REST_X26[25] = -9.81


def rest_frames(t0, nf=2):
    """IMU frames of a body at rest at the origin (the specific force cancels gravity exactly): with an identity lidar2baselink_T
    the deskew returns every point as it is; with stamp_readback_l2b() and velocity (1, 0, 0) it returns float32(stamp - t0)."""
    fr = np.zeros(nf, FRAME_DTYPE)
    fr["q"][:, 3] = 1.0
    fr["g"][:, 2] = -9.81
    fr["a"][:, 2] = 9.81
    fr["time"] = t0 + 1000.0 * np.arange(nf)
    return fr


def stamp_readback_frames(t0):
    fr = rest_frames(t0, 1)
    fr["v"][:, 0] = 1.0
    return fr


def stamp_readback_l2b():
    """lidar2baselink_T with a zero rotation block: T * [p, 1] is the frame's position, whatever the point."""
    m = np.zeros((4, 4), F32)
    m[3, 3] = 1.0
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# deskew
# ---------------------------------------------------------------------------------------------------------------------------------
NF_CASES = (1, 2, 3, 72, 73, 500)
N_DESKEW = 4096
EDGE_DT = (0.1, 0.11, 0.155, 0.16, 0.3)          # x 20 rad/s: 2.0, 2.2, 3.1, 3.2 and 6.0 rad before the first / after the last frame
EDGE_RATE = 20.0
THR = F32(1e-7)                                   # as a double 1.00000001e-7 > 1e-7: the reference compares the float as a double
ANGLES = (0.0, "lo", "hi", "thr", 0.01, 2.0, 2.2, 3.1, 3.2, 6.0)      # w_norm * dt of a frame's points at 63/64 of its interval
# mainly x, mainly y, mainly z and the diagonal, then the first three reversed: tilted, because about a pure axis the off-diagonal
# sums the quaternion-from-matrix branches use are all zero and a slip in them would not show
_U = [np.array(a, np.float64) / np.linalg.norm(a) for a in ((1, 0.3, -0.2), (0.25, 1, 0.35), (-0.3, 0.2, 1), (1, 1, 1))]
AXES = tuple(tuple(a) for a in _U) + tuple(tuple(-a) for a in _U[:3])
FRAME_T0 = 1.7e9 + 0.25


def _unit_quat(rs):
    q = rs.normal(size=4)
    return q / np.linalg.norm(q)


def _quat_to_rot64(q):
    x, y, z, w = (np.float64(c) for c in q)
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])


def _exact_norm_x(target):
    """A float32 x with sqrt(x * x) == target in float32 arithmetic."""
    for x in (target, np.nextafter(target, F32(1)), np.nextafter(target, F32(0))):
        if np.sqrt(F32(x * x)) == target:
            return F32(x)
    raise AssertionError("no float32 x whose norm is the threshold")


def deskew_frames(nf, case_idx, seed):
    """nf IMU frames, h apart, non-identity attitude and non-zero v, a, ba, bg, g; frame k turns about AXES[k % 7] at the rate that
    makes ANGLES[k % 10] at 63/64 of its interval; the first and the last frame turn at EDGE_RATE about the case's own axes."""
    rs = np.random.RandomState(seed)
    h = 1e-3 if nf >= 72 else 0.05
    fr = np.zeros(nf, FRAME_DTYPE)
    fr["time"] = FRAME_T0 + h * np.arange(nf)
    for k in range(nf):
        fr["p"][k] = rs.uniform(-20, 20, 3)
        fr["q"][k] = _unit_quat(rs)
        fr["v"][k] = rs.uniform(-5, 5, 3)
        fr["g"][k] = (0.1, -0.2, -9.79)
        fr["a"][k] = rs.uniform(-3, 3, 3) + [0, 0, 9.8]
        fr["ba"][k] = rs.uniform(-0.1, 0.1, 3)
        bg = rs.uniform(-0.01, 0.01, 3).astype(F32)
        ang, axis = ANGLES[k % len(ANGLES)], np.array(AXES[k % len(AXES)])
        if k == 0:
            w = np.array(AXES[case_idx % 4]) * EDGE_RATE
        elif k == nf - 1:
            w = np.array(AXES[(case_idx + 1) % 4]) * EDGE_RATE
        elif isinstance(ang, str):
            bg[:] = 0                                                                # w - bg is then w, exactly
            mag = {"lo": F32(0.9e-7), "hi": F32(1.1e-7), "thr": _exact_norm_x(THR)}[ang]
            w = np.zeros(3, F32)
            w[k % 3] = mag if (k // 3) % 2 == 0 else -mag
        else:
            w = axis * (ang / (h * 63.0 / 64.0))
        fr["bg"][k] = bg
        fr["w"][k] = (np.asarray(w, F32) + bg).astype(F32)
    return fr, h


def deskew_case(nf, with_far_frame=False):
    """One deskew input: N_DESKEW points, their stamps (sorted), nf frames, lidar2baselink_T with rotation and translation, a
    rotated and translated last state.  Stamps: before the first frame by up to 0.3 s, equal to every frame's time once, between
    frames (half of them at 63/64 of the interval), after the last frame by up to 0.3 s.  ``with_far_frame`` appends one frame
    10 s later that no stamp reaches (the nf = 73 case is the nf = 72 case with it)."""
    case_idx = NF_CASES.index(nf)
    rs = np.random.RandomState(100 + nf)
    fr, h = deskew_frames(nf, case_idx, 200 + nf)
    n = N_DESKEW
    xyz = (rs.uniform(-50, 50, (n, 3)) * [1, 1, 0.1]).astype(F32)
    ft = fr["time"]
    before = ft[0] - np.concatenate([np.tile(EDGE_DT, 8), rs.uniform(1e-4, 0.3, 24)])
    after = ft[-1] + np.concatenate([np.tile(EDGE_DT, 8), rs.uniform(1e-4, 0.3, 24)])
    equal = ft.copy()
    m = n - before.size - after.size - equal.size
    k = rs.randint(0, nf, m)
    f = np.where(np.arange(m) % 2 == 0, 63.0 / 64.0, rs.uniform(0, 1, m))
    if nf == 1:
        f = f * (0.3 / h)                                                            # one frame: its "interval" is the 0.3 s after it
    between = ft[k] + f * h
    t = np.concatenate([before, equal, between, after])
    o = np.argsort(t, kind="stable")
    t = np.ascontiguousarray(t[o])
    if with_far_frame:
        far = fr[-1:].copy()
        far["time"] += 10.0
        far["p"] += 3.0
        fr = np.concatenate([fr, far])
    L2B = np.eye(4, dtype=F32)
    L2B[:3, :3] = _quat_to_rot64(_unit_quat(rs)).astype(F32)
    L2B[:3, 3] = (0.3, -0.2, 0.5)
    x26 = REST_X26.copy()
    x26[0:3] = (12.5, -7.25, 1.5)
    x26[3:7] = _unit_quat(rs)
    return dict(xyz=xyz, t=t, frames=np.ascontiguousarray(fr), L2B=L2B, x26=x26, h=h)


def deskew_cases():
    """{nf: input} for NF_CASES; 73 is 72 with the far frame."""
    out = {nf: deskew_case(nf) for nf in NF_CASES if nf != 73}
    out[73] = deskew_case(72, with_far_frame=True)
    return out


def deskew_f64(case):
    """float64 deskew of every point of a case from the formulas of State.cpp:76-119 (no float32 step, no threshold on |w|: the
    exact rotation by |w| dt).  Returns body [n, 3], world [n, 3], and per point the update rotation's trace and diagonal (which
    quaternion-from-matrix branch the float32 code takes), dt, and the scale of the error bound
    |p| + |frame p| + |v| |dt| + |a0| dt^2 / 2 + |L2B t| + |last p|."""
    fr, t = case["frames"], case["t"]
    xyz = case["xyz"].astype(np.float64)
    L2B = case["L2B"].astype(np.float64)
    # the frame of a stamp: the last one not after it, the first one for a stamp before them all (Algorithms.hpp:25-38)
    i_f = np.clip(np.searchsorted(fr["time"], t, side="right") - 1, 0, None)
    last_p = case["x26"][0:3].astype(F32).astype(np.float64)
    last_R = _quat_to_rot64(case["x26"][3:7].astype(F32))
    n = xyz.shape[0]
    body, world = np.empty((n, 3)), np.empty((n, 3))
    tr, diag, dts, scale = np.empty(n), np.empty((n, 3)), np.empty(n), np.empty(n)
    for i in range(n):
        F = fr[i_f[i]]
        dt = t[i] - F["time"]
        w = F["w"].astype(np.float64) - F["bg"].astype(np.float64)
        wn = np.linalg.norm(w)
        R = np.eye(3)
        if wn > 0:
            r = w / wn
            K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
            ang = wn * dt
            R = R + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)
        Rq = _quat_to_rot64(F["q"])
        a0 = Rq @ (F["a"].astype(np.float64) - F["ba"].astype(np.float64)) + F["g"].astype(np.float64)
        Rn = Rq @ R                                                                   # q *= Quaternionf(R)
        v = F["v"].astype(np.float64)
        pn = F["p"].astype(np.float64) + v * dt + 0.5 * a0 * dt * dt
        pw = Rn @ (L2B[:3, :3] @ xyz[i] + L2B[:3, 3]) + pn
        world[i] = pw
        body[i] = last_R.T @ (pw - last_p)
        tr[i], diag[i], dts[i] = np.trace(R), np.diag(R), dt
        scale[i] = (np.linalg.norm(xyz[i]) + np.linalg.norm(F["p"].astype(np.float64)) + np.linalg.norm(v) * abs(dt) +
                    0.5 * np.linalg.norm(a0) * dt * dt + np.linalg.norm(L2B[:3, 3]) + np.linalg.norm(last_p))
    return dict(body=body, world=world, trace=tr, diag=diag, dt=dts, scale=scale, i_f=i_f)


def quat_branches(ref, margin=1e-3):
    """Points per quaternion-from-matrix branch of deskew_world -- [tr > 0, largest diagonal x, y, z] -- counting only points that
    lie ``margin`` away from the branch boundaries (float32 cannot flip them)."""
    tr, d = ref["trace"], ref["diag"]
    s = np.sort(d, axis=1)
    clear = (tr < -margin) & (s[:, 2] - s[:, 1] > margin)
    i = np.argmax(d, axis=1)
    return [int((tr > margin).sum())] + [int((clear & (i == a)).sum()) for a in range(3)]


# ---------------------------------------------------------------------------------------------------------------------------------
# voxel grid
# ---------------------------------------------------------------------------------------------------------------------------------
LEAVES = (0.1, 0.25, 1.0)
VOXEL_NS = (1, 2, 7, 8, 9, 255, 256, 257, 4099)
NONFINITE = np.array([[np.nan, 1, 2], [3, np.inf, 1], [-np.inf, np.nan, 0]], F32)


def voxel_reference(xyz, leaf):
    """pcl::VoxelGrid: centroid per occupied voxel (float32 sums in ascending point index), ascending voxel index; the lattice in
    int64: wherever the product of the three division counts exceeds INT_MAX (or a floor does not fit an int) the input comes
    back unchanged; no finite point: empty."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    inv = F32(1.0) / F32(leaf)
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return np.zeros((0, 3), F32)
    p = xyz[fin]
    with np.errstate(over="ignore"):
        fl, fh = np.floor(p.min(axis=0) * inv), np.floor(p.max(axis=0) * inv)
    if not (np.all(np.abs(fl) < F32(2.0**31)) and np.all(np.abs(fh) < F32(2.0**31))):
        return xyz.copy()
    lo = fl.astype(np.int64)
    div = fh.astype(np.int64) - lo + 1
    if int(div[0]) * int(div[1]) * int(div[2]) > INT_MAX:
        return xyz.copy()
    ijk = (np.floor(p * inv) - lo.astype(F32)).astype(np.int64)                      # (int)(floor(x * inv) - (float)min_b)
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    o = np.argsort(key, kind="stable")
    ks = key[o]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], ks.size]
    out = np.empty((starts.size, 3), F32)
    for v, (a, b) in enumerate(zip(starts, ends)):
        out[v] = np.cumsum(p[o[a:b]], axis=0, dtype=F32)[-1] / F32(b - a)             # cumsum: one float32 add after the other
    return out


def voxel_scan(n, leaf, seed):
    """n points with negative coordinates; every fourth one exactly on a voxel face (k * leaf as float32 rounds it)."""
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-6, 6, (n, 3)).astype(F32)
    on_face = (rs.randint(-40, 40, (n, 3)).astype(F32) * F32(leaf)).astype(F32)
    sel = np.arange(n) % 4 == 3
    xyz[sel] = on_face[sel]
    return xyz


def voxel_one_cell(n=4099):
    return np.random.RandomState(7).uniform(0.01, 0.09, (n, 3)).astype(F32)


def voxel_tail_run(m, n_nonfinite, base=300, seed=3):
    """base points below 5 m on every axis, then m points inside the voxel at (5, 5, 5) -- the largest key, the last run of the
    sorted keys -- then n_nonfinite non-finite points."""
    rs = np.random.RandomState(seed)
    lo = rs.uniform(-5, 4.9, (base, 3)).astype(F32)
    lo[0] = (-5, -5, -5)
    top = (5.0 + rs.uniform(0.0, 0.09, (m, 3))).astype(F32)
    top[0] = (5.0, 5.0, 5.0)
    return np.ascontiguousarray(np.concatenate([lo, top, NONFINITE[:n_nonfinite]]).astype(F32))


def voxel_passthrough_inputs():
    """(name, scan, leaf): lattices beyond INT_MAX cells.  "product": four corners spanning 2 000 m on every axis at leaf 0.1 --
    20 001 divisions per axis, each fits, the product does not.  "axis": x = +-1.2e9 m at leaf 1 -- one axis of 2.4e9 cells, which an
    int difference wraps -- with three more points sharing one voxel; the same at +-1.2e7 m and leaf 0.01.  "floor": x / leaf beyond
    2^31 itself."""
    corners = np.array([[-1000, -1000, -1000], [1000, 1000, 1000], [1000, -1000, 1000], [-1000, 1000, -1000]], F32)
    three = np.array([[0.2, 0.3, 0.4], [0.25, 0.35, 0.45], [0.3, 0.3, 0.3]], F32)
    return [
        ("product", np.concatenate([corners[:2], NONFINITE[:2], corners[2:], three]), 0.1),
        ("axis", np.concatenate([np.array([[-1.2e9, 0, 0]], F32), three, NONFINITE[:1], np.array([[1.2e9, 0.5, 0.5]], F32)]), 1.0),
        ("axis-small-leaf", np.concatenate([np.array([[-1.2e7, 0, 0]], F32), three * F32(0.01), np.array([[1.2e7, 0.005, 0.005]], F32)]), 0.01),
        ("floor", np.concatenate([three, np.array([[3.0e9, 0, 0]], F32)]), 1.0),
    ]


def voxel_inputs():
    """Every (name, scan, leaf) of the voxel-grid tests that is NOT a pass-through."""
    out = []
    for leaf in LEAVES:
        for n in VOXEL_NS:
            out.append((f"n{n}-leaf{leaf}", voxel_scan(n, leaf, 1000 + n), leaf))
        out.append((f"one-cell-leaf{leaf}", voxel_one_cell(), leaf))
    with_nan = voxel_scan(257, 0.25, 5)
    with_nan[[0, 100, 256]] = NONFINITE
    out.append(("nan-inside", with_nan, 0.25))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# stamps and ties
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_REF = 1.7e9 + 0.5          # a present-day epoch: neighbouring doubles lie 2.4e-7 s apart, far more than a float32 of the 0.1 s
                                 # after it resolves, so float32(stamp - SWEEP_REF) tells any two of them apart
N_STAMPS = 600


def one_tie(rel, where):
    """The stamps with the one of sorted rank ``where + 1`` made equal to its predecessor's: exactly one equal pair."""
    rel = rel.copy()
    o = np.argsort(rel, kind="stable")
    rel[o[where + 1]] = rel[o[where]]
    return rel


def stamp_cases():
    """[dict(name, kind, eos, ref, xyz, tw)]: every time_kind, start and end of sweep where the reference has both, the extremes of
    each decoding, and the tie layouts."""
    n = N_STAMPS
    xyz, rel = sweep(n, 31)
    perm = np.random.RandomState(32).permutation(n)
    cases = []

    def add(name, kind, eos, tw, ref=SWEEP_REF, pts=None):
        cases.append(dict(name=name, kind=kind, eos=eos, ref=ref, xyz=xyz[:len(tw)] if pts is None else pts, tw=tw))

    t_ns = (perm.astype(np.uint32) * np.uint32(150000) + np.uint32(7))
    for eos in (0, 1):
        add(f"ouster-unique-eos{eos}", 0, eos, t_ns)
        add(f"ouster-all-zero-eos{eos}", 0, eos, np.zeros(n, np.uint32))
        big = t_ns.copy(); big[n // 3] = 0xffffffff
        add(f"ouster-one-max-eos{eos}", 0, eos, big)
        add(f"ouster-all-max-eos{eos}", 0, eos, np.full(n, 0xffffffff, np.uint32))   # the point sorted last carries it either way
        add(f"velodyne-unique-eos{eos}", 1, eos, rel)
        # signed zeros (a tie), negative and denormal stamps; the largest and the smallest stamp are ordinary numbers
        odd = rel.copy()
        odd[0:8] = [-0.0, 0.0, 1e-45, 3e-45, -1e-45, -3e-45, 1e-39, -1e-39]
        odd[8:40] = -odd[8:40]
        add(f"velodyne-zeros-denormals-eos{eos}", 1, eos, odd)
        nozero = odd.copy(); nozero[0] = F32(0.05)
        add(f"velodyne-denormals-no-tie-eos{eos}", 1, eos, nozero)
        nan = rel.copy(); nan[n // 2] = np.nan
        add(f"velodyne-one-nan-eos{eos}", 1, eos, nan)
        add(f"velodyne-all-equal-eos{eos}", 1, eos, np.full(n, F32(0.0625)))
        add(f"velodyne-tie-255-256-eos{eos}", 1, eos, one_tie(rel, 255))
        add(f"velodyne-tie-last-pair-eos{eos}", 1, eos, one_tie(rel, n - 2))
        add(f"velodyne-one-point-eos{eos}", 1, eos, rel[:1])
        add(f"velodyne-two-points-eos{eos}", 1, eos, rel[:2])
        add(f"velodyne-two-equal-points-eos{eos}", 1, eos, np.array([0.03, 0.03], F32))
    rel64 = (perm + 0.25) * (0.1 / n)
    add("hesai-unique", 2, 0, SWEEP_REF + rel64)
    add("hesai-unique-eos-flag", 2, 1, SWEEP_REF + rel64)                           # end_of_sweep does not enter this decoding
    neg = rel64 - 0.05
    neg[5] = -0.0; neg[6] = 0.0
    add("hesai-negative-and-signed-zeros", 2, 0, neg, ref=0.0)
    add("hesai-tie-255-256", 2, 0, one_tie(SWEEP_REF + rel64, 255))
    add("hesai-one-nan", 2, 0, np.where(np.arange(n) == 17, np.nan, SWEEP_REF + rel64))
    add("livox-unique", 3, 0, (SWEEP_REF + rel64) * 1e9)
    lneg = (rel64 - 0.05) * 1e9
    lneg[5] = -0.0; lneg[6] = 0.0
    add("livox-negative-and-signed-zeros", 3, 0, lneg, ref=0.0)
    add("livox-tie-last-pair", 3, 0, one_tie((SWEEP_REF + rel64) * 1e9, n - 2))
    return cases
