"""Scan Context (flimo_scan_context / flimo_sc_db_* / flimo_sc_match, include/flimo_c.h) restated in numpy, shared by
tests/test_sc_host.py and tests/test_gpu_sc.py: the bin of a point, the descriptor, the normalised columns, the distance at every
shift with its fmaf chains and its 64-slot tree, the orders (bits of d, s) and (bits of dist, id), and the scene of the method's
test.  float32 throughout; fmaf is tests/desc_common.py's, atan2f this host's libm (tests/front_end_common.py)."""
import functools
import math

import numpy as np

from desc_common import bits, fmaf
from front_end_common import atan2f_host

F = np.float32
SLOTS = 64
TWO_PI_F = F(float.fromhex("0x1.921fb6p+2"))
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
SHAPES = ((20, 60), (32, 64), (1, 2))


def cfg(rings=20, sectors=60, min_range=0.0, max_range=80.0, z_offset=2.0):
    """A flimo_sc_cfg as a dict (the keyword arguments of HipCtx.scan_context)."""
    return dict(rings=int(rings), sectors=int(sectors), min_range=float(F(min_range)), max_range=float(F(max_range)), z_offset=float(F(z_offset)))


def scales(c):
    """(rscale, sscale): the double quotient rounded to float32 once."""
    return F(float(c["rings"]) / float(F(c["max_range"]))), F(float(c["sectors"]) / 6.283185307179586)


# ---- the descriptor -----------------------------------------------------------------------------------------------------------------
def bins(pts, c, frame12=None, atan2=atan2f_host):
    """sc_bin of every point: (has [n] bool, ring [n], sector [n], h [n] float32); ring = sector = -1, h = 0 where has is False."""
    p = np.asarray(pts, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        if frame12 is not None:
            f = np.asarray(frame12, F).reshape(3, 4)
            v = [(f[a, 0] * x + (f[a, 1] * y + (f[a, 2] * z + f[a, 3]).astype(F)).astype(F)).astype(F) for a in range(3)]
        else:
            v = [x, y, z]
        vx, vy, vz = v
        fin = np.isfinite(vx) & np.isfinite(vy) & np.isfinite(vz)
        sx, sy = np.where(fin, vx, F(1)), np.where(fin, vy, F(1))
        r = np.sqrt(((sx * sx).astype(F) + (sy * sy).astype(F)).astype(F)).astype(F)
        has = fin & (r > 0) & (r >= F(c["min_range"])) & (r < F(c["max_range"]))
        rscale, sscale = scales(c)
        ring = np.minimum(c["rings"] - 1, np.where(has, (r * rscale).astype(F), F(0)).astype(np.int64))
        a = atan2(sy, sx).astype(F)
        a = np.where(a < 0, (a + TWO_PI_F).astype(F), a)
        sector = np.minimum(c["sectors"] - 1, (a * sscale).astype(F).astype(np.int64))
        h = (np.where(fin, vz, F(0)) + F(c["z_offset"])).astype(F)
        has &= h > 0
    return has, np.where(has, ring, -1).astype(np.int32), np.where(has, sector, -1).astype(np.int32), np.where(has, h, F(0)).astype(F)


def descriptor(pts, c, frame12=None):
    """flimo_scan_context restated: (desc [rings, sectors] float32, used)."""
    has, ring, sector, h = bins(pts, c, frame12)
    desc = np.zeros((c["rings"], c["sectors"]), F)
    np.maximum.at(desc, (ring[has], sector[has]), h[has])
    return desc, int(has.sum())


# ---- the match ----------------------------------------------------------------------------------------------------------------------
def descs(D):
    D = np.ascontiguousarray(D, F)
    return D.reshape(1, *D.shape) if D.ndim == 2 else D


def normalise(D):
    """(u [n, rings, sectors] float32, valid [n, sectors] bool): n_j = sqrt of the ascending fmaf chain of the column's squares; a
    column is valid iff n_j > 0 and its descriptor has no non-finite entry; u = D / n_j there, +0 elsewhere."""
    D = descs(D)
    with np.errstate(all="ignore"):
        c = np.zeros((D.shape[0], D.shape[2]), F)
        for t in range(D.shape[1]):
            c = fmaf(D[:, t, :], D[:, t, :], c)
        nrm = np.sqrt(c).astype(F)
        valid = (nrm > 0) & np.isfinite(D).all(axis=(1, 2))[:, None]
        u = np.where(valid[:, None, :], (D / np.where(valid, nrm, F(1))[:, None, :]).astype(F), F(0)).astype(F)
    return u, valid


def slot_tree32(v):
    """The pairwise tree over the 64 slots (last axis) in float32: ((v0 + v1) + (v2 + v3)) + ..."""
    v = np.asarray(v, F)
    assert v.shape[-1] == SLOTS
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(F)
    return v[..., 0]


def fmaf_quick(a, b, c):
    """fmaf by desc_common.chain_matrix's cheaper route: the float64 a * b + c (the product exact, the sum rounded once) casts to
    the correctly rounded float32 unless that rounding landed exactly half-way between two float32 (or below float32's normal
    range); only those elements go through fmaf itself.  tests/test_sc_host.py compares the two."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = s.astype(F)
        cand = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | ((np.abs(s) < 2.0 ** -120) & (s != 0)) | ~np.isfinite(s)
    if cand.any():
        out[cand] = fmaf(a[cand], b[cand], c[cand])
    return out


def profiles(Q, E, min_cols=1):
    """d(s) of every (query, entry, shift): [nq, ne, sectors] float32, NaN where the shift is excluded."""
    uq, vq = normalise(Q)
    ue, ve = normalise(E)
    nq, R, S = uq.shape
    ne = ue.shape[0]
    out = np.full((nq, ne, S), np.nan, F)
    if ne == 0:
        return out
    sh = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S      # sh[s, j] = (j + s) % S
    for i in range(nq):
        c = np.zeros((S, ne, S), F)                                # [shift, entry, column]
        for t in range(R):
            c = fmaf_quick(uq[i, t][sh][:, None, :], ue[None, :, t, :], c)
        both = vq[i][sh][:, None, :] & ve[None, :, :]
        term = np.zeros((S, ne, SLOTS), F)
        term[:, :, :S] = np.where(both, c, F(0))
        m = both.sum(axis=2)
        with np.errstate(all="ignore"):
            d = (F(1) - (slot_tree32(term) / m.astype(F)).astype(F)).astype(F)
        d = np.where(d < 0, F(0), d).astype(F)
        out[i] = np.where((m >= min_cols) & (m > 0), d, F(np.nan)).T
    return out


def pair_best(P):
    """(have, dist, shift) of profiles P [.., sectors]: the first d(s) in the order (bits of d, s)."""
    P = np.asarray(P, F)
    S = P.shape[-1]
    key = (bits(P).astype(np.uint64) << np.uint64(6)) | np.arange(S, dtype=np.uint64)
    key = np.where(np.isnan(P), NONE, key)
    best = key.min(axis=-1)
    have = best != NONE
    dist = np.where(have, best >> np.uint64(6), 0).astype(np.uint32).view(F)
    shift = np.where(have, (best & np.uint64(63)).astype(np.int64), -1).astype(np.int32)
    return have, dist, shift


def match(Q, E, k=1, min_cols=1, max_dist=np.inf, first=0, n=None, P=None):
    """flimo_sc_match restated: dict idx / dist / shift [nq, k], cnt [nq], profile [nq, k, sectors].  P: profiles(Q, E, min_cols)
    where the caller has them."""
    Q, E = descs(Q), descs(E)
    nq, S = Q.shape[0], Q.shape[2]
    P = profiles(Q, E, min_cols) if P is None else P
    lo = min(int(first), E.shape[0])
    hi = E.shape[0] if n is None else min(lo + int(n), E.shape[0])
    have, dist, shift = pair_best(P[:, lo:hi])
    have = have & (dist < F(max_dist))
    ids = np.arange(lo, hi, dtype=np.uint64)
    key = np.where(have, (bits(dist).astype(np.uint64) << np.uint64(32)) | ids[None, :], NONE)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    out = dict(idx=np.full((nq, k), -1, np.int32), dist=np.zeros((nq, k), F), shift=np.full((nq, k), -1, np.int32),
               cnt=np.zeros(nq, np.int32), profile=np.full((nq, k, S), np.nan, F))
    for i in range(nq):
        for j, e in enumerate(order[i]):
            if key[i, e] == NONE:
                break
            out["idx"][i, j], out["dist"][i, j], out["shift"][i, j] = lo + e, dist[i, e], shift[i, e]
            out["profile"][i, j] = P[i, lo + e]
            out["cnt"][i] = j + 1
    return out


def same(got, want, tag, profile=True):
    np.testing.assert_array_equal(got["cnt"], want["cnt"], err_msg=f"{tag}: cnt")
    np.testing.assert_array_equal(got["idx"], want["idx"], err_msg=f"{tag}: idx")
    np.testing.assert_array_equal(got["shift"], want["shift"], err_msg=f"{tag}: shift")
    np.testing.assert_array_equal(bits(got["dist"]), bits(want["dist"]), err_msg=f"{tag}: dist bits")
    if profile and "profile" in got:
        g, w = np.asarray(got["profile"], F), np.asarray(want["profile"], F)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{tag}: profile NaNs")
        np.testing.assert_array_equal(bits(np.nan_to_num(g)), bits(np.nan_to_num(w)), err_msg=f"{tag}: profile bits")


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def random_descs(seed, n, rings, sectors, empty=0.2):
    """Descriptors in the method's range: heights up to 10 m, a fifth of the bins empty, and some whole columns empty."""
    rs = np.random.RandomState(seed)
    D = (rs.rand(n, rings, sectors) * 10.0).astype(F)
    D[rs.rand(n, rings, sectors) < empty] = 0
    D[np.broadcast_to(rs.rand(n, 1, sectors) < 0.1, D.shape)] = 0
    return D


def random_cloud(seed, n, reach=30.0):
    """n points around the sensor, heights within 3 m of it: most have a bin at the standard cfg."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-reach, reach, n), rs.uniform(-reach, reach, n), rs.uniform(-3.0, 3.0, n)], axis=1).astype(F)


def yaw_frame12(yaw, t=(0.0, 0.0, 0.0)):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2]], F)


def x26_of(pos, yaw):
    """A state row at ``pos`` turned by ``yaw`` about z: quaternion x y z w at [3:7], identity extrinsics."""
    x = np.zeros(26)
    x[0:3] = pos
    x[5], x[6] = math.sin(0.5 * yaw), math.cos(0.5 * yaw)
    x[10] = 1.0
    return x


def yaw_of(x26):
    qx, qy, qz, qw = np.asarray(x26, np.float64)[3:7]
    return math.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))


SCENE_CFG = cfg(rings=20, sectors=60, min_range=0.5, max_range=25.0, z_offset=2.0)
SENSOR_Z = 1.5      # the sensor above the ground: the ground's h is z_offset - SENSOR_Z = 0.5


@functools.lru_cache(maxsize=None)
def scene(seed=3, boxes=150, keyframes=20, spacing=10.0, off=1.0, step=0.6):
    """A ground plane and ``boxes`` random boxes along a strip, sampled every ``step`` metres on every face; ``keyframes`` poses
    ``spacing`` apart along the strip and one query per keyframe up to ``off`` metres away, every yaw random.  A sweep is the
    world's points within the cfg's range of the sensor, in the sensor's frame (no occlusion).  Returns a dict: world [N, 3],
    kf_x26 / q_x26 [K, 26], kf_sweep / q_sweep (lists of float32 [n, 3], body frame), truth [K] (the query's keyframe)."""
    rs = np.random.RandomState(seed)
    length, half = spacing * (keyframes - 1), 14.0
    reach = SCENE_CFG["max_range"]
    gx, gy = np.meshgrid(np.arange(-reach, length + reach, 2 * step), np.arange(-half - reach, half + reach, 2 * step))
    parts = [np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)]
    for _ in range(boxes):
        cx, cy = rs.uniform(-10.0, length + 10.0), rs.uniform(3.0, half + 8.0) * rs.choice([-1.0, 1.0])
        wx, wy, hz = rs.uniform(1.0, 5.0), rs.uniform(1.0, 5.0), rs.uniform(1.0, 7.0)
        xs, ys, zs = (np.arange(0.0, w + 1e-9, step) for w in (wx, wy, hz))
        for u, fixed, axis in ((xs, cy - wy / 2, 0), (xs, cy + wy / 2, 0), (ys, cx - wx / 2, 1), (ys, cx + wx / 2, 1)):
            a, b = np.meshgrid(u, zs)
            along = a.ravel() + (cx - wx / 2 if axis == 0 else cy - wy / 2)
            wall = np.stack([along, np.full(a.size, fixed), b.ravel()] if axis == 0 else [np.full(a.size, fixed), along, b.ravel()], axis=1)
            parts.append(wall)
        a, b = np.meshgrid(xs, ys)
        parts.append(np.stack([a.ravel() + cx - wx / 2, b.ravel() + cy - wy / 2, np.full(a.size, hz)], axis=1))
    world = np.concatenate(parts).astype(np.float64)

    def sweep(x26):
        yaw, p = yaw_of(x26), x26[0:3]
        d = world - p
        near = d[:, 0] ** 2 + d[:, 1] ** 2 < reach * reach
        d = d[near]
        c, s = math.cos(yaw), math.sin(yaw)
        return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], d[:, 2]], axis=1).astype(F)

    kf = np.stack([x26_of((spacing * i, 0.0, SENSOR_Z), rs.uniform(-math.pi, math.pi)) for i in range(keyframes)])
    qs = []
    for i in range(keyframes):
        r, th = off * math.sqrt(rs.rand()), rs.uniform(-math.pi, math.pi)
        qs.append(x26_of((spacing * i + r * math.cos(th), r * math.sin(th), SENSOR_Z), rs.uniform(-math.pi, math.pi)))
    qs = np.stack(qs)
    return dict(world=world.astype(F), kf_x26=kf, q_x26=qs, kf_sweep=[sweep(x) for x in kf], q_sweep=[sweep(x) for x in qs],
                truth=np.arange(keyframes))


@functools.lru_cache(maxsize=None)
def scene_descs(seed=3):
    """The scene's descriptors by the restatement: (keyframes' [K, 20, 60], queries' [K, 20, 60])."""
    sc = scene(seed)
    return (np.stack([descriptor(p, SCENE_CFG)[0] for p in sc["kf_sweep"]]), np.stack([descriptor(p, SCENE_CFG)[0] for p in sc["q_sweep"]]))


def wrap(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi
