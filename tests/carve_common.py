"""Shared helpers of the carve tests (flimo_map_seen_through / flimo_map_carve): the yardstick and the standard scene.

The yardstick is the definition in include/flimo_c.h restated in numpy: ``pixels``, ``range_image`` and ``seen_through``.  Every
operation is one float32 operation of IEEE arithmetic ('-', '/', '*', '+', compares, a truncating cast), in the order the header
gives, so the device's result is this one bit for bit -- no tolerance anywhere."""
import numpy as np

from fast_limo_amd import synth
from scan_fitness_common import world_points, x26_of

F = np.float32
INF = float("inf")
STD_CFG = dict(res=64, win=1, margin=0.2, rel_margin=0.02, max_depth=INF)
N_GHOST = 400


def pixels(x, s, res):
    """Per point of x [n, 3]: (has a pixel, face, row it, column iu, depth m); s: the sensor origin; float32 throughout."""
    x, s = np.asarray(x, F).reshape(-1, 3), np.asarray(s, F).reshape(3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = x - s
        av = np.abs(v)
        ok = np.isfinite(v).all(1)
        axis = np.where((av[:, 0] >= av[:, 1]) & (av[:, 0] >= av[:, 2]), 0, np.where(av[:, 1] >= av[:, 2], 1, 2))
        r = np.arange(len(x))
        va = v[r, axis]
        m = np.abs(va)
        ok &= m != 0
        face = 2 * axis + (va < 0)
        a, b = v[r, (axis + 1) % 3], v[r, (axis + 2) % 3]            # cyclic: x -> (y, z), y -> (z, x), z -> (x, y)
        mm = np.where(ok, m, F(1))
        u, t = np.where(ok, a, F(0)) / mm, np.where(ok, b, F(0)) / mm
        hr = F(0.5 * res)
        iu = np.minimum(res - 1, ((u + F(1.0)) * hr).astype(np.int32))
        it = np.minimum(res - 1, ((t + F(1.0)) * hr).astype(np.int32))
    return ok, face.astype(np.int32), it, iu, m.astype(F)


def range_image(world, s, res):
    """D [6, res, res] float32: the minimum depth of the scan's world points per pixel, +inf where there is none."""
    ok, f, it, iu, m = pixels(world, s, res)
    D = np.full((6, res, res), np.inf, F)
    np.minimum.at(D, (f[ok], it[ok], iu[ok]), m[ok])
    return D


def seen_through(q, D, s, win, margin, rel_margin, max_depth=INF):
    """Mask [n] of the stored points q that the range image D looks through."""
    res = D.shape[1]
    ok, f, it, iu, m = pixels(q, s, res)
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= m <= F(max_depth)
        ok &= (it - win >= 0) & (it + win <= res - 1) & (iu - win >= 0) & (iu + win <= res - 1)
        f, it, iu = np.where(ok, f, 0), np.where(ok, it, win), np.where(ok, iu, win)
        ok &= np.isfinite(D[f, it, iu])
        thr = m + (F(margin) + F(rel_margin) * m)
        for dt in range(-win, win + 1):
            for du in range(-win, win + 1):
                d = D[f, it + dt, iu + du]
                ok &= ~np.isfinite(d) | (thr < d)
    return ok


def yardstick(world, q, s, res, win, margin, rel_margin, max_depth=INF):
    return seen_through(q, range_image(world, s, res), s, win, margin, rel_margin, max_depth)


# ---- the standard scene: a box world, a ghost cluster inside it that the sweep looks through, one sweep from T* ----------------------
def standard_scene():
    """(static map points [8000, 3], ghost points [400, 3], scan [n, 3] body frame, x26 of T*, sensor origin float32[3])."""
    static = synth.box_world_map(8000, 12.0, 3)
    rs = np.random.RandomState(5)
    ghost = np.stack([rs.uniform(4, 6, N_GHOST), rs.uniform(1, 3, N_GHOST), rs.uniform(-1.8, -0.3, N_GHOST)], 1).astype(F)
    scan = np.ascontiguousarray(synth.velodyne_scan(32, 900, 12.0, 9)[:, :3])
    return static, ghost, scan, x26_of(), F(synth.T_STAR_T)


def standard_world(scan, x26):
    """The scan's world points without a GPU: transform_kernel's arithmetic in numpy (scan_fitness_common.world_points)."""
    return world_points(x26, scan)

