"""Shared helper of the outlier tests: flimo_map_outliers' definition (include/flimo_c.h) restated in numpy, and the scene.

The neighbour lists are knn_k_common.brute_knn's (flimo_knn_k's predicate and unique order), the distances np.sqrt on float32 (correctly
rounded, as the device's), a point's sum the pairwise tree over the 64 slots of its list, mu and sigma math.fsum's (correctly rounded
sums).  The device adds the same non-negative float64 terms in another order: any order of summing N of them lies within N * 2^-52
relative of the exact sum (each of the N - 1 additions rounds by at most 2^-53 relative of a partial sum that is at most the total), so
the tests hold the two sums -- and mu, sigma, threshold -- to BOUND(N) = 4 * N * 2^-52 relative, and ask of every configuration they
run that no mean distance of T lies within GAP = 1e-9 relative of the yardstick's threshold: the masks are then equal bit for bit."""
import functools
import math

import numpy as np

from fast_limo_amd import synth
from knn_k_common import brute_knn
from radius_common import sqdist_f32
from sums_common import shape_sums

INF = float("inf")
F = np.float32
SLOTS = 64
GAP = 1.0e-9
N_SCENE = 8356

# (k, max_dist) of the configurations the issue probed, each run with std_mul 1 and 2 ...
PROBED = [(8, INF), (16, 1.0), (17, INF), (63, 2.0), (3, 0.3), (1, INF)]
# ... and what the GPU tests run: dict(k, max_dist, min_pts, std_mul)
CONFIGS = [dict(k=k, max_dist=g, min_pts=0, std_mul=s) for k, g in PROBED for s in (1.0, 2.0)] + [
    dict(k=15, max_dist=INF, min_pts=0, std_mul=1.0), dict(k=16, max_dist=1.0, min_pts=3, std_mul=1.0)]


def bound(n_stat):
    return 4.0 * max(int(n_stat), 1) * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def scene():
    """8 356 points: a box world, 300 specks in the air, 40 exact duplicates, four points stored five times each."""
    static = synth.box_world_map(8000, 12.0, 3)
    rs = np.random.RandomState(11)
    x, y, z = rs.uniform(-10, 10, 300), rs.uniform(-10, 10, 300), rs.uniform(-1, 15, 300)
    specks = np.stack([x, y, z], 1).astype(F)
    pts = np.concatenate([static, specks, static[:40], np.tile(static[100:104], (4, 1))]).astype(F)
    assert pts.shape == (N_SCENE, 3)
    pts.setflags(write=False)
    return pts


FAR_POINTS = F([[500.0, 3.0, 1.0], [-20.0, -650.0, 20.0], [-560.0, 560.0, 5.0]])


@functools.lru_cache(maxsize=None)
def far_scene():
    """... plus three points 500 to 800 m away: their searches leave the block search for the walk over the tiles."""
    pts = np.concatenate([scene(), FAR_POINTS]).astype(F)
    pts.setflags(write=False)
    return pts


def slot_tree(v):
    """The pairwise tree over the slots of each row: ((v0 + v1) + (v2 + v3)) + ..."""
    v = np.asarray(v, np.float64)
    assert v.ndim == 2 and v.shape[1] == SLOTS
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def mean_dists(pts, first, n, k, max_dist):
    """(m [n] float64, c [n] int32, selfless [n] bool): mean neighbour distance and neighbour count of the stored points first ..
    first + n - 1; selfless: the point's own slot was missing from its full list (the last slot was dropped instead)."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    if n == 0:
        return np.zeros(0), np.zeros(0, np.int32), np.zeros(0, bool)
    idx, sqd, _ = brute_knn(pts[first:first + n], pts, k + 1, max_dist, chunk=256)
    has = idx >= 0
    own = idx == (first + np.arange(n, dtype=np.int64))[:, None]
    selfless = ~own.any(1) & has[:, k]
    drop = own.copy()
    drop[selfless, k] = True
    keep = has & ~drop
    c = keep.sum(1).astype(np.int32)
    d = np.sqrt(sqd.astype(F)).astype(np.float64)
    v = np.zeros((n, SLOTS))
    v[:, :k + 1] = np.where(keep, d, 0.0)
    s = slot_tree(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(c > 0, s / np.maximum(c, 1), np.nan)
    return m, c, selfless


def statistics(m, c, min_pts, std_mul):
    """dict(n, n_stat, mu, sigma, threshold, few, far, outliers, mask, in_t, sum_m, sum_d2)."""
    need = max(1, int(min_pts))
    t = c >= need
    n_stat = int(t.sum())
    mu = sigma = thr = float("nan")
    sum_m = sum_d2 = 0.0
    if n_stat:
        sum_m = math.fsum(m[t])
        mu = sum_m / n_stat
        sigma = 0.0
        if n_stat > 1:
            sum_d2 = math.fsum((m[t] - mu) * (m[t] - mu))
            sigma = math.sqrt(sum_d2 / (n_stat - 1))
        with np.errstate(invalid="ignore"):
            thr = float(np.float64(mu) + np.float64(F(std_mul)) * np.float64(sigma))
    few = c < int(min_pts)
    far = np.zeros(len(c), bool)
    if math.isfinite(std_mul) and n_stat:
        far = t & (m > thr)
    assert not np.any(few & far)
    return dict(n=len(c), n_stat=n_stat, mu=mu, sigma=sigma, threshold=thr, few=int(few.sum()), far=int(far.sum()),
                outliers=int(few.sum() + far.sum()), mask=few | far, in_t=t, sum_m=sum_m, sum_d2=sum_d2)


def device_stats(m, c, min_pts, std_mul):
    """dict(n_stat, mu, sigma, threshold) as the call forms them, bit for bit, from the mean_dist and cnt it returned: the device's two
    sums in their one shape (sums_common.shape_sums, one number a slot; a slot outside T adds +0.0), the host's arithmetic around them
    (mu = S / N; sigma = sqrt(S / (N - 1)), 0.0 for N = 1; threshold = mu + float64(float32(std_mul)) * sigma, two roundings)."""
    m = np.asarray(m, np.float64)
    t = np.asarray(c) >= max(1, int(min_pts))
    n_stat = int(t.sum())
    mu = sigma = thr = np.float64("nan")
    if n_stat:
        mu = shape_sums(np.where(t, m, 0.0)[:, None, None])[0] / np.float64(n_stat)
        sigma = np.float64(0.0)
        if n_stat > 1:
            with np.errstate(invalid="ignore"):
                d2 = np.where(t, (m - mu) * (m - mu), 0.0)
            sigma = np.sqrt(shape_sums(d2[:, None, None])[0] / np.float64(n_stat - 1))
        with np.errstate(invalid="ignore"):
            thr = mu + np.float64(F(std_mul)) * sigma
    return dict(n_stat=n_stat, mu=float(mu), sigma=float(sigma), threshold=float(thr))


def same_bits(got, want, what=""):
    """n_stat equal; mu, sigma and threshold of the same bits (a NaN on both sides is the same: its sign is the host's choice)."""
    assert got["n_stat"] == want["n_stat"], (what, got["n_stat"], want["n_stat"])
    for key in ("mu", "sigma", "threshold"):
        g, w = np.float64(got[key]), np.float64(want[key])
        assert (np.isnan(g) and np.isnan(w)) or g.tobytes() == w.tobytes(), (what, key, repr(got[key]), repr(want[key]))


def rel_gap(m, st):
    """The smallest relative distance of a mean of T from the threshold (inf: the statistical rule is off or T is empty)."""
    thr = st["threshold"]
    if not (math.isfinite(thr) and st["n_stat"]):
        return INF
    return float(np.min(np.abs(m[st["in_t"]] - thr)) / abs(thr))


@functools.lru_cache(maxsize=None)
def cached_means(which, k, max_dist):
    """mean_dists over the whole scene (`which`: "scene" or "far"), computed once per (k, gate)."""
    pts = scene() if which == "scene" else far_scene()
    m, c, s = mean_dists(pts, 0, len(pts), k, max_dist)
    for a in (m, c, s):
        a.setflags(write=False)
    return m, c, s


def yardstick(which, first=0, n=None, k=8, max_dist=INF, min_pts=0, std_mul=1.0):
    """(m, c, statistics) of the range [first, first + n) of a scene."""
    m, c, _ = cached_means(which, k, max_dist)
    n = len(m) - first if n is None else n
    m, c = m[first:first + n], c[first:first + n]
    return m, c, statistics(m, c, min_pts, std_mul)


def radius_counts(pts, radius, chunk=256):
    """Stored points with float32 squared distance < float32(radius)^2 of each stored point, the point itself included."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    r2 = F(F(radius) * F(radius))
    out = np.zeros(len(pts), np.int64)
    for a in range(0, len(pts), chunk):
        out[a:a + chunk] = (sqdist_f32(pts[a:a + chunk], pts) < r2).sum(1)
    return out


def same_stats(got, want, what=""):
    """The counts exact; mu, sigma, threshold within BOUND(N) relative (NaN where the yardstick has NaN, inf where it has inf)."""
    for key in ("n", "n_stat", "few", "far", "outliers"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    b = bound(want["n_stat"])
    for key in ("mu", "sigma", "threshold"):
        g, w = got[key], want[key]
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) and math.isnan(w)) or g == w, (what, key, g, w)
        else:
            assert abs(g - w) <= b * abs(w), (what, key, g, w, b)
