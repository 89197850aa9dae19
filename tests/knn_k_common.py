"""Shared helper of the k-NN-for-any-k tests: the numpy brute force in flimo_knn_k's unique order."""
import numpy as np

from radius_common import bits, sqdist_f32


def brute_knn(q, pts, k, max_dist=np.inf, chunk=64, extra=0):
    """(idx [nq, k + extra], sqd [nq, k + extra], cnt [nq]): per query the first k + extra stored points in the order (float32
    squared-distance bits, index) among those with squared distance < float32(max_dist)^2 (strict; inf: no gate), padded with
    idx -1 / sqd 0; cnt = min(k, admitted).  `extra` further columns let a test look at the (k+1)-th distance."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    nq, n, w = q.shape[0], pts.shape[0], k + extra
    idx = np.full((nq, w), -1, np.int32)
    sqd = np.zeros((nq, w), np.float32)
    cnt = np.zeros(nq, np.int32)
    gate = not np.isinf(max_dist)
    with np.errstate(over="ignore"):
        r2 = np.float32(np.float32(max_dist) * np.float32(max_dist))
    ar = np.arange(n, dtype=np.uint64)
    for a in range(0, nq, chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            d = sqdist_f32(q[a:a + chunk], pts)
        key = (bits(d).astype(np.uint64) << np.uint64(32)) | ar[None, :]
        bad = np.isnan(d) | (np.isnan(q[a:a + chunk]).any(1)[:, None])
        if gate:
            bad |= ~(d < r2)
        key[bad] = np.uint64(0xFFFFFFFFFFFFFFFF)
        m = min(w, n)
        if m == 0:
            continue
        part = np.argpartition(key, m - 1, axis=1)[:, :m] if m < n else np.tile(np.arange(n), (key.shape[0], 1))
        pk = np.take_along_axis(key, part, 1)
        o = np.argsort(pk, axis=1, kind="stable")
        part, pk = np.take_along_axis(part, o, 1), np.take_along_axis(pk, o, 1)
        ok = pk != np.uint64(0xFFFFFFFFFFFFFFFF)
        idx[a:a + chunk, :m] = np.where(ok, part, -1)
        sqd[a:a + chunk, :m] = np.where(ok, np.take_along_axis(d, part, 1), np.float32(0))
        cnt[a:a + chunk] = np.minimum(ok.sum(1), k)
    return idx, sqd, cnt
