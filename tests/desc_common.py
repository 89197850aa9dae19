"""Nearest descriptors (flimo_desc_match, include/flimo_c.h) restated in numpy, shared by tests/test_desc_host.py and
tests/test_gpu_desc.py: a vectorised correctly rounded float32 fmaf, the definition on top of it -- the chains of the dot product and
the norms, d = (n(q) + n(r)) - 2 dot clamped at +0, the exclusions, the order (bits of d, index) --, the pairing rule of
api.desc_pairs, and the scenes."""
import concurrent.futures
import functools

import numpy as np

F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)      # the key of a pair that is not returned
BLOCK = 1 << 18                           # (query, reference) pairs per block of the restatement


# ---- fmaf ---------------------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, elementwise (broadcasting).  The product of two float32 is exact in float64;
    the sum with c is formed by TwoSum; where its residual is not zero and the float64 sum's last mantissa bit is even, the sum is
    stepped one ulp towards the residual -- rounding to odd: the sticky bit the final cast needs --, and then cast: 53 >= 2 * 24 + 2
    bits make the double rounding innocuous.  Non-finite operands go the plain way (they round nowhere)."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = np.ascontiguousarray(s).view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)      # (a NaN residual compares unequal: the isfinite guards it)
        away = (err > 0) == (s > 0)                                # the residual points away from zero: the magnitude grows
        s = (bits + np.where(fix, np.where(away, 1, -1), 0)).view(np.float64)
        return s.astype(F)


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def rows(x):
    x = np.ascontiguousarray(x, F)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def dot_pairs(A, B):
    """The chain c_0 = +0, c_{t+1} = fmaf(a[t], b[t], c_t) of row i of A with row i of B: [n] float32."""
    A, B = rows(A), rows(B)
    c = np.zeros(A.shape[0], F)
    for t in range(A.shape[1]):
        c = fmaf(A[:, t], B[:, t], c)
    return c


def norms(X):
    """n(a) = dot(a, a); NaN for a row with a non-finite entry (an excluded row)."""
    X = rows(X)
    n = dot_pairs(X, X)
    n[~np.isfinite(X).all(axis=1)] = np.nan
    return n


def finish(nq, nr, dot):
    """d = (n(q) + n(r)) - 2 dot, one float32 addition and one rounding of the difference; a negative result +0; NaN stays."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = (np.asarray(nq, F) + np.asarray(nr, F)).astype(F)
        d = (t - (np.asarray(dot, F) + np.asarray(dot, F)).astype(F)).astype(F)
        return np.where(d < 0, F(0), d).astype(F)


def dist_pairs(A, B):
    """d of row i of A and row i of B (what flimo_desc_dist_host returns)."""
    return finish(norms(A), norms(B), dot_pairs(A, B))


def chain_matrix(Q, R):
    """The dot-product chain of every (query, reference) pair, [nq, nr] float32: fmaf's result by a cheaper route.  The float64
    sum s = a * b + c (the product exact, the sum rounded once) casts to the correctly rounded float32 UNLESS that first rounding
    landed s exactly half-way between two float32 -- the only way a double rounding errs -- so only the elements whose low 29
    mantissa bits are that half-way pattern (and the ones below float32's normal range, where the half-way bit sits elsewhere) go
    through fmaf itself.  tests/test_desc_host.py compares it with the plain fmaf chain."""
    Q, R = rows(Q), rows(R)
    q64, r64 = Q.astype(np.float64), R.astype(np.float64)
    mags = np.abs(np.concatenate([q64.ravel(), r64.ravel()]))
    tame = bool(np.all(q64 >= 0) and np.all(r64 >= 0) and np.all((mags == 0) | (mags >= 2.0 ** -40)))      # no cancellation, no tiny products
    out = np.empty((Q.shape[0], R.shape[0]), F)
    step = max(BLOCK // max(R.shape[0], 1), 1)

    def block(a0):
        qa = q64[a0:a0 + step]
        c32 = np.zeros((qa.shape[0], R.shape[0]), F)
        c = np.zeros((qa.shape[0], R.shape[0]), np.float64)
        s = np.empty_like(c)
        with np.errstate(over="ignore", invalid="ignore"):
            for t in range(Q.shape[1]):
                np.multiply(qa[:, t:t + 1], r64[None, :, t], out=s)
                s += c
                cand = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
                if not tame:
                    cand |= (np.abs(s) < 2.0 ** -120) & (s != 0)
                c32 = s.astype(F)
                if cand.any():
                    i, j = np.nonzero(cand)
                    c32[i, j] = fmaf(Q[a0 + i, t], R[j, t], c[i, j].astype(F))
                c = c32.astype(np.float64)
        out[a0:a0 + step] = c32

    starts = range(0, Q.shape[0], step)
    if len(starts) > 1:      # (numpy releases the interpreter lock inside its loops: the blocks run side by side)
        with concurrent.futures.ThreadPoolExecutor(min(8, len(starts))) as pool:
            list(pool.map(block, starts))
    else:
        for a0 in starts:
            block(a0)
    return out


def dist_matrix(Q, R):
    """d of every (query, reference) pair: [nq, nr] float32, NaN where the pair is excluded."""
    Q, R = rows(Q), rows(R)
    return finish(norms(Q)[:, None], norms(R)[None, :], chain_matrix(Q, R))


def keys(D):
    """(bits of d << 32 | reference index) per pair, NONE for a NaN."""
    k = (np.ascontiguousarray(D, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(D.shape[1], dtype=np.uint64)[None, :]
    return np.where(np.isnan(D), NONE, k)


def match(Q, R, k, D=None):
    """flimo_desc_match restated: dict idx [nq, k] int32, dist [nq, k] float32, cnt [nq] int32."""
    Q, R = rows(Q), rows(R)
    D = dist_matrix(Q, R) if D is None else D
    key = np.sort(keys(D), axis=1)[:, :k]
    if key.shape[1] < k:
        key = np.concatenate([key, np.full((key.shape[0], k - key.shape[1]), NONE)], axis=1)
    have = key != NONE
    idx = np.where(have, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    dist = np.where(have, (key >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(F)
    return dict(idx=idx, dist=dist, cnt=have.sum(axis=1).astype(np.int32))


class Restated:
    """An object that answers ``desc_match`` from the restatement: what api.desc_pairs runs on when no GPU is there."""

    def __init__(self, ref=None):
        self.ref = None if ref is None else rows(ref)

    def desc_ref_set(self, desc):
        self.ref = rows(desc)

    def desc_match(self, q, k=2):
        return match(q, self.ref, k)


def pairs(q_desc, r_desc, ratio=0.9, mutual=True, D=None):
    """api.desc_pairs written out pair by pair from the restated matches (D: dist_matrix(q, r) where the caller has it; the
    reverse direction reads its transpose: fmaf(a, b, c) = fmaf(b, a, c) and the sum of the norms commutes)."""
    q, r = rows(q_desc), rows(r_desc)
    D = dist_matrix(q, r) if D is None else D
    fwd, back = match(q, r, 2, D=D), match(r, q, 1, D=D.T)
    out = []
    for i in range(q.shape[0]):
        if fwd["cnt"][i] < 1 or not q[i].any():
            continue
        j = int(fwd["idx"][i, 0])
        if not r[j].any():
            continue
        if fwd["cnt"][i] >= 2 and not float(fwd["dist"][i, 0]) <= (ratio * ratio) * float(fwd["dist"][i, 1]):
            continue
        if mutual and not (back["cnt"][j] >= 1 and back["idx"][j, 0] == i):
            continue
        out.append((i, j))
    out = np.int64(out).reshape(-1, 2)
    return out[:, 0], out[:, 1]


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def random_rows(seed, n, dim, scale=100.0):
    """Rows in the descriptors' range: non-negative, up to ``scale`` (an FPFH bin is a percentage)."""
    return (np.random.RandomState(seed).rand(n, dim) * scale).astype(F)


def integer_rows(seed, n, dim, hi=4):
    """Small-integer rows: every product, sum and difference is exact, d is the integer squared distance and ties abound."""
    return np.random.RandomState(seed).randint(0, hi, (n, dim)).astype(F)


@functools.lru_cache(maxsize=None)
def tie_scene(dim=33):
    """(queries [96, dim], references [1300, dim]) of zeros and ones -- d is the Hamming distance: at dim 33 some 170 to 210
    references share a query's commonest distance --; reference rows 5, 37, 700 and 1299 are one row (different tiles of 32,
    different splits of 128), rows 64 .. 95 are all one other row."""
    Q, R = integer_rows(21, 96, dim, 2), integer_rows(22, 1300, dim, 2)
    R[[37, 700, 1299]] = R[5]
    R[64:96] = R[64]
    Q[0] = R[5]
    Q[1] = R[64]
    Q.setflags(write=False)
    R.setflags(write=False)
    return Q, R


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
