"""Shared helpers of the consistency-graph tests (flimo_corr_graph): the definition of include/flimo_c.h restated in numpy.

The predicate is float64 array arithmetic on the float32 inputs widened, written term by term in the header's association (numpy's
elementwise + - * sqrt are IEEE operations and never contracted); the core numbers come from plain peeling, which shares nothing
with the iteration the device runs.  Every output is an integer or a bit: the comparisons are exact."""
import numpy as np

import corr_common as cc

MAX_M = 32768
CFG = dict(tol=0.05, min_edge=0.5, edge_sim=0.0)      # of the random scenes


def graph(src, dst, tol=0.05, min_edge=0.0, edge_sim=0.0):
    """The dense adjacency [m, m] bool: for i != j, e_s = sq(s_j - s_i), e_d = sq(d_j - d_i); an edge iff e_s >= min2 and e_d >= min2,
    fabs(sqrt(e_s) - sqrt(e_d)) <= tol and fmin(e_s, e_d) >= s2 * fmax(e_s, e_d).  The cfg values are float32, widened."""
    s = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64)
    d = np.asarray(dst, np.float32).reshape(-1, 3).astype(np.float64)
    m = s.shape[0]
    t = float(np.float32(tol))
    min2 = float(np.float32(min_edge)) * float(np.float32(min_edge))
    s2 = float(np.float32(edge_sim)) * float(np.float32(edge_sim))
    A = np.zeros((m, m), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, m, 512):      # (rows in blocks: the differences of 4 096 pairs squared would be 400 MB at once)
            es = cc.sq(s[None, :, :] - s[a:a + 512, None, :])
            ed = cc.sq(d[None, :, :] - d[a:a + 512, None, :])
            A[a:a + 512] = ((es >= min2) & (ed >= min2) & (np.abs(np.sqrt(es) - np.sqrt(ed)) <= t) &
                            (np.fmin(es, ed) >= s2 * np.fmax(es, ed)))
    A[np.arange(m), np.arange(m)] = False
    return A


def pack(A):
    """The bit rows [m, (m + 63) // 64] uint64: bit j & 63 of word j >> 6 of row i; the padding bits are 0."""
    A = np.asarray(A, bool)
    m = A.shape[0]
    W = (m + 63) // 64
    padded = np.zeros((m, W * 64), bool)
    padded[:, :m] = A
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(m, W)


def unpack(words, m):
    """pack's inverse, the padding bits included: [m, W * 64] bool."""
    w = np.ascontiguousarray(np.asarray(words, np.uint64).astype("<u8"))
    return np.unpackbits(w.view(np.uint8).reshape(m, -1), axis=1, bitorder="little").astype(bool)


def cores(A):
    """The core numbers [m] int32 by plain peeling: at level k remove every live vertex of degree <= k (among the live ones) until
    none is left, then k + 1.  A vertex's core number is the level at which it goes."""
    A = np.asarray(A, bool)
    m = A.shape[0]
    deg = A.sum(1).astype(np.int64)
    live = np.ones(m, bool)
    core = np.zeros(m, np.int32)
    k = 0
    while live.any():
        while True:
            go = live & (deg <= k)
            if not go.any():
                break
            core[go] = k
            live[go] = False
            deg -= A[:, go].sum(1)
        k += 1
    return core


def cores_by_definition(A):
    """The core numbers of a graph of at most 12 vertices from the definition: over ALL vertex subsets, core[v] = the largest
    minimum inside degree of a subset that contains v."""
    A = np.asarray(A, bool)
    n = A.shape[0]
    assert n <= 12
    S = ((np.arange(1, 1 << n)[:, None] >> np.arange(n)) & 1).astype(bool)      # every non-empty subset
    inside = S.astype(np.int64) @ A.astype(np.int64)                            # neighbours of v inside the subset
    low = np.where(S, inside, n).min(1)                                         # its minimum inside degree
    return np.array([low[S[:, v]].max() for v in range(n)], np.int32)


def reference(src, dst, **cfg):
    A = graph(src, dst, **cfg)
    return dict(A=A, adj=pack(A), degree=A.sum(1).astype(np.int32), core=cores(A))


def check(got, A, tag="", core=None):
    """What ``HipCtx.corr_graph`` returned against the dense adjacency A: adj (where asked for) bit for bit with zero padding and
    symmetric, degree the row popcounts, core and max_core the peeling's (``core``: computed before, for A)."""
    A = np.asarray(A, bool)
    m = A.shape[0]
    assert got["degree"].dtype == np.int32 and got["core"].dtype == np.int32 and got["degree"].shape == got["core"].shape == (m,)
    if "adj" in got:
        assert got["adj"].dtype == np.uint64 and got["adj"].shape == (m, (m + 63) // 64)
        bits = unpack(got["adj"], m)
        assert not bits[:, m:].any(), f"{tag}: padding bits"
        np.testing.assert_array_equal(bits[:, :m], bits[:, :m].T, err_msg=f"{tag}: adj is symmetric")
        np.testing.assert_array_equal(got["adj"], pack(A), err_msg=f"{tag}: adj")
    np.testing.assert_array_equal(got["degree"], A.sum(1), err_msg=f"{tag}: degree")
    want = cores(A) if core is None else core
    np.testing.assert_array_equal(got["core"], want, err_msg=f"{tag}: core")
    assert got["max_core"] == (int(want.max()) if m else 0), f"{tag}: max_core"


def same_bytes(a, b, tag="", names=None):
    for name in (names or sorted(a)):
        if name == "max_core":
            assert a[name] == b[name], f"{tag}: max_core differs"
        else:
            assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), f"{tag}: {name} differs"


def rotation(seed):
    """A rotation matrix, float64, from a seeded random quaternion."""
    q = np.random.RandomState(seed).randn(4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def moved(src, seed, t=(3.0, -2.0, 0.5), noise=0.0):
    """src under the rigid motion (rotation(seed), t), plus N(0, noise) per coordinate, float32."""
    rs = np.random.RandomState(1000 + seed)
    p = np.asarray(src, np.float64) @ rotation(seed).T + np.float64(t)
    return (p + rs.randn(*p.shape) * noise).astype(np.float32)


def planted(m, seed, share=0.3, box=10.0, noise=0.005):
    """Random clouds with a planted rigid subset: src and dst uniform in a cube of ``box`` metres; about ``share`` of the pairs (at
    least min(m, 3)) have dst = their src under one rigid motion plus noise.  Returns (src, dst, true [m] bool)."""
    rs = np.random.RandomState(seed)
    src = ((rs.rand(m, 3) - 0.5) * box).astype(np.float32)
    dst = ((rs.rand(m, 3) - 0.5) * box).astype(np.float32)
    true = rs.rand(m) < share
    true[rs.permutation(m)[:min(m, 3)]] = True
    dst[true] = moved(src[true], seed, noise=noise)
    return src, np.ascontiguousarray(dst), true


def chain(m=257):
    """The graph that is one path: src[i] = (i, 0, 0), dst[i] = ((i + 1) // 2, i // 2, 0) -- a staircase.  Neighbours in the order
    are 1 m apart in both clouds; two points k >= 2 steps apart are k m apart in src and at most sqrt((k/2 + 1/2)^2 + (k/2)^2) m in
    dst, shorter by 0.4 m and more.  With tol 0.01 and min_edge 0.5 the degrees are 1, 2, .., 2, 1 and every core number is 1.
    Returns (src, dst, cfg)."""
    i = np.arange(m)
    src = np.stack([i, 0 * i, 0 * i], 1).astype(np.float32)
    dst = np.stack([(i + 1) // 2, i // 2, 0 * i], 1).astype(np.float32)
    return src, dst, dict(tol=0.01, min_edge=0.5, edge_sim=0.0)
