"""Nearest descriptors (flimo_desc_match) as far as they can be checked without a GPU: the entry points are exported, declared and
listed; NULL arguments and a bad dim are rejected; the numpy fmaf of tests/desc_common.py equals libm's fmaf bit for bit, so the
restatement built on it is the definition; flimo_desc_dist_host -- the host / device functions the device code uses for the norms and
the final step, run on the host -- equals the restatement with no tolerance; the error bound include/flimo_c.h states holds; the
restatement's order is a plain sort of (bits, index); and api.desc_pairs on an object that answers from the restatement.  The match
itself runs on the GPU: tests/test_gpu_desc.py."""
import ctypes as C
import ctypes.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

import desc_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ERR_INVALID, ERR_UNSUPPORTED = -2, -6
DIMS = (1, 2, 3, 33, 34, 64)


def host_dist(A, B):
    """flimo_desc_dist_host per pair of rows: [n] float32."""
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    A, B = dc.rows(A), dc.rows(B)
    out = np.full(A.shape[0], 7, F)
    for i in range(A.shape[0]):
        assert L.flimo_desc_dist_host(A[i].ctypes.data, B[i].ctypes.data, A.shape[1], out[i:].ctypes.data) == 0
    return out


def equal_bits(got, want, tag=""):
    """The bits of two float32 arrays, every NaN pattern counting as NaN."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{tag}: NaN")
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(dc.bits(got[ok]), dc.bits(want[ok]), err_msg=f"{tag}: bits")


def test_desc_entry_points_are_exported_declared_and_listed(built):
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    dev = open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in ("flimo_desc_ref_set", "flimo_desc_ref_size", "flimo_desc_ref_dim", "flimo_desc_match", "flimo_desc_dist_host"):
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS and name + "(" in pub, name
    for word in ("FLIMO_DESC_MAX_DIM 64", "FLIMO_DESC_MAX_K 8", "fmaf(a[t], b[t], c_t)", "(2 dim + 4) * 2^-24", "tests/desc_common.py"):
        assert word in pub, word
    for name in ("flimo_set_desc_chunk", "flimo_desc_last_ms"):
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS and name + "(" in dev, name
    for name in ("flimo_loc_desc_ref_set", "flimo_loc_desc_match"):
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for cls, names in ((_lib.HipCtx, ("desc_ref_set", "desc_ref_size", "desc_match", "set_desc_chunk")),
                       (api.Localizer, ("desc_ref_set", "desc_ref_size", "desc_match"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert callable(api.desc_pairs) and callable(api.relocalize)
    assert (_lib.DESC_MAX_DIM, _lib.DESC_MAX_K) == (64, 8)
    # the equality of the headers and the symbol lists (tests/test_host_logic.py) holds with the new names in
    import test_host_logic
    test_host_logic.test_c_abi_exports_every_declared_symbol(True)


def test_the_calls_reject_null_arguments_and_a_bad_dim_and_leave_their_outputs(built):
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    q = np.ones((2, 33), F)
    idx, dist, cnt = np.full((2, 2), 7, np.int32), np.full((2, 2), 7, F), np.full(2, 7, np.int32)
    out = (idx.ctypes.data, dist.ctypes.data, cnt.ctypes.data)
    assert L.flimo_desc_match(None, q.ctypes.data, 2, 33, 2, *out) == ERR_INVALID
    assert L.flimo_desc_ref_set(None, q.ctypes.data, 2, 33) == ERR_INVALID
    assert L.flimo_set_desc_chunk(None, 32, 32) == ERR_INVALID
    assert L.flimo_desc_ref_size(None) == 0 and L.flimo_desc_ref_dim(None) == 0 and L.flimo_desc_last_ms(None) == 0.0
    assert H.flimo_loc_desc_match(None, q.ctypes.data, 2, 33, 2, *out) == ERR_INVALID
    assert H.flimo_loc_desc_ref_set(None, q.ctypes.data, 2, 33) == ERR_INVALID
    assert np.all(idx == 7) and np.all(dist == 7) and np.all(cnt == 7)
    d = np.full(1, 7, F)
    fn = L.flimo_desc_dist_host
    assert fn(None, q.ctypes.data, 33, d.ctypes.data) == ERR_INVALID
    assert fn(q.ctypes.data, None, 33, d.ctypes.data) == ERR_INVALID
    assert fn(q.ctypes.data, q.ctypes.data, 33, None) == ERR_INVALID
    for dim in (0, -1, 65):
        assert fn(q.ctypes.data, q.ctypes.data, dim, d.ctypes.data) == ERR_UNSUPPORTED, dim
    assert d[0] == 7
    assert fn(q.ctypes.data, q.ctypes.data, 64, d.ctypes.data) == 0 and d[0] == 0


def _libm_fmaf():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = C.c_float
    m.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    return lambda a, b, c: np.array([m.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F)


def near_tie_triples(seed, n):
    """a * b + c a hair beside a rounding boundary of the float32 result, closer than float64 resolves: a an odd integer of 12 bits,
    b = round(2^35 / a) (24 bits), so a * b = 2^35 + e with |e| < 2^11; c = M * 2^36 with M of 24 bits and either sign, so the
    result's last place is 2^36 and the product sits e beside HALF of it.  The float64 sum has its last place at 2^7 or 2^8: wherever
    0 < |e| < 64 it rounds onto the tie itself, and a cast then rounds to even -- wrongly for half of those."""
    rs = np.random.RandomState(seed)
    a = (rs.randint(1 << 11, 1 << 12, n) | 1).astype(np.int64)
    b = np.rint(2.0 ** 35 / a).astype(np.int64)
    c = rs.randint(1 << 23, 1 << 24, n).astype(np.float64) * 2.0 ** 36
    sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    assert np.all(b < (1 << 24))
    return a.astype(F), b.astype(F), (sign * c).astype(F)


def test_the_numpy_fmaf_is_libms_fmaf_bit_for_bit():
    ref = _libm_fmaf()
    rs = np.random.RandomState(1)
    n = 100000
    a, b = (rs.rand(n) * 100).astype(F), (rs.rand(n) * 100).astype(F)
    c = (rs.rand(n) * 30000).astype(F)
    np.testing.assert_array_equal(dc.bits(dc.fmaf(a, b, c)), dc.bits(ref(a, b, c)))
    # both signs, many magnitudes
    a = (rs.standard_normal(n) * 10.0 ** rs.randint(-20, 20, n)).astype(F)
    b = (rs.standard_normal(n) * 10.0 ** rs.randint(-20, 20, n)).astype(F)
    c = (rs.standard_normal(n) * 10.0 ** rs.randint(-38, 38, n)).astype(F)
    got, want = dc.fmaf(a, b, c), ref(a, b, c)
    np.testing.assert_array_equal(dc.bits(got), dc.bits(want))
    # near ties: the double rounding a plain float64 a * b + c commits shows here
    a, b, c = near_tie_triples(2, 20000)
    got, want = dc.fmaf(a, b, c), ref(a, b, c)
    np.testing.assert_array_equal(dc.bits(got), dc.bits(want))
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    e = a.astype(np.int64) * b.astype(np.int64) - (1 << 35)
    print("near-tie triples where float64 a * b + c then a cast differs from fmaf:", int((dc.bits(plain) != dc.bits(want)).sum()), "of", a.size,
          "; within 64 of the tie:", int(((e != 0) & (np.abs(e) < 64)).sum()))
    assert (dc.bits(plain) != dc.bits(want)).any(), "the constructed triples must reach the double-rounding cases"
    # the specials
    s = F([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0e-45])
    a, b, c = (v.ravel() for v in np.meshgrid(s, s, s, indexing="ij"))
    got, want = dc.fmaf(a, b, c), ref(a, b, c)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(dc.bits(got[~np.isnan(want)]), dc.bits(want[~np.isnan(want)]))


def test_the_restatements_quick_chain_is_the_plain_fmaf_chain():
    """dc.chain_matrix sends only the half-way cases through fmaf: the same bits as fmaf at every step, on descriptor-like rows, on
    signed rows over forty decades (cancellation, results below float32's normal range, overflow) and on rows built to hit the
    half-way pattern (near_tie_triples laid out as rows of dim 2: the pairs on the diagonal are its triples)."""
    def plain(Q, R):
        c = np.zeros((Q.shape[0], R.shape[0]), F)
        for t in range(Q.shape[1]):
            c = dc.fmaf(Q[:, t:t + 1], R[None, :, t], c)
        return c
    rs = np.random.RandomState(3)
    cases = [(dc.random_rows(1, 70, 33), dc.random_rows(2, 300, 33))]
    cases.append(((rs.standard_normal((60, 33)) * 10.0 ** rs.randint(-25, 20, (60, 33))).astype(F),
                  (rs.standard_normal((200, 33)) * 10.0 ** rs.randint(-25, 20, (200, 33))).astype(F)))
    a, b, c = near_tie_triples(5, 1500)
    cases.append((np.stack([c * F(2.0 ** -36), a], axis=1), np.stack([np.full(1500, 2.0 ** 36, F), b], axis=1)))
    for Q, R in cases:
        got, want = dc.chain_matrix(Q, R), plain(Q, R)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(dc.bits(got[~np.isnan(want)]), dc.bits(want[~np.isnan(want)]))
    # (and the plain float64 route alone is NOT enough on the last case: the half-way cases exist)
    Q, R = cases[2]
    c = np.zeros((1500, 1500))
    for t in range(2):
        c = (Q[:, t:t + 1].astype(np.float64) * R[None, :, t].astype(np.float64) + c).astype(F).astype(np.float64)
    differ = int((dc.bits(c.astype(F)) != dc.bits(want)).sum())
    print("elements where casting the float64 sum differs from the fmaf chain:", differ)
    assert differ > 0


@pytest.mark.parametrize("dim", DIMS)
def test_host_distance_equals_the_restatement_on_random_rows(built, dim):
    A, B = dc.random_rows(dim, 400, dim), dc.random_rows(100 + dim, 400, dim)
    want = dc.dist_pairs(A, B)
    equal_bits(host_dist(A, B), want, f"dim {dim}")
    # the bound of include/flimo_c.h against float64
    exact = ((A.astype(np.float64) - B.astype(np.float64)) ** 2).sum(axis=1)
    n2 = (A.astype(np.float64) ** 2).sum(axis=1) + (B.astype(np.float64) ** 2).sum(axis=1)
    bound = (2 * dim + 4) * 2.0 ** -24 * n2
    err = np.abs(want.astype(np.float64) - exact)
    print(f"dim {dim}: largest error {err.max():.3e}, largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # signed rows of mixed magnitudes
    rs = np.random.RandomState(7 + dim)
    A = (rs.standard_normal((300, dim)) * 10.0 ** rs.randint(-3, 4, (300, dim))).astype(F)
    B = (rs.standard_normal((300, dim)) * 10.0 ** rs.randint(-3, 4, (300, dim))).astype(F)
    want = dc.dist_pairs(A, B)
    equal_bits(host_dist(A, B), want, f"dim {dim}, signed")
    exact = ((A.astype(np.float64) - B.astype(np.float64)) ** 2).sum(axis=1)
    n2 = (A.astype(np.float64) ** 2).sum(axis=1) + (B.astype(np.float64) ** 2).sum(axis=1)
    assert np.all(np.abs(want.astype(np.float64) - exact) <= (2 * dim + 4) * 2.0 ** -24 * n2)


@pytest.mark.parametrize("dim", DIMS)
def test_host_distance_on_integer_identical_and_non_finite_rows(built, dim):
    A, B = dc.integer_rows(dim, 300, dim, 16), dc.integer_rows(50 + dim, 300, dim, 16)
    want = ((A.astype(np.int64) - B.astype(np.int64)) ** 2).sum(axis=1)
    got = host_dist(A, B)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(F))
    equal_bits(got, dc.dist_pairs(A, B), "integers")
    # identical rows: exactly +0.0, whatever the values
    R = dc.random_rows(3, 200, dim, 1.0e4)
    got = host_dist(R, R.copy())
    assert np.all(dc.bits(got) == 0)
    equal_bits(got, dc.dist_pairs(R, R), "identical")
    # a NaN or an infinity anywhere in either row: NaN (the pair is excluded)
    for bad in (np.nan, np.inf, -np.inf):
        for at in sorted({0, dim // 2, dim - 1}):
            X = R[:4].copy()
            X[:, at] = bad
            for a, b in ((X, R[4:8]), (R[4:8], X), (X, X)):
                got = host_dist(a, b)
                assert np.isnan(got).all() and np.isnan(dc.dist_pairs(a, b)).all()
    # huge finite entries: every chain overflows, inf - inf
    H = np.full((2, dim), 1.0e20, F)
    assert np.isnan(host_dist(H, H)).all() and np.isnan(dc.dist_pairs(H, H)).all()
    # one huge row against a small one: +inf is a distance like any other
    got = host_dist(H, R[:2])
    assert np.all(np.isposinf(got))
    equal_bits(got, dc.dist_pairs(H, R[:2]), "inf")


def test_the_restated_order_is_a_plain_sort_of_bits_and_index():
    Q, R = dc.tie_scene()
    R = R.copy()
    R[3, 0] = np.nan
    R[9, 5] = np.inf
    Q = Q.copy()
    Q[7, 2] = np.nan
    D = dc.dist_matrix(Q, R)
    assert np.isnan(D[:, 3]).all() and np.isnan(D[:, 9]).all() and np.isnan(D[7]).all() and np.isnan(D).sum() == 2 * 96 + 1300 - 2
    # integers: the matrix is the integer squared distance
    ok = ~np.isnan(D)
    want = ((np.nan_to_num(Q, posinf=0)[:, None, :].astype(np.int64) - np.nan_to_num(R, posinf=0)[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
    assert np.array_equal(D[ok].astype(np.int64), want[ok])
    B, nan = dc.bits(D).tolist(), np.isnan(D).tolist()
    for k in (1, 2, 8):
        got = dc.match(Q, R, k, D=D)
        for i in range(Q.shape[0]):
            plain = sorted((B[i][j], j) for j in range(R.shape[0]) if not nan[i][j])[:k]
            n = len(plain)
            assert got["cnt"][i] == n == (0 if i == 7 else k)
            assert [int(v) for v in got["idx"][i, :n]] == [j for _, j in plain]
            assert [int(v) for v in dc.bits(got["dist"][i, :n])] == [b for b, _ in plain]
            assert np.all(got["idx"][i, n:] == -1) and np.all(dc.bits(got["dist"][i, n:]) == 0)
    # the duplicated rows: the lowest index first, at distance exactly 0
    got = dc.match(Q, R, 8, D=D)
    assert list(got["idx"][0, :4]) == [5, 37, 700, 1299] and np.all(got["dist"][0, :4] == 0)
    assert list(got["idx"][1]) == list(range(64, 72)) and np.all(got["dist"][1] == 0)
    # fewer admissible rows than k
    few = dc.match(Q[:3], R[:4], 8)
    assert list(few["cnt"]) == [3, 3, 3] and np.all(few["idx"][:, 3:] == -1) and np.all(few["idx"][:, :3] != 3)


def test_desc_pairs_on_an_object_that_answers_from_the_restatement():
    from fast_limo_amd import api
    rs = np.random.RandomState(4)
    R = dc.random_rows(5, 60, 33)
    # queries: noisy copies of reference rows 0 .. 39 in another order, then rows of their own
    perm = rs.permutation(40)
    Q = np.concatenate([(R[perm] + rs.standard_normal((40, 33)).astype(F) * 0.5).astype(F), dc.random_rows(6, 10, 33)])
    Q[3] = 0                    # an all-zero query row never pairs
    R = R.copy()
    R[perm[5]] = 0              # nor an all-zero reference row, though query 5's nearest row is now whatever it is
    Q[8] = Q[9]                 # two queries on one reference row: the mutual check keeps at most one of them
    for ratio, mutual in ((0.9, True), (0.9, False), (0.5, True), (1.0, True), (1.0, False)):
        qi, rj = api.desc_pairs(dc.Restated(R), dc.Restated(Q), Q, R, ratio=ratio, mutual=mutual)
        wi, wj = dc.pairs(Q, R, ratio, mutual)
        assert qi.dtype == np.int64 and rj.dtype == np.int64
        assert np.array_equal(qi, wi) and np.array_equal(rj, wj), (ratio, mutual)
        assert 3 not in qi and perm[5] not in rj
        if mutual:
            assert len(np.unique(rj)) == len(rj) and not (8 in qi and 9 in qi)
    # the copies pair with their originals
    qi, rj = api.desc_pairs(dc.Restated(R), dc.Restated(Q), Q, R, ratio=0.9, mutual=True)
    true = {(i, int(perm[i])) for i in range(40)}
    found = set(zip(qi.tolist(), rj.tolist()))
    assert len(found & true) >= 30 and len(found - true) <= 3
    # ratio: a stricter one keeps a subset
    strict = set(zip(*[a.tolist() for a in api.desc_pairs(dc.Restated(R), dc.Restated(Q), Q, R, ratio=0.5, mutual=False)]))
    loose = set(zip(*[a.tolist() for a in api.desc_pairs(dc.Restated(R), dc.Restated(Q), Q, R, ratio=1.0, mutual=False)]))
    nearest = dc.match(Q, R, 1)["idx"][:, 0]
    assert strict <= loose and len(strict) < len(loose) == int((Q.any(axis=1) & R[nearest].any(axis=1)).sum())
    # cnt < 2: a single reference row passes the ratio test untested; none at all gives no pair
    qi, rj = api.desc_pairs(dc.Restated(R[:1]), dc.Restated(Q), Q, R[:1], ratio=0.1, mutual=False)
    assert np.array_equal(qi, np.delete(np.arange(50), 3)) and np.all(rj == 0)
    qi, rj = api.desc_pairs(dc.Restated(R[:0]), dc.Restated(Q), Q, R[:0], ratio=0.9, mutual=True)
    assert qi.size == 0 and rj.size == 0


def test_mirror_header_declares_the_descriptor_calls():
    """The mirror's Mapper carries desc_ref_set and desc_match (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
int f(fast_limo::Mapper& map, const float* desc, const float* q, int32_t* idx, float* dist, int32_t* cnt) {
  int rc = map.desc_ref_set(desc, 5000, 33);
  rc += map.desc_match(q, 512, 33, 2, idx, dist, cnt);
  return rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "desc.cpp")
        open(path, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
