"""The consistency graph of correspondences (flimo_corr_graph) as far as it can be checked without a GPU: the restatement's peeling
against the definition of a core number by brute force; the entry points exported, declared and listed; a NULL context rejected by
both libraries; flimo_corr_compatible_host -- the host / device function the adjacency kernel calls, run on the host -- against the
numpy restatement of include/flimo_c.h (tests/corr_graph_common.py) on random pairs and on both sides of every threshold; and the
plumbing of api.corr_prune and api.relocalize(prune=..) through stand-ins.  The call itself runs on the GPU:
tests/test_gpu_corr_graph.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import corr_graph_common as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
NAN = float("nan")


# ---- 1. the yardstick itself ---------------------------------------------------------------------------------------------------------
def test_peeling_gives_the_core_numbers_of_the_definition():
    """400 random graphs of 1 .. 10 vertices at every density, and a few whose answer is known: cores() (peeling) against the largest
    minimum inside degree over all vertex subsets that hold the vertex."""
    rs = np.random.RandomState(0)
    for t in range(400):
        n = 1 + t % 10
        U = np.triu(rs.rand(n, n) < rs.rand(), 1)
        A = U | U.T
        np.testing.assert_array_equal(cg.cores(A), cg.cores_by_definition(A), err_msg=f"graph {t}")
    K5 = ~np.eye(5, dtype=bool)
    assert list(cg.cores(K5)) == [4] * 5
    path = np.zeros((6, 6), bool)
    path[np.arange(5), np.arange(1, 6)] = path[np.arange(1, 6), np.arange(5)] = True
    assert list(cg.cores(path)) == [1] * 6
    tail = np.zeros((6, 6), bool)      # a triangle with a tail of two and an isolated vertex
    for a, b in ((0, 1), (1, 2), (0, 2), (2, 3), (3, 4)):
        tail[a, b] = tail[b, a] = True
    assert list(cg.cores(tail)) == [2, 2, 2, 1, 1, 0] == list(cg.cores_by_definition(tail))
    assert cg.cores(np.zeros((0, 0), bool)).shape == (0,)
    # pack / unpack: bit j & 63 of word j >> 6
    A = np.zeros((70, 70), bool)
    A[1, 0] = A[0, 1] = A[2, 65] = A[65, 2] = True
    P = cg.pack(A)
    assert P.shape == (70, 2) and P.dtype == np.uint64 and P[1, 0] == 1 and P[0, 0] == 2 and P[2, 1] == 2 and P[65, 0] == 4 and P.sum() == 9
    assert np.array_equal(cg.unpack(P, 70)[:, :70], A)


# ---- 2. the entry points -------------------------------------------------------------------------------------------------------------
def test_corr_graph_entry_points_are_exported_declared_and_listed(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    for name in ("flimo_corr_graph", "flimo_corr_compatible_host"):
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS and name + "(" in pub, name
    for word in ("flimo_corr_graph_cfg", "FLIMO_CORR_GRAPH_MAX_M 32768"):
        assert word in pub, word
    H = api.load_host()
    assert hasattr(H, "flimo_loc_corr_graph") and "flimo_loc_corr_graph" in api.HOST_SYMBOLS
    assert "flimo_loc_corr_graph(" in open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for cls in (_lib.HipCtx, api.Localizer):
        assert callable(getattr(cls, "corr_graph"))
    for name in ("corr_prune", "corr_compatible_host"):
        assert callable(getattr(api, name)), name
    assert callable(_lib.corr_graph_cfg) and _lib.HipCtx.corr_graph is api.Localizer.corr_graph      # (one method, two symbols)
    assert C.sizeof(_lib.CorrGraphCfg) == 12 and _lib.CORR_GRAPH_MAX_M == cg.MAX_M == 32768
    k = _lib.corr_graph_cfg()
    assert (k.tol, k.min_edge, k.edge_sim) == (F(0.05), 0.0, 0.0)


def test_corr_graph_rejects_a_null_context_and_the_host_function_its_bad_arguments(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    pts = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    k = _lib.corr_graph_cfg(0.05, 0.1, 0.5)
    deg, core, top, adj = np.full(3, 7, np.int32), np.full(3, 7, np.int32), np.full(1, 7, np.int32), np.full((3, 1), 7, np.uint64)
    args = (pts.ctypes.data, pts.ctypes.data, 3, C.byref(k), deg.ctypes.data, core.ctypes.data, top.ctypes.data, adj.ctypes.data)
    assert L.flimo_corr_graph(None, *args) == -2      # FLIMO_ERR_INVALID
    assert api.load_host().flimo_loc_corr_graph(None, *args) == -2
    for a in (deg, core, top, adj):
        assert np.all(a == 7)
    fn = L.flimo_corr_compatible_host
    p = [pts[0].ctypes.data, pts[1].ctypes.data, pts[0].ctypes.data, pts[2].ctypes.data]
    assert fn(*p, C.byref(k)) == 1
    for at in range(4):
        assert fn(*[None if t == at else v for t, v in enumerate(p)], C.byref(k)) == -2, at
    assert fn(*p, None) == -2
    # every cfg the call rejects: NaN or negative fields, edge_sim above 1, an infinite tol or min_edge
    for bad in ((-0.01, 0.1, 0.5), (NAN, 0.1, 0.5), (INF, 0.1, 0.5), (0.05, -0.1, 0.5), (0.05, NAN, 0.5), (0.05, INF, 0.5), (0.05, 0.1, -0.5),
                (0.05, 0.1, NAN), (0.05, 0.1, 1.0001), (0.05, 0.1, INF), (-INF, 0.1, 0.5)):
        assert fn(*p, C.byref(_lib.corr_graph_cfg(*bad))) == -2, bad
        with pytest.raises(api.FlimoError):
            api.corr_compatible_host(pts[0], pts[1], pts[0], pts[2], tol=bad[0], min_edge=bad[1], edge_sim=bad[2])
    for good in ((0.0, 0.0, 0.0), (0.05, 0.0, 1.0), (3e38, 3e38, 0.0)):
        assert fn(*p, C.byref(_lib.corr_graph_cfg(*good))) in (0, 1), good


# ---- 3. the predicate on the host against the restatement ----------------------------------------------------------------------------
def host_graph(api, src, dst, pairs, **cfg):
    return np.array([api.corr_compatible_host(src[i], src[j], dst[i], dst[j], **cfg) for i, j in pairs], bool)


def test_host_predicate_equals_the_restatement_on_random_pairs(built):
    """4 000 pairs i != j of a planted scene of 300 correspondences under three cfgs: every answer is the restatement's, both ways
    round (the predicate is symmetric), and both answers occur."""
    from fast_limo_amd import api
    src, dst, true = cg.planted(300, 5)
    rs = np.random.RandomState(1)
    pairs = rs.randint(0, 300, (4000, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    pairs = np.concatenate([pairs, np.stack(np.nonzero(np.outer(true, true) & ~np.eye(300, dtype=bool)), 1)[:500]])
    for cfg in (cg.CFG, dict(tol=0.3, min_edge=0.0, edge_sim=0.95), dict(tol=0.0, min_edge=0.0, edge_sim=0.0), dict(tol=2.0, min_edge=3.0, edge_sim=0.8)):
        A = cg.graph(src, dst, **cfg)
        want = A[pairs[:, 0], pairs[:, 1]]
        got = host_graph(api, src, dst, pairs, **cfg)
        np.testing.assert_array_equal(got, want, err_msg=str(cfg))
        np.testing.assert_array_equal(host_graph(api, src, dst, pairs[:, ::-1], **cfg), want, err_msg=f"{cfg}, j before i")
        np.testing.assert_array_equal(A, A.T)
        print(cfg, "edges among the pairs:", int(want.sum()), "of", want.size)
        assert cfg["tol"] == 0.0 or 0 < want.sum() < want.size
    assert cg.graph(src, dst, **cg.CFG)[np.ix_(true, true)].sum() >= 0.9 * (true.sum() * (true.sum() - 1))      # the planted pairs: nearly a clique


def both(api, si, sj, di, dj, want, tag, **cfg):
    """The host function and the restatement on ONE pair of correspondences, in both orders; ``want``: the answer known by hand."""
    src, dst = F([si, sj]), F([di, dj])
    A = cg.graph(src, dst, **cfg)
    assert A[0, 1] == A[1, 0] == want and not A[0, 0] and not A[1, 1], tag
    assert api.corr_compatible_host(src[0], src[1], dst[0], dst[1], **cfg) == want, tag
    assert api.corr_compatible_host(src[1], src[0], dst[1], dst[0], **cfg) == want, f"{tag}, exchanged"
    assert api.corr_compatible_host(dst[0], dst[1], src[0], src[1], **cfg) == want, f"{tag}, clouds exchanged"


def test_host_predicate_on_both_sides_of_every_threshold(built):
    from fast_limo_amd import api
    o = (0, 0, 0)
    up, down = (lambda v: np.nextafter(F(v), F(INF))), (lambda v: np.nextafter(F(v), F(-INF)))
    # the 3-4-5 case: the src edge (3, 4, 0) is exactly 5 m long, the dst edge exactly 4 m: the difference is 1.0.  tol = 1.0 passes,
    # the float32 below does not; the same for edges of exactly 3 m and 4 m
    for sj, dj in (((3, 4, 0), (0, 0, 4)), ((3, 0, 0), (0, 4, 0)), ((0, -3, 0), (4, 0, 0))):
        both(api, o, sj, o, dj, True, "difference at tol", tol=1.0, min_edge=0.0, edge_sim=0.0)
        both(api, o, sj, o, dj, False, "difference above tol", tol=down(1.0), min_edge=0.0, edge_sim=0.0)
        both(api, o, sj, o, dj, True, "tol one step wider", tol=up(1.0), min_edge=0.0, edge_sim=0.0)
    # ... and with tol fixed, the point moved: 4 m against 3 m + one float32 step is inside, against 3 m - one step outside
    both(api, o, (up(3.0), 0, 0), o, (0, 4, 0), True, "edge one step longer", tol=1.0, min_edge=0.0, edge_sim=0.0)
    both(api, o, (down(3.0), 0, 0), o, (0, 4, 0), False, "edge one step shorter", tol=1.0, min_edge=0.0, edge_sim=0.0)
    both(api, o, (3, 0, 0), o, (0, 3, 0), True, "tol 0 on equal edges", tol=0.0, min_edge=0.0, edge_sim=0.0)
    both(api, o, (3, 0, 0), o, (0, up(3.0), 0), False, "tol 0 on edges one step apart", tol=0.0, min_edge=0.0, edge_sim=0.0)
    # min_edge: an edge exactly at it passes (0.25 >= 0.5 * 0.5), one float32 step shorter does not -- in either cloud
    both(api, o, (0.5, 0, 0), o, (0, 0.5, 0), True, "edges at min_edge", tol=0.1, min_edge=0.5, edge_sim=0.0)
    both(api, o, (down(0.5), 0, 0), o, (0, 0.5, 0), False, "an edge below min_edge", tol=0.1, min_edge=0.5, edge_sim=0.0)
    both(api, o, (0.5, 0, 0), o, (0, 0.5, 0), False, "min_edge one step above", tol=0.1, min_edge=up(0.5), edge_sim=0.0)
    both(api, o, (down(0.5), 0, 0), o, (0, 0.5, 0), True, "no shortest edge", tol=0.1, min_edge=0.0, edge_sim=0.0)
    # edge_sim: edges of 1 m and 2 m at 0.5 pass (1 >= 0.25 * 4), one step longer they do not
    both(api, o, (1, 0, 0), o, (0, 2, 0), True, "similarity at the threshold", tol=1.5, min_edge=0.0, edge_sim=0.5)
    both(api, o, (1, 0, 0), o, (0, up(2.0), 0), False, "similarity below the threshold", tol=1.5, min_edge=0.0, edge_sim=0.5)
    both(api, o, (1, 0, 0), o, (0, 2, 0), False, "edge_sim one step above", tol=1.5, min_edge=0.0, edge_sim=up(0.5))
    both(api, o, (1, 0, 0), o, (0, up(2.0), 0), True, "no polygon test", tol=1.5, min_edge=0.0, edge_sim=0.0)
    both(api, o, (1, 2, 3), (5, 5, 5), (6, 7, 8), True, "edge_sim 1 keeps equal edges", tol=0.0, min_edge=0.0, edge_sim=1.0)


def test_host_predicate_of_nan_infinite_and_coinciding_points(built):
    from fast_limo_amd import api
    o, a, b = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    loose = dict(tol=1e30, min_edge=0.0, edge_sim=0.0)
    for at in range(3):
        bad = list(a)
        bad[at] = NAN
        both(api, o, bad, o, b, False, "NaN in src", **loose)
        both(api, bad, a, o, b, False, "NaN in src, the other point", **loose)
        both(api, o, a, o, bad, False, "NaN in dst", **loose)
        bad[at] = INF
        both(api, o, bad, o, b, False, "an infinite coordinate", **loose)
        both(api, o, bad, o, bad, False, "two infinite edges", **loose)
    # i == j is the call's rule: the restatement's diagonal is empty, whatever the function says of a point paired with itself
    A = cg.graph(F([a, a]), F([b, b]), **loose)
    assert not A[0, 0] and not A[1, 1] and A[0, 1]      # (two DIFFERENT pairs of equal points are compatible without a shortest edge)
    assert api.corr_compatible_host(a, a, b, b, **loose) is True
    assert api.corr_compatible_host(a, a, b, b, tol=1.0, min_edge=1e-3, edge_sim=0.0) is False
    # several scan points paired with ONE map point: e_d = 0 fails a shortest edge
    both(api, o, a, b, b, False, "two pairs sharing their dst", tol=10.0, min_edge=0.1, edge_sim=0.0)
    both(api, o, a, b, b, True, "... without a shortest edge", tol=10.0, min_edge=0.0, edge_sim=0.0)
    both(api, o, a, b, b, False, "... the polygon test fails a zero edge against a real one", tol=10.0, min_edge=0.0, edge_sim=0.1)


# ---- 4. the plumbing -----------------------------------------------------------------------------------------------------------------
class _Graph:
    """``corr_graph`` by the restatement, recording its calls."""

    def __init__(self):
        self.calls = []

    def corr_graph(self, src, dst, want=(), **cfg):
        self.calls.append(dict(src=np.array(src), dst=np.array(dst), want=tuple(want), cfg=dict(cfg)))
        ref = cg.reference(src, dst, **cfg)
        return dict(degree=ref["degree"], core=ref["core"], max_core=int(ref["core"].max()))


def test_corr_prune_selects_by_core_number():
    from fast_limo_amd import api
    src, dst, true = cg.planted(120, 3)
    core = cg.cores(cg.graph(src, dst, **cg.CFG))
    obj = _Graph()
    out = api.corr_prune(obj, src, dst, **cg.CFG)
    assert sorted(out) == ["core", "degree", "keep", "max_core"] and out["keep"].dtype == np.int64
    assert out["max_core"] == core.max() and np.array_equal(out["core"], core)
    assert np.array_equal(out["keep"], np.nonzero(core == core.max())[0]) and np.all(true[out["keep"]])
    assert len(obj.calls) == 1 and obj.calls[0]["cfg"] == cg.CFG and obj.calls[0]["want"] == () and np.array_equal(obj.calls[0]["dst"], dst)
    for level in (0, 1, 3, int(core.max()), int(core.max()) + 1):
        out = api.corr_prune(obj, src, dst, min_core=level, **cg.CFG)
        assert np.array_equal(out["keep"], np.nonzero(core >= level)[0]), level
    assert api.corr_prune(obj, src, dst, min_core=0, **cg.CFG)["keep"].size == 120
    # no pairs: nothing is called
    n = len(obj.calls)
    out = api.corr_prune(obj, np.zeros((0, 3), F), np.zeros((0, 3), F), tol=0.1)
    assert len(obj.calls) == n and out["max_core"] == 0
    for name, dt in (("keep", np.int64), ("core", np.int32), ("degree", np.int32)):
        assert out[name].shape == (0,) and out[name].dtype == dt


class _Ctx:
    """What api.relocalize asks of a context, canned."""

    def __init__(self, pts):
        self.pts, self.log = pts, []

    def map_fpfh(self, want=(), **cfg):
        return dict(fpfh=np.ones((len(self.pts), 33), F))

    def desc_ref_set(self, desc):
        self.log.append("desc_ref_set")

    def map_points(self):
        return self.pts

    def scan_fitness(self, x26s, max_dist):
        n = len(x26s)
        return np.arange(n, dtype=np.int32), np.zeros(n)

    def scan_size(self):
        return 10


@pytest.fixture
def canned(monkeypatch):
    """relocalize's stages replaced by recorders: (map stand-in, scan stand-in, the log of (stage, arguments))."""
    from fast_limo_amd import api
    rs = np.random.RandomState(2)
    map_obj, scan_obj = _Ctx(rs.rand(50, 3).astype(F)), _Ctx(rs.rand(30, 3).astype(F))
    log = []
    qi, rj = np.int64([1, 4, 5, 9, 20, 29]), np.int64([7, 0, 49, 3, 3, 11])
    monkeypatch.setattr(api, "desc_pairs", lambda *a, **k: (qi, rj))

    def prune(obj, src, dst, **kw):
        log.append(("prune", obj, np.array(src), np.array(dst), kw))
        return dict(keep=np.int64([0, 2, 5]), core=np.int32([2, 0, 2, 1, 0, 2]), degree=np.int32([2, 0, 2, 1, 0, 2]), max_core=2)

    def consensus(obj, src, dst, nh, **kw):
        log.append(("consensus", obj, np.array(src), np.array(dst), nh))
        x = np.zeros((2, 26))
        x[:, 6] = x[:, 10] = 1.0
        return dict(x26=x, tri=np.int32([[0, 1, 2], [2, 1, 0]]))
    monkeypatch.setattr(api, "corr_prune", prune)
    monkeypatch.setattr(api, "corr_consensus", consensus)
    monkeypatch.setattr(api, "scan_align", lambda obj, x, **k: dict(x26=np.array(x)))
    return map_obj, scan_obj, log, qi, rj


def test_relocalize_without_prune_takes_the_unpruned_route(canned):
    from fast_limo_amd import api
    map_obj, scan_obj, log, qi, rj = canned
    for kw in ({}, dict(prune=None)):
        del log[:]
        out = api.relocalize(map_obj, scan_obj, nh=64, **kw)
        assert [e[0] for e in log] == ["consensus"] and "prune" not in out
        assert np.array_equal(log[0][2], scan_obj.pts[qi]) and np.array_equal(log[0][3], map_obj.pts[rj]) and log[0][4] == 64
        assert np.array_equal(out["src"], scan_obj.pts[qi]) and np.array_equal(out["dst"], map_obj.pts[rj])
        assert sorted(out) == ["align", "consensus", "dst", "fitness", "fpfh", "pairs", "src", "x26"]


def test_relocalize_with_prune_samples_from_the_kept_pairs_alone(canned):
    from fast_limo_amd import api
    map_obj, scan_obj, log, qi, rj = canned
    out = api.relocalize(map_obj, scan_obj, nh=64, prune=dict(tol=0.06, min_edge=0.5, min_core=2))
    assert [e[0] for e in log] == ["prune", "consensus"]
    stage, obj, src, dst, kw = log[0]
    assert obj is map_obj and kw == dict(tol=0.06, min_edge=0.5, min_core=2)
    assert np.array_equal(src, scan_obj.pts[qi]) and np.array_equal(dst, map_obj.pts[rj])
    keep = np.int64([0, 2, 5])
    assert np.array_equal(log[1][2], scan_obj.pts[qi][keep]) and np.array_equal(log[1][3], map_obj.pts[rj][keep])
    # what comes back is unpruned, with the prune stage's own dict next to it
    assert np.array_equal(out["pairs"][0], qi) and np.array_equal(out["pairs"][1], rj)
    assert np.array_equal(out["src"], scan_obj.pts[qi]) and np.array_equal(out["dst"], map_obj.pts[rj])
    assert np.array_equal(out["prune"]["keep"], keep) and out["prune"]["max_core"] == 2
    # an empty dict prunes with corr_prune's defaults
    del log[:]
    api.relocalize(map_obj, scan_obj, nh=64, prune={})
    assert [e[0] for e in log] == ["prune", "consensus"] and log[0][4] == {}


def test_mirror_header_declares_corr_graph():
    """The mirror's Mapper carries corr_graph (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
int f(fast_limo::Mapper& map, const float* src, const float* dst, int32_t* degree, int32_t* core, int32_t* top, uint64_t* adj) {
  flimo_corr_graph_cfg cfg{0.05f, 0.5f, 0.0f};
  int rc = map.corr_graph(src, dst, 512, &cfg, degree, core);
  rc += map.corr_graph(src, dst, 512, &cfg, degree, core, top, adj);
  return rc + (FLIMO_CORR_GRAPH_MAX_M == 32768 ? 0 : 1);
}
"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corr_graph.cpp")
        open(path, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
