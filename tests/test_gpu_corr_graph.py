"""GPU: flimo_corr_graph (the consistency graph of point correspondences and its core numbers) through the C ABI, api.corr_prune over it
and api.relocalize(prune=..) over that.

The yardstick (tests/corr_graph_common.py) is the definition of include/flimo_c.h restated in numpy: the dense predicate in float64
and plain peeling.  Every output is an integer or a bit and is compared exactly; wherever two calls must give the same result the
arrays are compared byte for byte.  Nothing here depends on how the device finds the core numbers."""
import ctypes as C
import functools

import numpy as np
import pytest

import corr_common as cc
import corr_graph_common as cg
import fpfh_common as fc
import scan_fitness_common as sf
import scan_linearize_common as sl
from common import CAPS

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5
F = np.float32
INF, NAN = float("inf"), float("nan")
# The sizes the issue names, and the ones the launches divide at: an adjacency tile is 64 rows by 64 columns (one word), a workgroup
# takes four words (256 columns) of 64 rows; the degree and core kernels put 4 vertices (one per wave) into a workgroup; a wave of the
# core kernel scans a row 64 words (4 096 columns) at a trip, so 4 097 vertices are the first to need a second trip.
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
TIGHT = dict(tol=0.3, min_edge=0.0, edge_sim=0.97)      # a second cfg: the polygon test decides, no shortest edge


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device; an empty context will do
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def scene600():
    """600 pairs with a planted rigid subset and their restated graph: what the invariance tests compare against."""
    src, dst, true = cg.planted(600, 21)
    ref = cg.reference(src, dst, **cg.CFG)
    return src, dst, true, ref


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_against_the_restatement(hip, m):
    """Random clouds with a planted rigid subset (about 30 % of the pairs): adj is pack(graph(..)) with zero padding bits and
    symmetric, degree the row popcounts, core and max_core the peeling's."""
    src, dst, true = cg.planted(m, m)
    cfgs = (cg.CFG,) if m > 1000 else (cg.CFG, TIGHT)
    for cfg in cfgs:
        ref = cg.reference(src, dst, **cfg)
        got = hip.corr_graph(src, dst, want=("adj",), **cfg)
        print(f"m {m}, {cfg}: {int(ref['degree'].sum()) // 2} edges, max degree {ref['degree'].max()}, max core {ref['core'].max()}, "
              f"{int(true.sum())} planted")
        cg.check(got, ref["A"], f"m {m}, {cfg}", core=ref["core"])
        if m >= 63:
            assert ref["core"].max() >= 0.8 * (true.sum() - 1) and len(np.unique(ref["core"])) >= (3 if m >= 255 else 2)


def test_one_larger_case(hip):
    """4 096 pairs of which 3 % are true over the FPFH scene's points (a 2 MB matrix, tens of rounds on the device)."""
    src, dst, true = cc.scene(9, fc.scene(), m=4096, keep=0.03, noise=0.014)
    cfg = dict(tol=0.06, min_edge=0.5, edge_sim=0.0)
    ref = cg.reference(src, dst, **cfg)
    got = hip.corr_graph(src, dst, want=("adj",), **cfg)
    print(f"{int(true.sum())} true pairs, {int(ref['degree'].sum()) // 2} edges, max core {ref['core'].max()}, core levels {len(np.unique(ref['core']))}")
    cg.check(got, ref["A"], "m 4096", core=ref["core"])
    assert len(np.unique(ref["core"])) >= 10


# ---- 2. shapes whose answer is known by hand -----------------------------------------------------------------------------------------
def test_a_complete_graph_of_true_pairs(hip):
    rs = np.random.RandomState(3)
    src = ((rs.rand(130, 3) - 0.5) * 20).astype(F)
    dst = cg.moved(src, 3)
    got = hip.corr_graph(src, dst, want=("adj",), tol=0.01, min_edge=0.0, edge_sim=0.9)
    assert np.all(got["degree"] == 129) and np.all(got["core"] == 129) and got["max_core"] == 129
    cg.check(got, ~np.eye(130, dtype=bool), "complete")


def test_two_rigid_groups_far_apart(hip):
    """40 pairs under one motion and 25 under another, the groups 1 km apart in dst: an edge between the groups is about as long as
    the distance in src and about 1 km in dst.  Two cliques: cores 39 and 24."""
    rs = np.random.RandomState(4)
    src = ((rs.rand(65, 3) - 0.5) * 20).astype(F)
    dst = np.concatenate([cg.moved(src[:40], 1), cg.moved(src[40:], 2, t=(1000.0, 0.0, 0.0))])
    order = rs.permutation(65)
    got = hip.corr_graph(src[order], dst[order], want=("adj",), tol=0.01, min_edge=0.0, edge_sim=0.0)
    first = order < 40
    assert np.all(got["core"][first] == 39) and np.all(got["core"][~first] == 24) and got["max_core"] == 39
    assert np.array_equal(got["degree"], got["core"])
    A = np.equal.outer(first, first) & ~np.eye(65, dtype=bool)
    cg.check(got, A, "two groups")
    np.testing.assert_array_equal(cg.graph(src[order], dst[order], tol=0.01), A)


def test_tol_zero_on_random_clouds_leaves_no_edge(hip):
    src = ((np.random.RandomState(8).rand(300, 3) - 0.5) * 10).astype(F)
    dst = ((np.random.RandomState(80).rand(300, 3) - 0.5) * 10).astype(F)
    assert not cg.graph(src, dst, tol=0.0).any()
    got = hip.corr_graph(src, dst, want=("adj",), tol=0.0, min_edge=0.0, edge_sim=0.0)
    assert not got["adj"].any() and not got["degree"].any() and not got["core"].any() and got["max_core"] == 0
    cg.check(got, cg.graph(src, dst, tol=0.0), "tol 0")


def test_the_chain(hip):
    """257 vertices in one path: degrees 1, 2, .., 2, 1 and every core number 1.  An h-index iteration needs 128 rounds that change an
    estimate and one that does not here, the most of any graph in this suite; peeling needs one level."""
    src, dst, cfg = cg.chain(257)
    A = cg.graph(src, dst, **cfg)
    path = np.abs(np.subtract.outer(np.arange(257), np.arange(257))) == 1
    np.testing.assert_array_equal(A, path)
    got = hip.corr_graph(src, dst, want=("adj",), **cfg)
    assert list(got["degree"]) == [1] + [2] * 255 + [1] and np.all(got["core"] == 1) and got["max_core"] == 1
    cg.check(got, path, "chain")


def test_pairs_sharing_one_map_point_are_never_compatible(hip):
    rs = np.random.RandomState(6)
    src = ((rs.rand(20, 3) - 0.5) * 10).astype(F)
    dst = np.tile(F([[1.0, 2.0, 3.0]]), (20, 1))
    got = hip.corr_graph(src, dst, want=("adj",), tol=100.0, min_edge=0.1, edge_sim=0.0)
    assert not got["adj"].any() and not got["degree"].any() and not got["core"].any() and got["max_core"] == 0
    # ... among good pairs: they hang on the clique one at a time
    good = ((rs.rand(30, 3) - 0.5) * 10).astype(F)
    s2, d2 = np.concatenate([good, src]), np.concatenate([cg.moved(good, 6), cg.moved(src[:1], 6).repeat(20, 0)])
    got = hip.corr_graph(s2, d2, want=("adj",), tol=0.01, min_edge=0.1, edge_sim=0.0)
    ref = cg.reference(s2, d2, tol=0.01, min_edge=0.1, edge_sim=0.0)
    cg.check(got, ref["A"], "many to one among good pairs", core=ref["core"])
    assert not ref["A"][30:, 30:].any() and np.all(got["core"][:30] >= 29) and np.all(got["core"][31:] <= 2)


def test_nan_rows_are_isolated_and_the_others_do_not_see_them(hip):
    src, dst, _, ref = scene600()
    s, d = src.copy(), dst.copy()
    bad = np.array([0, 63, 64, 300, 599])
    s[bad[0], 1] = s[bad[1], 0] = NAN
    d[bad[2], 2] = d[bad[3], 0] = NAN
    s[bad[4]] = NAN
    d[bad[4]] = NAN
    got = hip.corr_graph(s, d, want=("adj",), **cg.CFG)
    cg.check(got, cg.graph(s, d, **cg.CFG), "NaN rows")
    assert not got["degree"][bad].any() and not got["core"][bad].any() and not got["adj"][bad].any()
    rest = np.setdiff1d(np.arange(600), bad)
    clean = hip.corr_graph(src[rest], dst[rest], **cg.CFG)
    assert np.array_equal(got["degree"][rest], clean["degree"]) and np.array_equal(got["core"][rest], clean["core"])
    assert got["max_core"] == clean["max_core"]


# ---- 3. the call moves nothing -------------------------------------------------------------------------------------------------------
def test_repetition_another_context_the_outputs_asked_for_and_a_larger_call_before(built, hip):
    from fast_limo_amd import _lib
    src, dst, _, ref = scene600()
    first = hip.corr_graph(src, dst, want=("adj",), **cg.CFG)
    cg.check(first, ref["A"], "600 pairs", core=ref["core"])
    cg.same_bytes(first, hip.corr_graph(src, dst, want=("adj",), **cg.CFG), "called twice")
    plain = hip.corr_graph(src, dst, **cg.CFG)
    assert sorted(plain) == ["core", "degree", "max_core"]
    cg.same_bytes(plain, first, "without adj", names=sorted(plain))
    big_s, big_d, _ = cg.planted(1500, 33, share=0.6)      # (a denser, larger graph first: stale scratch would show)
    assert hip.corr_graph(big_s, big_d, want=("adj",), **cg.CFG)["max_core"] > first["max_core"]
    cg.same_bytes(first, hip.corr_graph(src, dst, want=("adj",), **cg.CFG), "after a larger call")
    small = hip.corr_graph(src[:70], dst[:70], want=("adj",), **cg.CFG)
    cg.check(small, ref["A"][:70, :70], "a prefix after it")
    other = _lib.HipCtx(0)
    try:
        cg.same_bytes(first, other.corr_graph(src, dst, want=("adj",), **cg.CFG), "a second context")
    finally:
        other.close()
    # through ctypes: max_core and adj may be left out
    L = _lib.load_hip()
    k = _lib.corr_graph_cfg(**cg.CFG)
    deg, core = np.zeros(600, np.int32), np.zeros(600, np.int32)
    assert L.flimo_corr_graph(hip._h, src.ctypes.data, dst.ctypes.data, 600, C.byref(k), deg.ctypes.data, core.ctypes.data, None, None) == 0
    assert np.array_equal(deg, first["degree"]) and np.array_equal(core, first["core"])


def test_the_call_touches_neither_the_map_nor_the_scan_nor_a_later_pass(built):
    """Against a twin context that never makes the call: the pass before and the pass after have the twin's HTH / HTh bits."""
    from fast_limo_amd import _lib
    mp = fc.scene()
    scan = np.ascontiguousarray(mp[::3] + F([0.01, -0.01, 0.005]))
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    src, dst, _, ref = scene600()

    def run(graphing):
        h = _lib.HipCtx(0)
        try:
            h.map_config(0.2, 2, True, 0.0)
            h.map_add(mp, stamp=0.5)
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if graphing:
                cg.check(h.corr_graph(src, dst, want=("adj",), **cg.CFG), ref["A"], "on a context with a map", core=ref["core"])
            out.append(h.match_reduce(x, mcfg))
            return out, h.map_size(), h.map_points().copy(), h.scan_get().copy()
        finally:
            h.close()

    (plain, pn, pm, ps), (graphed, gn, gm, gs) = run(False), run(True)
    assert pn == gn == len(mp) and pm.tobytes() == gm.tobytes() == mp.tobytes() and ps.tobytes() == gs.tobytes() == scan.tobytes()
    for a, b in zip(plain, graphed):
        assert a[2] == b[2] > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_localizer_forwards(hip):
    from fast_limo_amd import api
    src, dst, _, ref = scene600()
    first = hip.corr_graph(src, dst, want=("adj",), **cg.CFG)
    loc = api.Localizer(api.default_cfg())
    try:
        cg.same_bytes(first, loc.corr_graph(src, dst, want=("adj",), **cg.CFG), "Localizer with no map")
        loc.map_add(np.concatenate(sf.standard_batches()[:1]))
        size = loc.map_size()
        cg.same_bytes(first, loc.corr_graph(src, dst, want=("adj",), **cg.CFG), "Localizer with a map")
        assert loc.map_size() == size
        pruned = api.corr_prune(loc, src, dst, **cg.CFG)
        assert np.array_equal(pruned["keep"], np.nonzero(ref["core"] == ref["core"].max())[0])
        with pytest.raises(api.FlimoError):
            loc.corr_graph(src, dst, tol=-1.0)
    finally:
        loc.close()


# ---- 4. rejected arguments and the limit ---------------------------------------------------------------------------------------------
def test_rejected_arguments_and_the_limit_leave_the_outputs_alone(hip):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    src, dst, _, ref = scene600()
    m, W = 600, 10
    deg, core, top, adj = np.full(m, 7, np.int32), np.full(m, 7, np.int32), np.full(1, 7, np.int32), np.full((m, W), 7, np.uint64)
    good = _lib.corr_graph_cfg(**cg.CFG)

    def call(src_p=src.ctypes.data, dst_p=dst.ctypes.data, m_=m, cfg=good, deg_p=deg.ctypes.data, core_p=core.ctypes.data, top_p=top.ctypes.data,
             adj_p=adj.ctypes.data):
        return L.flimo_corr_graph(hip._h, src_p, dst_p, m_, None if cfg is None else C.byref(cfg), deg_p, core_p, top_p, adj_p)
    for kw in (dict(src_p=None), dict(dst_p=None), dict(cfg=None), dict(deg_p=None), dict(core_p=None)):
        assert call(**kw) == ERR_INVALID, kw
    for bad in ((-0.01, 0.5, 0.0), (NAN, 0.5, 0.0), (INF, 0.5, 0.0), (0.05, -0.5, 0.0), (0.05, NAN, 0.0), (0.05, INF, 0.0), (0.05, 0.5, -0.1),
                (0.05, 0.5, NAN), (0.05, 0.5, 1.0001), (0.05, 0.5, INF)):
        assert call(cfg=_lib.corr_graph_cfg(*bad)) == ERR_INVALID, bad
    # one past the limit is refused before anything is read or launched: the arrays hold 600 pairs
    assert call(m_=cg.MAX_M + 1) == ERR_TOO_LARGE and b"at most" in L.flimo_last_error(hip._h)
    assert call(m_=2 ** 40) == ERR_TOO_LARGE
    for a in (deg, core, top, adj):
        assert np.all(a == 7)
    assert call(m_=0) == 0 and call(m_=0, src_p=None, dst_p=None) == 0
    for a in (deg, core, top, adj):
        assert np.all(a == 7)
    # the arrays were good all along; the optional ones may be left out
    assert call(top_p=None, adj_p=None) == 0 and np.all(top == 7) and np.all(adj == 7) and np.array_equal(core, ref["core"])
    assert call() == 0
    cg.check(dict(degree=deg, core=core, max_core=int(top[0]), adj=adj), ref["A"], "through ctypes", core=ref["core"])
    with pytest.raises(ValueError):
        hip.corr_graph(src, dst, want=("core",), **cg.CFG)
    with pytest.raises(ValueError):
        hip.corr_graph(src, dst[:-1], **cg.CFG)
    with pytest.raises(_lib.FlimoError):
        hip.corr_graph(src, dst, edge_sim=2.0)
    empty = hip.corr_graph(np.zeros((0, 3), F), np.zeros((0, 3), F), want=("adj",))
    assert empty["degree"].shape == empty["core"].shape == (0,) and empty["adj"].shape == (0, 0) and empty["max_core"] == 0


# ---- 5. recovery on synthetic pairs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_recovery_from_six_percent_true_pairs(hip, seed):
    """1 400 pairs of which about 6 % are true (noise 0.014 m), the rest random points of the FPFH scene: the share
    tests/test_gpu_desc.py meets on real descriptors.  Pruned to the innermost core at tol 0.06 m, min_edge 0.5 m: every kept pair
    is true and at least 90 % of the true ones are kept (the restatement: 100, 98, 100, 99 %); corr_consensus on the kept pairs
    with 2 048 samples puts its first row within tests/test_gpu_corr.py's first bar, 0.05 m and 0.5 degrees (the restatement:
    0.0073 m, 0.035 degrees at worst).  Unpruned, 2 048 samples hold 0.44 all-true triplets on average."""
    from fast_limo_amd import api
    src, dst, true = cc.scene(seed, fc.scene(), m=1400, keep=0.06, noise=0.014)
    pruned = api.corr_prune(hip, src, dst, tol=0.06, min_edge=0.5)
    keep = pruned["keep"]
    A = cg.graph(src, dst, tol=0.06, min_edge=0.5)
    core = cg.cores(A)
    assert np.array_equal(pruned["core"], core) and np.array_equal(pruned["degree"], A.sum(1)) and pruned["max_core"] == core.max()
    assert np.array_equal(keep, np.nonzero(core == core.max())[0])
    print(f"seed {seed}: {int(true.sum())} true pairs of 1400, max core {pruned['max_core']}, kept {keep.size}, of them true {int(true[keep].sum())}")
    assert np.all(true[keep])
    assert keep.size >= 0.9 * true.sum()
    best = api.corr_consensus(hip, src[keep], dst[keep], 2048, seed=seed, edge_sim=0.9, min_edge=1.5, max_dist=0.15)
    dt, dr = cc.pose_error(best["x26"][0], sf.x26_of())
    print(f"seed {seed}: {best['survivors']} survivors, best has {best['inliers'][0]} inliers of {keep.size}, off by {dt:.4f} m, {dr:.3f} deg")
    assert dt <= 0.05 and dr <= 0.5


# ---- 6. the chain: relocalize with the pruning between the pairs and the samples ----------------------------------------------------
# tests/test_gpu_desc.py's scene and parameters (imported, not restated): unpruned, 6 % of the pairs are true and the chain needs 2^20
# samples.  Measured on an MI355X, seeds 0 - 2, nh = 2^4 .. 2^18 (profiles/corr_graph/README.md has the table):
#  - tol 0.04 m, min_edge 0.5 m: the innermost core holds 57 / 59 / 52 pairs, ALL true (of 96 / 85 / 88 true among 1 448 / 1 394 /
#    1 422).  Every seed meets both bars at nh = 2^4; seed 1 misses the first at 2^5 (0.70 degrees: with every sample all true the
#    bar is about the accuracy of a pose from three pairs 2.4 cm off, which the scan_fitness ranking picks among few), and from 2^6
#    on every nh tried meets them on every seed.  The test uses four times that: 2^8, 4 096 times fewer samples than unpruned.
#  - tol 0.03 m does the same with 57 / 55 / 48 pairs; tol 0.06 m keeps 245 / 380 / 109 pairs of which 38 / 22 / 71 % are true (false
#    pairs shifted along a plane are consistent with each other and with a part of the true ones): all three seeds meet the bars
#    at 2^12 alone; tol 0.1 m (53 / 22 / 52 % true): at 2^11, 2^13 and 2^15 .. 2^17; min_edge 1.0 m at tol 0.06 m (58 / 17 / 63 %):
#    at 2^11 alone.  A core that is not all true is no basis for a test; the tolerance has to be below the false pairs' slack.
CHAIN_PRUNE = dict(tol=0.04, min_edge=0.5)
CHAIN_NH = 1 << 8


@pytest.mark.parametrize("s", [0, 1, 2])
def test_relocalize_with_pruned_pairs(s):
    from fast_limo_amd import api
    import test_gpu_desc as gd
    body, world, x_true = gd.body_scan(s)
    map_ctx, scan_ctx = gd._map_ctx(fc.scene()), gd._map_ctx(body)
    try:
        map_ctx.scan_set(body)
        out = api.relocalize(map_ctx, scan_ctx, fpfh=dict(gd.CHAIN_FPFH, viewpoint=gd.TRUE_T), scan_fpfh=dict(gd.CHAIN_FPFH, viewpoint=(0.0, 0.0, 0.0)),
                             seed=s, prune=CHAIN_PRUNE, **dict(gd.RELOC, nh=CHAIN_NH))
        qi, rj = out["pairs"]
        keep = out["prune"]["keep"]
        true = np.linalg.norm(world[qi].astype(np.float64) - fc.scene()[rj].astype(np.float64), axis=1) < 0.1
        dt1, dr1 = cc.pose_error(out["fitness"]["x26"][0], x_true)
        dt2, dr2 = cc.pose_error(out["x26"], x_true)
        print(f"seed {s}: {len(qi)} pairs, {int(true.sum())} true ({true.mean():.3f}); max core {out['prune']['max_core']}, kept {keep.size}, "
              f"{int(true[keep].sum())} true ({true[keep].mean() if keep.size else 0.0:.3f}); nh {CHAIN_NH}, survivors {out['consensus']['survivors']}; "
              f"ranked first {dt1:.4f} m {dr1:.3f} deg; aligned {dt2 * 1e3:.2f} mm {dr2:.4f} deg")
        # the relations that hold by construction: the unpruned pairs come back, the pruning is corr_prune's, the consensus saw the kept pairs
        assert np.array_equal(out["src"], body[qi]) and np.array_equal(out["dst"], fc.scene()[rj])
        by_hand = api.corr_prune(map_ctx, out["src"], out["dst"], **CHAIN_PRUNE)
        cg.same_bytes(by_hand, out["prune"], "corr_prune by hand")
        cons = api.corr_consensus(map_ctx, out["src"][keep], out["dst"][keep], CHAIN_NH, seed=s, top=gd.RELOC["top"], **gd.RELOC["corr"])
        assert np.array_equal(cons["tri"], out["consensus"]["tri"]) and np.array_equal(cons["x26"], out["consensus"]["x26"])
        assert out["consensus"]["tri"].max() < keep.size
        # the existing test's own bars
        assert dt1 <= 0.05 and dr1 <= 0.5
        assert dt2 <= sl.POS_BAR and dr2 <= sl.ROT_BAR_DEG
    finally:
        map_ctx.close()
        scan_ctx.close()
