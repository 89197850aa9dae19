"""Outlier removal by neighbour statistics (flimo_map_outliers / flimo_map_remove_outliers) as far as it can be checked without a GPU:
both libraries export and declare the new entry points, the calls reject a null context, and the numpy yardstick
(tests/outliers_common.py) has the properties the GPU tests lean on -- the self rule's special cases occur in the scene, the gated
configurations hold points without a neighbour, no mean distance of any configuration the GPU tests run lies within 1e-9 relative of
its threshold, and a tree-shaped sum stays within the derived bound of math.fsum.  The kernels run on the GPU:
tests/test_gpu_outliers.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import outliers_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
INF = float("inf")

HIP_NAMES = ("flimo_map_outliers", "flimo_map_remove_outliers", "flimo_set_outlier_chunk")
HOST_NAMES = ("flimo_loc_map_outliers", "flimo_loc_map_remove_outliers")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in HIP_NAMES:
        getattr(L, name)
    for name in HOST_NAMES:
        getattr(H, name)


def test_new_entry_points_are_exported_and_declared():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    dev = open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in HIP_NAMES:
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS, name
    assert "flimo_map_outliers" in pub and "flimo_map_remove_outliers" in pub and "flimo_set_outlier_chunk" in dev
    assert "flimo_outlier_cfg" in pub and "flimo_outlier_stats" in pub
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name in decl, name
    for name in ("map_outliers", "map_remove_outliers", "set_outlier_chunk"):
        assert hasattr(_lib.HipCtx, name), name
    for name in ("map_outliers", "map_remove_outliers"):
        assert hasattr(api.Localizer, name), name
    # the structs as the header lays them out
    assert C.sizeof(_lib.OutlierCfg) == 16 and C.sizeof(_lib.OutlierStats) == 64
    assert [f[0] for f in _lib.OutlierCfg._fields_] == ["k", "max_dist", "min_pts", "std_mul"]
    assert [f[0] for f in _lib.OutlierStats._fields_] == ["n", "n_stat", "mu", "sigma", "threshold", "few", "far", "outliers"]


def test_the_calls_reject_a_null_context_and_leave_their_outputs():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k = _lib.outlier_cfg()
    mask = np.full(4, 7, np.uint8)
    st = _lib.OutlierStats(n=9, mu=3.0)
    removed = C.c_size_t(5)
    assert L.flimo_map_outliers(None, 0, 0, C.byref(k), mask.ctypes.data, None, None, C.byref(st)) == ERR_INVALID
    assert L.flimo_map_remove_outliers(None, 0, 0, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert L.flimo_set_outlier_chunk(None, 5) == ERR_INVALID
    assert H.flimo_loc_map_outliers(None, 0, 0, C.byref(k), mask.ctypes.data, None, None, C.byref(st)) == ERR_INVALID
    assert H.flimo_loc_map_remove_outliers(None, 0, 0, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert np.all(mask == 7) and st.n == 9 and st.mu == 3.0 and removed.value == 5


def test_slot_tree_is_the_pairwise_tree_and_stays_within_the_bound_of_fsum():
    v = np.zeros((3, oc.SLOTS))
    v[0, :4] = [1.0, 2.0 ** -53, 2.0 ** -53, 1.0]            # ((1 + e) + (e + 1)): both halves round to 1; left to right gives 2 + 2e
    v[1, :] = np.arange(64)
    v[2, 5] = 0.3
    s = oc.slot_tree(v)
    assert s[0] == 2.0 and s[1] == 2016.0 and s[2] == 0.3
    # zeros in the upper slots change nothing: a list of 16 in a tree of 64 is the tree of 16
    rs = np.random.RandomState(0)
    w = np.zeros((200, oc.SLOTS))
    w[:, :16] = rs.uniform(0, 3, (200, 16))
    t16 = w[:, :16]
    while t16.shape[1] > 1:
        t16 = t16[:, 0::2] + t16[:, 1::2]
    assert np.array_equal(oc.slot_tree(w), t16[:, 0])
    # a tree-shaped sum of N non-negative terms against fsum, N as in the scene
    x = rs.uniform(0, 2, 8192)
    tree = x.copy()
    while len(tree) > 1:
        tree = tree[0::2] + tree[1::2]
    exact = math.fsum(x)
    assert abs(tree[0] - exact) <= oc.bound(len(x)) * exact
    assert abs(float(np.cumsum(x)[-1]) - exact) <= oc.bound(len(x)) * exact


def test_the_scene_holds_the_cases_of_the_self_rule():
    pts = oc.scene()
    assert len(pts) == oc.N_SCENE > 256 * 32                   # more than one tile of the ordered compaction
    # five copies of four points, two of forty
    _, cnts = np.unique(pts.view(np.dtype((np.void, 12))).reshape(-1), return_counts=True)
    assert np.sum(cnts == 5) == 4 and np.sum(cnts == 2) == 40 and np.sum(cnts == 1) == len(cnts) - 44
    for k, want in ((3, 4), (1, 12), (8, 0)):
        m, c, selfless = oc.cached_means("scene", k, INF)
        assert int(selfless.sum()) == want, (k, int(selfless.sum()))
        assert np.all(c == k)                                   # ungated: every list is full, one slot dropped
        assert np.all(m[selfless] == 0.0)                       # all neighbours of such a point are its duplicates
    for k, gate in ((16, 1.0), (63, 2.0), (3, 0.3)):
        m, c, _ = oc.cached_means("scene", k, gate)
        lonely = int((c == 0).sum())
        assert 70 <= lonely <= 2685, (k, gate, lonely)
        assert np.all(np.isnan(m[c == 0])) and not np.any(np.isnan(m[c > 0]))


def test_a_gate_of_zero_admits_not_even_the_point_itself():
    pts = oc.scene()[:500]
    m, c, selfless = oc.mean_dists(pts, 0, 500, 4, 0.0)
    assert np.all(c == 0) and np.all(np.isnan(m)) and not selfless.any()
    st = oc.statistics(m, c, 1, INF)
    assert st["n_stat"] == 0 and math.isnan(st["mu"]) and st["few"] == 500 and st["far"] == 0 and st["mask"].all()


@pytest.mark.parametrize("cfg", oc.CONFIGS, ids=lambda c: "k%d-g%s-m%d-s%g" % (c["k"], c["max_dist"], c["min_pts"], c["std_mul"]))
@pytest.mark.parametrize("which", ["scene", "far"])
def test_no_mean_distance_lies_at_the_threshold(which, cfg):
    """The condition under which a threshold within the bound gives the yardstick's mask bit for bit -- for every configuration and
    range the GPU tests run."""
    ranges = [(0, None)] if which == "far" else [(0, None), (8000, 300), (8191, 3)]
    for first, n in ranges:
        m, c, st = oc.yardstick(which, first, n, **cfg)
        if st["n_stat"] == 0:
            continue
        assert oc.rel_gap(m, st) > oc.GAP, (which, first, n, cfg, oc.rel_gap(m, st))
        assert oc.bound(st["n_stat"]) < oc.GAP / 100
        assert st["outliers"] == st["few"] + st["far"] == int(st["mask"].sum())
    if which == "far" and math.isinf(cfg["max_dist"]):
        m, c, st = oc.yardstick(which, **cfg)
        if cfg["std_mul"] == 1.0 and cfg["k"] >= 3:
            assert np.array_equal(np.where(st["mask"])[0], oc.N_SCENE + np.arange(3)), cfg


def test_the_pure_forms_are_the_standard_filters():
    """std_mul = INFINITY: the radius filter -- fewer than min_pts neighbours inside the gate; min_pts = 0, no gate: the statistical one."""
    pts = oc.scene()
    k, r, need = 16, 1.0, 5
    m, c, st = oc.yardstick("scene", k=k, max_dist=r, min_pts=need, std_mul=INF)
    cnt = oc.radius_counts(pts, r) - 1
    small = cnt <= k
    assert small.sum() > 1000 and (~small).sum() > 1000
    assert np.array_equal(c[small], cnt[small]) and np.all(c[~small] == k)
    assert np.array_equal(st["mask"], cnt < need) and st["far"] == 0 and 100 < st["few"] < 8000
    m, c, st = oc.yardstick("scene", k=8, max_dist=INF, min_pts=0, std_mul=1.0)
    assert st["few"] == 0 and st["n_stat"] == oc.N_SCENE
    mu, sd = m.mean(), m.std(ddof=1)
    assert abs(st["mu"] - mu) <= 1e-12 * mu and abs(st["sigma"] - sd) <= 1e-10 * sd
    assert np.array_equal(st["mask"], m > st["threshold"])
    assert st["mask"][8000:8300].mean() > 0.8 and st["mask"][:8000].mean() < 0.05      # the specks go, the surfaces stay
