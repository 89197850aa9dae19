"""Euclidean clusters of the stored points (flimo_map_clusters) as far as they can be checked without a GPU: both libraries export and
declare the new entry points, the calls reject a null context, the restatement of the definition (tests/clusters_common.py: dense
float32 predicate, plain union-find) equals a second form (breadth-first search over the dense matrix) and -- where scipy imports --
scipy's connected components, the cases worked by hand come out as the hand says, api.cluster_lists has PCL's shape, and every
scene-level property the GPU tests assert holds for the restatement first.  The kernels run on the GPU: tests/test_gpu_clusters.py."""
import ctypes as C
import os

import numpy as np
import pytest

import clusters_common as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
F = np.float32

HIP_NAMES = ("flimo_map_clusters", "flimo_map_remove_clusters", "flimo_set_cluster_chunk")
HOST_NAMES = ("flimo_loc_map_clusters", "flimo_loc_map_remove_clusters")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in HIP_NAMES:
        getattr(L, name)
    for name in HOST_NAMES:
        getattr(H, name)
    api.cluster_lists


def test_new_entry_points_are_exported_and_declared():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    dev = open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in HIP_NAMES:
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS, name
    assert "int flimo_map_clusters(flimo_ctx* ctx, size_t first, size_t n, const flimo_cluster_cfg* cfg, int32_t* label, int32_t* size," in pub
    assert "int flimo_map_remove_clusters(flimo_ctx* ctx, size_t first, size_t n, const flimo_cluster_cfg* cfg, size_t* removed," in pub
    assert "} flimo_cluster_cfg;" in pub and "} flimo_cluster_stats;" in pub and "tests/clusters_common.py" in pub
    assert "flimo_set_cluster_chunk(" in dev
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for name in ("map_clusters", "map_remove_clusters", "set_cluster_chunk"):
        assert hasattr(_lib.HipCtx, name), name
    assert hasattr(api.Localizer, "map_clusters") and hasattr(api.Localizer, "map_remove_clusters")
    # the structs as the header lays them out, and the wrapper's defaults as the restatement's
    assert C.sizeof(_lib.ClusterCfg) == 12 and C.sizeof(_lib.ClusterStats) == 40
    assert [f[0] for f in _lib.ClusterCfg._fields_] == ["tol", "min_size", "max_size"]
    assert [f[0] for f in _lib.ClusterStats._fields_] == ["n", "clusters", "largest", "sel_clusters", "sel_points"]
    k = _lib.cluster_cfg()
    for name, v in cc.DEFAULTS.items():
        assert float(getattr(k, name)) == float(F(v)), name
    k = _lib.cluster_cfg(tol=0.3, max_size=9)
    assert (k.tol, k.min_size, k.max_size) == (float(F(0.3)), 1, 9)


def test_the_calls_reject_a_null_context_and_leave_their_outputs():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k = _lib.cluster_cfg()
    label, size, mask = np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.uint8)
    st = _lib.ClusterStats(n=9, clusters=9, largest=9, sel_clusters=9, sel_points=9)
    removed = C.c_size_t(7)
    args = (0, 2, C.byref(k), label.ctypes.data, size.ctypes.data, mask.ctypes.data, C.byref(st))
    assert L.flimo_map_clusters(None, *args) == ERR_INVALID
    assert H.flimo_loc_map_clusters(None, *args) == ERR_INVALID
    assert L.flimo_map_remove_clusters(None, 0, 2, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert H.flimo_loc_map_remove_clusters(None, 0, 2, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert L.flimo_set_cluster_chunk(None, 5) == ERR_INVALID
    assert np.all(label == 7) and np.all(size == 7) and np.all(mask == 7) and removed.value == 7
    assert st.as_dict() == dict(n=9, clusters=9, largest=9, sel_clusters=9, sel_points=9)


# ---- the restatement against a second and a third form -------------------------------------------------------------------------------
def _small_cases():
    return {"first-1500-of-the-scene": (cc.scene()[:1500], 0.13), "lattice": (cc.lattice(8, 8, 8), 1.0), "duplicates": (cc.duplicates(), 0.5),
            "chains-2x400": (cc.chains(n=400)[0], 0.25), "sparse": (cc.sparse(), 20.0), "n65": (cc.small(65), 0.5)}


def test_the_restatement_equals_breadth_first_search_over_the_dense_matrix():
    for name, (pts, tol) in _small_cases().items():
        a, b = cc.labels(pts, tol), cc.labels_bfs(pts, tol)
        np.testing.assert_array_equal(a, b, err_msg=name)
        print(name, "points", len(pts), "clusters", len(np.unique(a)))
        assert np.all(a <= np.arange(len(pts))) and np.all(a[a] == a), name          # a label is a member, and its own label


def test_the_restatement_equals_scipys_connected_components():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, (pts, tol) in dict(_small_cases(), scene=(cc.scene(), 0.105)).items():
        I, J = cc.edges(pts, tol)
        n = len(pts)
        k, comp = connected_components(sp.coo_matrix((np.ones(len(I), np.int8), (I, J)), shape=(n, n)), directed=False)
        first = np.full(k, n, np.int64)
        np.minimum.at(first, comp, np.arange(n))                                     # the smallest index of each component
        np.testing.assert_array_equal(cc.components(n, I, J), first[comp], err_msg=name)


# ---- cases worked by hand ------------------------------------------------------------------------------------------------------------
def test_the_threshold_is_strict_and_one_float32_step_decides():
    far, near = cc.pair_at(0.5), cc.pair_at(cc.below(0.5))
    assert cc.sqdist_block(far, 0, 1)[0, 3] == F(0.25) == F(0.5) * F(0.5)            # exactly tol^2: no edge
    assert cc.sqdist_block(near, 0, 1)[0, 3] < F(0.25)
    r = cc.restate(far, tol=0.5)
    assert r["label"].tolist() == [0, 0, 0, 3, 3, 3] and r["size"].tolist() == [3] * 6 and r["stats"]["clusters"] == 2
    r = cc.restate(near, tol=0.5)
    assert r["label"].tolist() == [0] * 6 and r["size"].tolist() == [6] * 6 and r["stats"] == dict(n=6, clusters=1, largest=6, sel_clusters=1, sel_points=6)
    L = cc.lattice()
    r = cc.restate(L, tol=1.0)
    assert r["stats"]["clusters"] == len(L) == 2048 and r["stats"]["largest"] == 1
    np.testing.assert_array_equal(r["label"], np.arange(len(L)))
    r = cc.restate(L, tol=float(np.nextafter(F(1), F(2))))
    assert r["stats"]["clusters"] == 1 and r["stats"]["largest"] == 2048 and not r["label"].any()


def test_duplicates_are_apart_at_tol_zero_and_together_above():
    pts = cc.duplicates()
    r = cc.restate(pts, tol=0.0)
    assert r["stats"] == dict(n=700, clusters=700, largest=1, sel_clusters=700, sel_points=700)
    np.testing.assert_array_equal(r["label"], np.arange(700))
    r = cc.restate(pts, tol=1e-3)
    assert np.all(r["label"][200:500] == 200) and np.all(r["size"][200:500] == 300) and r["stats"]["clusters"] == 401
    assert np.all(np.delete(r["size"], np.arange(200, 500)) == 1)
    r = cc.restate(pts, tol=0.5)
    assert r["stats"]["largest"] >= 300 and len(np.unique(r["label"][200:500])) == 1


def test_both_readings_of_max_size():
    pts = F([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [5, 0, 0], [5.1, 0, 0], [9, 9, 9]])        # sizes 3, 2, 1
    r = cc.restate(pts, tol=0.15, min_size=1, max_size=0)                                      # 0: no upper bound
    assert r["size"].tolist() == [3, 3, 3, 2, 2, 1] and r["label"].tolist() == [0, 0, 0, 3, 3, 5] and r["mask"].all()
    assert r["stats"] == dict(n=6, clusters=3, largest=3, sel_clusters=3, sel_points=6)
    r = cc.restate(pts, tol=0.15, min_size=2, max_size=0)
    assert r["mask"].tolist() == [True] * 5 + [False] and r["stats"]["sel_clusters"] == 2
    r = cc.restate(pts, tol=0.15, min_size=1, max_size=2)                                      # debris below 3
    assert r["mask"].tolist() == [False] * 3 + [True] * 3 and r["stats"]["sel_clusters"] == 2 and r["stats"]["sel_points"] == 3
    r = cc.restate(pts, tol=0.15, min_size=2, max_size=2)
    assert r["mask"].tolist() == [False, False, False, True, True, False]
    r = cc.restate(pts, tol=0.15, min_size=0, max_size=0)
    assert r["mask"].all()
    r = cc.restate(pts, first=2, n=3, tol=0.15, min_size=3, max_size=3)                        # a range: the whole map's components
    assert r["label"].tolist() == [0, 3, 3] and r["size"].tolist() == [3, 2, 2] and r["mask"].tolist() == [True, False, False]
    assert r["stats"] == dict(n=3, clusters=3, largest=3, sel_clusters=1, sel_points=1)
    r = cc.restate(pts, first=6, n=0, tol=0.15)
    assert len(r["label"]) == 0 and r["stats"] == dict(n=0, clusters=3, largest=3, sel_clusters=3, sel_points=0)


def test_cluster_lists_has_pcls_shape():
    from fast_limo_amd import api
    label = np.array([0, 1, 0, 3, 1, 0, 6, 3, 8], np.int32)                                    # counts: 0 -> 3, 1 -> 2, 3 -> 2, 6 -> 1, 8 -> 1
    got = api.cluster_lists(label)
    assert [g.tolist() for g in got] == [[0, 2, 5], [1, 4], [3, 7], [6], [8]]                  # by size descending, then by label
    assert all(g.dtype == np.int64 for g in got)
    assert [g.tolist() for g in api.cluster_lists(label, min_size=2)] == [[0, 2, 5], [1, 4], [3, 7]]
    assert [g.tolist() for g in api.cluster_lists(label, min_size=1, max_size=2)] == [[1, 4], [3, 7], [6], [8]]
    assert [g.tolist() for g in api.cluster_lists(label, min_size=2, max_size=2)] == [[1, 4], [3, 7]]
    assert api.cluster_lists(np.zeros(0, np.int32)) == [] and api.cluster_lists(label, min_size=4) == []
    with pytest.raises(ValueError):
        api.cluster_lists(label, min_size=3, max_size=2)
    # on a scene: a partition of the points, every list one label, the sizes the restatement's
    r = cc.restate(cc.scene(), tol=0.105)
    lists = api.cluster_lists(r["label"])
    assert len(lists) == r["stats"]["clusters"] and len(lists[0]) == r["stats"]["largest"]
    assert np.array_equal(np.sort(np.concatenate(lists)), np.arange(len(r["label"])))
    for g in lists[:50]:
        assert len(np.unique(r["label"][g])) == 1 and r["label"][g[0]] == g[0] and np.all(np.diff(g) > 0) and np.all(r["size"][g] == len(g))
    assert [len(g) for g in lists] == sorted((len(g) for g in lists), reverse=True)


# ---- what the GPU tests assert about their scenes, on the restatement first ----------------------------------------------------------
def test_the_scenes_have_the_properties_the_gpu_tests_rely_on():
    pts = cc.scene()
    assert 4000 <= len(pts) <= 8000
    seen = []
    for tol in cc.SCENE_TOLS:
        s = cc.restate(pts, tol=tol)["stats"]
        print("scene tol", tol, s)
        seen.append((s["clusters"], s["largest"]))
    assert seen[0][0] > 4000 and 100 < seen[1][0] < 1000 and seen[2][0] < 20          # three different regimes
    assert seen[0][1] < 100 and seen[2][1] >= 5060
    pts, which = cc.chains()                                                           # the chain: one cluster each, labels 0 and 1
    assert len(pts) == 10000 and which[0] == 0 and which[1] == 1
    r = cc.restate(pts, tol=0.25)
    assert r["stats"] == dict(n=10000, clusters=2, largest=5000, sel_clusters=2, sel_points=10000)
    np.testing.assert_array_equal(r["label"], which)
    s = cc.restate(cc.sparse(), tol=20.0)["stats"]
    assert 300 == s["n"] and 10 < s["clusters"] < 60 and s["largest"] >= 10            # several clusters, not one, and groups that join
    for n in (1, 2, 63, 64, 65, 255, 256, 257):
        s = cc.restate(cc.small(n), tol=0.5)["stats"]
        assert s["n"] == n and (n < 3 or 1 < s["clusters"] < n), (n, s)                # edges and isolated points both occur


def test_after_a_carve_no_size_separates_the_residue_from_this_structure():
    """The scene of tests/test_gpu_carve.py's departed object (carve_common.standard_scene): 8 000 points of a box world, 400 of a
    ghost, one sweep.  The carve (restated: carve_common.yardstick) takes 316 ghost points and leaves 84, the ones within 0.45 m of
    the floor.  The box world is a sparse random sample (about 0.65 m between points).  At every tol at which its floor holds
    together the residue hangs on it, and below that the structure itself is in pieces no larger than the residue's.  So there is
    NO tol and m on this scene for which "components of fewer than m points" is the residue and nothing of the structure; the
    figures, by the restatement alone:
        tol 0.2: 64 of the 84 residue points share a component with structure points; the largest component of all has 34 points
        tol 0.4, tol 1.2: all 84 share a component with structure points
    The GPU test on this scene (tests/test_gpu_clusters.py) therefore asserts what the definition gives, without a tolerance, at
    CARVE_TOL = 0.2 and M_CARVE = 8 (min_size = 1, max_size = 7): 31 residue points and 7 810 structure points are selected."""
    kept, ghost = cc.carve_residue_scene()
    assert len(kept) == 8084 and ghost.sum() == 84
    for tol, want in ((0.2, 64), (0.4, 84), (1.2, 84)):
        lab = cc.labels(kept, tol)
        shared = np.isin(lab[ghost], np.intersect1d(lab[ghost], lab[~ghost])).sum()
        print("tol", tol, "residue points sharing a component with the structure", shared)
        assert shared == want
    r = cc.restate(kept, tol=cc.CARVE_TOL, min_size=1, max_size=cc.M_CARVE - 1)
    assert (cc.CARVE_TOL, cc.M_CARVE) == (0.2, 8) and r["stats"]["largest"] == 34
    assert r["mask"][ghost].sum() == 31 and r["mask"][~ghost].sum() == 7810
