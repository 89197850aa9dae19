"""Smooth-surface regions of the stored points (flimo_map_regions, flimo_map_region_list, flimo_map_remove_regions) as far as they
can be checked without a GPU: both libraries export and declare the new entry points, the structs are laid out as the header says,
the calls reject a null context, flimo_region_joined_host -- the predicates the link kernel calls -- equals the numpy predicate
(tests/regions_common.py) on random pairs, one float32 step either side of every threshold, on NaN and infinite normals and at
min_cos 0 / max_curv INFINITY, the union-find equals a breadth-first search, api.region_planes is right on hand covariances, and
every scene-level property the GPU tests assert holds on the restatement fed with numpy normals.  The kernels run on the GPU:
tests/test_gpu_regions.py."""
import ctypes as C
import os

import numpy as np
import pytest

import clusters_common as cc
import regions_common as rc
import voxels_common as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
F = np.float32
D = np.float64
INF = float("inf")

HIP_NAMES = ("flimo_map_regions", "flimo_map_region_list", "flimo_map_remove_regions", "flimo_region_joined_host", "flimo_set_region_chunk")
HOST_NAMES = ("flimo_loc_map_regions", "flimo_loc_map_region_list", "flimo_loc_map_remove_regions")


def test_new_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    dev = open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in HIP_NAMES:
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS, name
    assert "int flimo_map_regions(flimo_ctx* ctx, size_t first, size_t n, const flimo_region_cfg* cfg, int32_t* label, int32_t* size," in pub
    assert "int flimo_map_region_list(flimo_ctx* ctx, const flimo_region_cfg* cfg, size_t cap, size_t* nr, int32_t* label" in pub
    assert "int flimo_map_remove_regions(flimo_ctx* ctx, size_t first, size_t n, const flimo_region_cfg* cfg, size_t* removed," in pub
    assert "int flimo_region_joined_host(const float pi[3], const float ni[4], const float pj[3], const float nj[4], const flimo_region_cfg* cfg," in pub
    assert "} flimo_region_cfg;" in pub and "} flimo_region_stats;" in pub and "tests/regions_common.py" in pub
    assert "flimo_set_region_chunk(" in dev
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for name in ("map_regions", "map_region_list", "map_remove_regions", "set_region_chunk"):
        assert hasattr(_lib.HipCtx, name), name
    for name in ("map_regions", "map_region_list", "map_remove_regions"):
        assert hasattr(api.Localizer, name), name
    api.region_planes, api.region_joined_host
    # the structs as the header lays them out, and the wrapper's defaults as the restatement's
    assert C.sizeof(_lib.RegionCfg) == 36 and C.sizeof(_lib.RegionStats) == 56
    assert [f[0] for f in _lib.RegionCfg._fields_] == ["tol", "normal_k", "normal_max_dist", "normal_min_pts", "min_cos", "max_curv", "border",
                                                      "min_size", "max_size"]
    assert [f[1] for f in _lib.RegionCfg._fields_] == [C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    assert [f[0] for f in _lib.RegionStats._fields_] == list(rc.STATS)
    assert all(f[1] is C.c_uint64 for f in _lib.RegionStats._fields_)
    k = _lib.region_cfg()
    for name, _ in _lib.RegionCfg._fields_:
        want = rc.DEFAULTS[name]
        assert getattr(k, name) == (float(F(want)) if isinstance(want, float) else want), name
    k = _lib.region_cfg(tol=0.3, border=0)
    assert (k.tol, k.border, k.normal_k) == (float(F(0.3)), 0, 16)
    # the order of the fields in the header
    body = pub[pub.index("typedef struct flimo_region_cfg {"):pub.index("} flimo_region_cfg;")]
    at = [body.index(" %s;" % name) for name, _ in _lib.RegionCfg._fields_]
    assert at == sorted(at)
    body = pub[pub.index("typedef struct flimo_region_stats {"):pub.index("} flimo_region_stats;")]
    at = [body.index(" %s;" % name) for name in rc.STATS]
    assert at == sorted(at)


def test_the_calls_reject_a_null_context_and_leave_their_outputs(built):
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k = _lib.region_cfg()
    nr, removed, st = C.c_size_t(7), C.c_size_t(7), _lib.RegionStats(7, 7, 7, 7, 7, 7, 7)
    i1, d3, d6, mask = np.full(2, 7, np.int32), np.full(6, 7.0), np.full(12, 7.0), np.full(2, 7, np.uint8)
    for lib, pre in ((L, "flimo_"), (H, "flimo_loc_")):
        assert getattr(lib, pre + "map_regions")(None, 0, 2, C.byref(k), i1.ctypes.data, i1.ctypes.data, mask.ctypes.data, C.byref(st)) == ERR_INVALID
        assert getattr(lib, pre + "map_region_list")(None, C.byref(k), 2, C.byref(nr), i1.ctypes.data, i1.ctypes.data, i1.ctypes.data, d3.ctypes.data,
                                                     d6.ctypes.data, C.byref(st)) == ERR_INVALID
        assert getattr(lib, pre + "map_remove_regions")(None, 0, 2, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert L.flimo_set_region_chunk(None, 1) == ERR_INVALID
    assert np.all(i1 == 7) and np.all(d3 == 7) and np.all(d6 == 7) and np.all(mask == 7)
    assert nr.value == 7 and removed.value == 7 and st.as_dict() == dict.fromkeys(rc.STATS, 7)


# ---- flimo_region_joined_host against the numpy predicate -------------------------------------------------------------------------------
def _host(pi, ni, pj, nj, **cfg):
    from fast_limo_amd import api
    return api.region_joined_host(pi, ni, pj, nj, **cfg)


def _both(pi, ni, pj, nj, tol, min_cos, max_curv, what=""):
    """The host function and the restatement agree, and the predicate is symmetric; returns (smooth_i, smooth_j, joined)."""
    got = _host(pi, ni, pj, nj, tol=tol, min_cos=min_cos, max_curv=max_curv)
    assert got == rc.joined_pair(pi, ni, pj, nj, tol, min_cos, max_curv), (what, pi, ni, pj, nj, tol, min_cos, max_curv, got)
    back = _host(pj, nj, pi, ni, tol=tol, min_cos=min_cos, max_curv=max_curv)
    assert back == (got[1], got[0], got[2]), (what, got, back)
    return got


def _unit(rs, n):
    v = rs.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def test_random_pairs_and_symmetry(built):
    rs = np.random.RandomState(3)
    n = 1500
    pi, pj = rs.uniform(-5, 5, (n, 3)).astype(F), None
    pj = (pi + rs.uniform(-0.4, 0.4, (n, 3))).astype(F)
    ni = np.concatenate([_unit(rs, n), rs.uniform(0, 0.1, (n, 1)).astype(F)], 1)
    nj = np.concatenate([_unit(rs, n), rs.uniform(0, 0.1, (n, 1)).astype(F)], 1)
    nj[::3, :3] = ni[::3, :3] * F(-1) ** np.arange(len(ni[::3]))[:, None]      # parallel and antiparallel normals
    seen = set()
    for t in range(n):
        seen.add(_both(pi[t], ni[t], pj[t], nj[t], 0.5, rc.COS20, 0.05, "random"))
    assert len(seen) == 8, seen                            # every combination of the three answers occurs


def test_each_threshold_one_float32_step_either_side(built):
    flat = F([0.0, 0.0, 1.0, 0.0])
    origin = F([1.0, 2.0, 3.0])
    for d in (0.5, 0.15, 0.3, 1.0, 0.123):
        d = F(d)
        pj = origin + F([d, 0.0, 0.0])
        d = F(pj[0] - origin[0])                           # (the difference the predicate forms)
        r2 = d * d
        for tol, want in ((d, False), (rc.up(d), True), (rc.down(d), False)):
            assert (F(tol) * F(tol) > r2) == want
            assert _both(origin, flat, pj, flat, tol, 1.0, 0.05, "tol")[2] == want, (d, tol)
    for deg in (20.0, 12.0, 45.0, 89.0, 1.0):
        c, s = F(np.cos(np.radians(deg))), F(np.sin(np.radians(deg)))
        ni, nj = F([1.0, 0.0, 0.0, 0.0]), F([c, s, 0.0, 0.0])      # the dot product is c itself
        for sign in (1.0, -1.0):
            njs = nj * F([sign, sign, sign, 1.0])
            assert _both(origin, ni, origin, njs, 0.5, c, 0.05, "min_cos")[2] is True
            assert _both(origin, ni, origin, njs, 0.5, rc.up(c), 0.05, "min_cos")[2] is False
            assert _both(origin, ni, origin, njs, 0.5, rc.down(c), 0.05, "min_cos")[2] is True
    for v in (0.05, 0.02, 0.0, 0.3333):
        n4 = F([0.0, 1.0, 0.0, v])
        assert _both(origin, n4, origin, flat, 0.5, 0.0, F(v), "max_curv")[0] is True
        assert _both(origin, n4, origin, flat, 0.5, 0.0, rc.up(v), "max_curv")[0] is True
        if v > 0:
            assert _both(origin, n4, origin, flat, 0.5, 0.0, rc.down(v), "max_curv")[0] is False


def test_nan_and_infinite_normals_zero_min_cos_and_infinite_max_curv(built):
    p, q = F([0.0, 0.0, 0.0]), F([0.1, 0.0, 0.0])
    good = F([0.0, 0.0, 1.0, 0.01])
    for bad in (F([np.nan, 0, 1, 0.01]), F([0, np.nan, 1, 0.01]), F([0, 0, np.nan, 0.01]), F([0, 0, 1, np.nan]), F([np.nan] * 4),
                F([np.inf, 0, 0, 0.01]), F([0, 0, 1, np.inf]), F([0, -np.inf, 0, 0.01])):
        for min_cos, max_curv in ((rc.COS20, 0.05), (0.0, INF)):
            assert _both(p, bad, q, good, 0.5, min_cos, max_curv, "bad normal") == (False, True, False)
    # min_cos 0 admits perpendicular normals; max_curv INFINITY admits every finite curvature
    across = F([1.0, 0.0, 0.0, 0.9])
    assert _both(p, across, q, good, 0.5, 0.0, INF, "open") == (True, True, True)
    assert _both(p, across, q, good, 0.5, 0.0, 0.05, "open") == (False, True, True)
    assert _both(p, across, q, good, 0.5, 1e-6, INF, "open") == (True, True, False)
    assert _both(p, good, q, good, 0.0, 0.0, INF, "tol 0") == (True, True, False)      # tol 0: d < 0 holds for no pair
    assert _both(p, good, p, good, 0.0, 0.0, INF, "tol 0, one place") == (True, True, False)


def test_the_host_function_rejects_what_the_calls_reject(built):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    p, n4 = F([0, 0, 0]), F([0, 0, 1, 0])
    out = [C.c_int(7), C.c_int(7), C.c_int(7)]
    refs = [C.byref(o) for o in out]
    for kw in (dict(tol=np.nan), dict(tol=-1.0), dict(tol=INF), dict(min_cos=np.nan), dict(min_cos=-0.1), dict(min_cos=1.5), dict(max_curv=np.nan),
               dict(max_curv=-0.01)):
        k = _lib.region_cfg(**kw)
        assert L.flimo_region_joined_host(p.ctypes.data, n4.ctypes.data, p.ctypes.data, n4.ctypes.data, C.byref(k), *refs) == ERR_INVALID, kw
    k = _lib.region_cfg()
    assert L.flimo_region_joined_host(None, n4.ctypes.data, p.ctypes.data, n4.ctypes.data, C.byref(k), *refs) == ERR_INVALID
    assert L.flimo_region_joined_host(p.ctypes.data, n4.ctypes.data, p.ctypes.data, n4.ctypes.data, None, *refs) == ERR_INVALID
    assert [o.value for o in out] == [7, 7, 7]
    assert L.flimo_region_joined_host(p.ctypes.data, n4.ctypes.data, p.ctypes.data, n4.ctypes.data, C.byref(k), None, None, None) == 0


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_scene():
    """The standard scene with numpy normals at both neighbourhood sizes, and the labels of the three settings, computed once."""
    pts = rc.scene()
    nrm = {k: rc.cpu_normals(pts, k) for k in (16, 10)}
    labels = [rc.labels(pts, nrm[s["normal_k"]], **rc.cfg_of(**s)) for s in rc.SETTINGS]
    return dict(pts=pts, nrm=nrm, labels=labels)


def test_union_find_equals_breadth_first_search(cpu_scene):
    pts = cpu_scene["pts"]
    s = rc.SETTINGS[0]
    np.testing.assert_array_equal(cpu_scene["labels"][0], rc.labels_bfs(pts, cpu_scene["nrm"][16], s["tol"], s["min_cos"], s["max_curv"]))
    rs = np.random.RandomState(5)
    for n in (1, 2, 3, 64, 257):
        p = cc.small(n)
        nrm = np.concatenate([_unit(rs, n), rs.uniform(0, 0.08, (n, 1)).astype(F)], 1)
        nrm[rs.rand(n) < 0.1] = np.nan
        for tol, min_cos, max_curv in ((0.5, 0.5, 0.05), (0.5, 0.0, INF), (0.0, 0.0, INF), (2.0, 0.9, 0.02)):
            a = rc.labels(p, nrm, tol=tol, min_cos=min_cos, max_curv=max_curv, border=0)
            np.testing.assert_array_equal(a, rc.labels_bfs(p, nrm, tol, min_cos, max_curv))
            sm = rc.smooth(nrm, max_curv)
            assert np.all(a[~sm] == -1) and np.all(a[sm] >= 0) and np.all(a[sm] <= np.flatnonzero(sm))
            if tol == 0.0:
                np.testing.assert_array_equal(a[sm], np.flatnonzero(sm))


def test_the_scene_is_recovered_on_the_restatement(cpu_scene):
    """The issue's experiment: exactly four regions of at least 100 points, each entirely on one surface, 4 748 points in them and
    312 unassigned without the border; 1 842, 1 600, 1 244 and 298 points and 76 unassigned with it; one Euclidean cluster."""
    pts, surf = cpu_scene["pts"], rc.scene_surface()
    big, purity, inside = rc.recovery(cpu_scene["labels"][0], surf)
    sizes = sorted(int((cpu_scene["labels"][0] == r).sum()) for r in big)
    assert sizes == [235, 1145, 1570, 1798] and purity == [1.0] * 4 and inside == 4748
    fin = rc.finish(cpu_scene["labels"][0], cpu_scene["nrm"][16], 0.05)
    assert fin["stats"] == dict(n=5060, smooth=4748, regions=4, largest=1798, sel_regions=4, unassigned=312, sel_points=4748)
    lab = cpu_scene["labels"][1]
    big, purity, inside = rc.recovery(lab, surf)
    assert sorted(int((lab == r).sum()) for r in big) == [298, 1244, 1600, 1842] and int((lab < 0).sum()) == 76
    for r in big:                                          # at most 3 points of any region come from another surface
        assert (lab == r).sum() - np.bincount(surf[lab == r], minlength=3).max() <= 3
    # the border changes no label of a smooth point
    sm = rc.smooth(cpu_scene["nrm"][16], 0.05)
    np.testing.assert_array_equal(lab[sm], cpu_scene["labels"][0][sm])
    assert len(np.unique(cc.labels(pts, 0.15))) == 1
    big, purity, inside = rc.recovery(cpu_scene["labels"][2], surf)
    assert len(big) == 4 and min(purity) >= 0.99


def test_degenerate_settings_on_the_restatement(cpu_scene):
    pts, nrm = cpu_scene["pts"], cpu_scene["nrm"][16]
    lab = rc.labels(pts, nrm, tol=0.15, min_cos=0.0, max_curv=INF, border=0)
    np.testing.assert_array_equal(lab, cc.labels(pts, 0.15))              # every point has a normal here: the Euclidean clusters
    assert np.all(lab == 0)                                               # (the whole scene as one region)
    lab = rc.labels(pts, nrm, tol=0.0, min_cos=0.0, max_curv=0.05, border=1)
    sm = rc.smooth(nrm, 0.05)
    np.testing.assert_array_equal(lab, np.where(sm, np.arange(len(pts)), -1))
    fin = rc.finish(lab, nrm, 0.05, min_size=2)
    assert fin["stats"]["regions"] == fin["stats"]["smooth"] == int(sm.sum()) and fin["stats"]["sel_points"] == 0 and fin["stats"]["largest"] == 1


def test_the_tie_case_on_the_restatement(built):
    """numpy normals: the patches' curvature is exactly 0, the middle point's 0.0187 (k 9) and 0.0321 (k 16); its two nearest
    candidates are equally far, bit for bit, and the smaller index wins whichever patch comes first."""
    for k, curv in ((9, 0.0187), (16, 0.0321)):
        for swap in (False, True):
            pts = rc.tie_case(swap)
            nrm = rc.cpu_normals(pts, k)
            assert np.all(nrm[:128, 3] == 0.0) and abs(float(nrm[128, 3]) - curv) < 5e-4
            sm = rc.smooth(nrm, rc.TIE_CFG["max_curv"])
            assert sm[:128].all() and not sm[128] and rc.has_normal(nrm)[128]
            d = cc.sqdist_block(pts, 128, 129)[0]
            near = np.argsort((rc.bits32(d).astype(np.uint64) << np.uint64(32)) | np.arange(129, dtype=np.uint64))[:3]
            assert near[0] == 128 and rc.bits32(d)[near[1]] == rc.bits32(d)[near[2]] and near[1] < 64 <= near[2]
            lab = rc.labels(pts, nrm, **rc.cfg_of(**rc.TIE_CFG))
            assert lab[near[1]] == 0 and lab[near[2]] == 64 and lab[128] == 0
            assert (pts[0, 2] == 1.0) == swap              # label 0 is the lower patch, or the upper one after the swap
            fin = rc.finish(lab, nrm, rc.TIE_CFG["max_curv"])
            assert fin["size"][128] == 65 and fin["size"][64] == 64 and fin["stats"]["unassigned"] == 0
            assert rc.labels(pts, nrm, **rc.cfg_of(**dict(rc.TIE_CFG, border=0)))[128] == -1


def test_points_without_a_normal_are_unassigned_on_the_restatement(built):
    pts = rc.gated_scene()
    nrm = rc.cpu_normals(pts, 16, 0.5)
    lone = np.flatnonzero(~rc.has_normal(nrm))
    assert lone.tolist() == [2000, 2001, 5062, 5063, 5064]
    out = rc.restate(pts, nrm, tol=0.15, normal_max_dist=0.5, min_size=0)
    assert np.all(out["label"][lone] == -1) and np.all(out["size"][lone] == 0) and not out["mask"][lone].any()
    assert out["stats"]["unassigned"] >= 5 and out["stats"]["regions"] >= 4


def test_the_listing_on_the_restatement(cpu_scene):
    pts, which = rc.hand_regions()
    nrm = rc.cpu_normals(pts, 9)
    cfg = rc.cfg_of(tol=0.15, normal_k=9, min_cos=0.9, max_curv=0.01, border=1)
    lab = rc.labels(pts, nrm, **cfg)
    li = rc.listing(pts, lab, nrm, cfg["max_curv"])
    assert li["nr"] == 4 and sorted(li["count"].tolist()) == [63, 64, 65, 1025]
    for r in range(4):
        m = np.flatnonzero(lab == li["label"][r])
        assert len(np.unique(which[m])) == 1 and li["first"][r] == m[0] == li["label"][r] and li["count"][r] == len(m)
        x = pts[m].astype(D)
        cen = [vc.sum_shape_plain(x[:, a]) / float(len(m)) for a in range(3)]
        assert vc.bits(cen).tolist() == vc.bits(li["centroid"][r]).tolist()
        d = x - np.array(cen)
        cov = [vc.sum_shape_plain(d[:, a] * d[:, b]) / float(len(m)) for a in range(3) for b in range(a, 3)]
        assert vc.bits(cov).tolist() == vc.bits(li["cov"][r]).tolist()
    assert np.all(li["label"][1:] > li["label"][:-1])
    # the selection narrows the listing, not the regions
    few = rc.listing(pts, lab, nrm, cfg["max_curv"], min_size=64, max_size=65)
    assert few["nr"] == 2 and few["stats"]["regions"] == 4 and few["stats"]["sel_points"] == 129
    # the standard scene with the border: members of a region include its border points
    li = rc.listing(cpu_scene["pts"], cpu_scene["labels"][1], cpu_scene["nrm"][16], 0.05, min_size=100)
    assert sorted(li["count"].tolist()) == [298, 1244, 1600, 1842]


def test_region_planes_on_hand_covariances(built):
    from fast_limo_amd import api
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    full = lambda m: [m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]]
    cases = [(np.diag([2.0, 1.0, 0.25]), [1.0, 2.0, 3.0]),              # the plane z = 3, thick 0.5 rms
             (np.diag([0.0, 1.0, 2.0]), [-4.0, 0.0, 0.0]),                # the plane x = -4, exact
             (R @ np.diag([1e-4, 3.0, 2.0]) @ R.T, [1.0, 1.0, 0.0]),      # a plane whose normal is (c, s, 0)
             (-R @ np.diag([1e-4, 3.0, 2.0]) @ R.T * -1.0, [-1.0, -1.0, 5.0])]
    out = api.region_planes(dict(centroid=np.array([cn for _, cn in cases]), cov=np.array([full(m) for m, _ in cases])))
    np.testing.assert_allclose(out["normal"], [[0, 0, 1], [1, 0, 0], [c, s, 0], [c, s, 0]], atol=1e-12)
    np.testing.assert_allclose(out["d"], [-3.0, 4.0, -(c + s), c + s], atol=1e-12)
    np.testing.assert_allclose(out["eigenvalues"], [[0.25, 1, 2], [0, 1, 2], [1e-4, 2, 3], [1e-4, 2, 3]], atol=1e-12)
    np.testing.assert_allclose(out["rms"], [0.5, 0.0, 1e-2, 1e-2], atol=1e-12)
    big = np.argmax(np.abs(out["normal"]), axis=1)
    assert np.all(out["normal"][np.arange(4), big] > 0)                   # flimo_map_normals' sign rule
    empty = api.region_planes(dict(centroid=np.zeros((0, 3)), cov=np.zeros((0, 6))))
    assert empty["normal"].shape == (0, 3) and empty["d"].shape == (0,) and empty["rms"].shape == (0,)
