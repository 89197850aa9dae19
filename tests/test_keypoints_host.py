"""ISS keypoints of the stored points (flimo_map_keypoints) as far as they can be checked without a GPU: both libraries export and
declare the new entry points, the calls reject a null context, the numpy restatement of the definition (tests/keypoints_common.py)
equals a second form written as a loop over points and slots, the worked cases come out as the hand computation says, every
scene-level property the GPU tests assert holds for brute-force neighbourhoods first, and api.relocalize(keypoints=None) forwards
exactly what it forwarded before.  The kernels run on the GPU: tests/test_gpu_keypoints.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import fpfh_common as fc
import keypoints_common as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
F = np.float32
INF = float("inf")

HIP_NAMES = ("flimo_map_keypoints", "flimo_set_keypoints_chunk")
HOST_NAMES = ("flimo_loc_map_keypoints",)


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
    assert "int flimo_map_keypoints(flimo_ctx* ctx, size_t first, size_t n, const flimo_keypoint_cfg* cfg," in pub
    assert "} flimo_keypoint_cfg;" in pub and "tests/keypoints_common.py" in pub and "flimo_set_keypoints_chunk(" in dev
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for name in ("map_keypoints", "set_keypoints_chunk"):
        assert hasattr(_lib.HipCtx, name), name
    assert hasattr(api.Localizer, "map_keypoints")
    # the struct as the header lays it out, and the wrapper's defaults as the restatement's
    assert C.sizeof(_lib.KeypointCfg) == 28
    assert [f[0] for f in _lib.KeypointCfg._fields_] == ["k", "max_dist", "min_pts", "gamma21", "gamma32", "nms_k", "nms_max_dist"]
    k = _lib.keypoint_cfg()
    for name, v in kc.DEFAULTS.items():
        assert float(getattr(k, name)) == float(F(v)), name
    k = _lib.keypoint_cfg(k=12, nms_max_dist=0.5, gamma21=0.7)
    assert (k.k, k.nms_max_dist, k.gamma21, math.isinf(k.max_dist)) == (12, 0.5, float(F(0.7)), True)


def test_the_calls_reject_a_null_context_and_leave_their_outputs():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k = _lib.keypoint_cfg()
    mask, sal, cnt, count = np.full(2, 7, np.uint8), np.full(2, 7.0), np.full(2, 7, np.int32), C.c_size_t(7)
    args = (0, 2, C.byref(k), mask.ctypes.data, sal.ctypes.data, cnt.ctypes.data, C.byref(count))
    assert L.flimo_map_keypoints(None, *args) == ERR_INVALID
    assert H.flimo_loc_map_keypoints(None, *args) == ERR_INVALID
    assert L.flimo_set_keypoints_chunk(None, 5) == ERR_INVALID
    assert np.all(mask == 7) and np.all(sal == 7.0) and np.all(cnt == 7) and count.value == 7


# ---- the restatement against its slow form ----------------------------------------------------------------------------------------------
HOST_CASES = {
    "scene-first-600": (lambda: fc.scene()[:600], dict(k=16, nms_k=16)),
    "scene-first-600-gates": (lambda: fc.scene()[:600], dict(k=17, nms_k=5, max_dist=0.6, nms_max_dist=0.4, min_pts=8, gamma21=0.7, gamma32=0.5)),
    "corner-twice": (kc.corner_twice, dict(k=16, nms_k=16)),
    "cross": (kc.cross, dict(k=7, nms_k=7, gamma21=kc.above(0.25), gamma32=kc.above(0.25))),
    "lattice-patch": (kc.lattice_patch, dict(k=9, nms_k=9)),
}


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, (cloud, cfg) in HOST_CASES.items():
        inputs = kc.cpu_inputs(cloud(), cfg)
        out[name] = (inputs, cfg, kc.restate(*inputs, cfg))
    return out


def test_the_restatement_equals_the_loop_over_points(restated):
    for name, (inputs, cfg, r) in restated.items():
        slow = kc.restate_loop(*inputs, cfg)
        kc.same(r, slow, name)
        print(name, "points", len(r["mask"]), "salient", int((~np.isnan(r["saliency"])).sum()), "keypoints", r["count"])
    assert 0 < restated["scene-first-600"][2]["count"] < 600
    some = restated["scene-first-600-gates"][2]
    assert 0 < (~np.isnan(some["saliency"])).sum() < 600                     # the thresholds reject some points and keep others
    # a range is the slice of the whole
    inputs, cfg, r = restated["scene-first-600"]
    part = kc.restate(*inputs, cfg, first=100, n=70)
    kc.same(part, dict(saliency=r["saliency"][100:170], cnt=r["cnt"][100:170], mask=r["mask"][100:170], count=int(r["mask"][100:170].sum())), "range")


def test_a_keypoint_beats_its_list_and_a_suppressed_point_is_beaten(restated):
    """The definition read the other way round, from the outputs."""
    for name, ((eig, cnt, idx, ncnt), cfg, r) in restated.items():
        s = r["salient"]
        for j in range(len(s)):
            others = [int(t) for t in idx[j, :ncnt[j]] if t != j and not np.isnan(s[t])]
            better = [t for t in others if s[t] > s[j] or (s[t] == s[j] and t < j)]
            assert bool(r["mask"][j]) == (not np.isnan(s[j]) and not better), (name, j)


# ---- worked cases ---------------------------------------------------------------------------------------------------------------------
def test_a_neighbourhood_worked_by_hand():
    """The cross: a = 1, b = 1/2, c = 1/4.  Every point's list is all 7 points; about their centroid (the centre) the sums of squares
    are 2 a^2, 2 b^2, 2 c^2 and every mixed sum is 0: l2 = 2/7, l1 = l2 / 4, l0 = l1 / 4 exactly.  gamma = 1/4 fails the strict compare,
    the next float32 passes; all 7 then tie in saliency and the lowest index -- the centre -- is the one keypoint."""
    pts = kc.cross()
    cfg = dict(k=7, nms_k=7, gamma21=0.25, gamma32=0.25)
    eig, cnt, idx, ncnt = kc.cpu_inputs(pts, cfg)
    assert np.all(cnt == 7) and np.all(ncnt == 7)
    exact = np.float64(kc.CROSS_EIG)
    assert exact[1] == exact[2] / 4 and exact[0] == exact[1] / 4
    assert np.all(np.abs(eig - exact) <= 1e-15)                          # (numpy's eigenvalues; the device's are exact: tests/test_gpu_keypoints.py)
    eig = np.tile(exact, (7, 1))
    up = kc.above(0.25)
    assert up > 0.25 and F(up) == up
    for g21, g32, salient in ((0.25, 0.25, False), (up, 0.25, False), (0.25, up, False), (up, up, True), (1.0, 1.0, True)):
        r = kc.restate(eig, cnt, idx, ncnt, dict(cfg, gamma21=g21, gamma32=g32))
        assert (~np.isnan(r["saliency"])).all() == salient and (~np.isnan(r["saliency"])).any() == salient, (g21, g32)
        assert r["mask"].tolist() == [salient] + [False] * 6 and r["count"] == int(salient)
        if salient:
            assert np.all(r["saliency"] == exact[0])


def test_a_planar_lattice_patch_is_not_salient_at_any_gamma():
    pts = kc.lattice_patch()
    assert len(np.unique(pts[:, 2])) == 1
    for cfg in (dict(k=9, nms_k=9, gamma21=1.0, gamma32=1.0), dict(k=32, nms_k=4, gamma21=0.5, gamma32=1.0)):
        eig, cnt, idx, ncnt = kc.cpu_inputs(pts, cfg)
        assert np.all(np.abs(eig[:, 0]) <= 1e-15)
        eig[:, 0] = 0.0                                                   # (what the device gives exactly: every z-difference is 0)
        r = kc.restate(eig, cnt, idx, ncnt, cfg)
        assert np.isnan(r["saliency"]).all() and not r["mask"].any() and r["count"] == 0


def test_of_exact_duplicates_the_lower_index_survives():
    pts = kc.corner_twice()
    n = len(pts) // 2
    assert np.array_equal(pts[:n], pts[n:])
    cfg = dict(k=16, nms_k=16)
    eig, cnt, idx, ncnt = kc.cpu_inputs(pts, cfg)
    assert np.array_equal(idx[:n], idx[n:]) and eig[:n].tobytes() == eig[n:].tobytes()
    r = kc.restate(eig, cnt, idx, ncnt, cfg)
    s = r["saliency"]
    assert (~np.isnan(s[:n])).sum() > 100 and np.array_equal(s[:n], s[n:], equal_nan=True)      # saliency ties occur
    assert not r["mask"][n:].any() and 0 < r["count"] == int(r["mask"][:n].sum())
    # the survivors are the keypoints of the cluster stored once with half the neighbourhoods (each neighbour is listed twice)
    once = kc.cpu_keypoints(pts[:n], dict(k=8, nms_k=8))
    assert once["count"] > 0


def test_a_box_on_a_lattice_has_no_keypoint_inside_a_face():
    pts, ijk = kc.box()
    r = kc.cpu_keypoints(pts, kc.BOX_CFG)
    inside = kc.box_face_interior(ijk, kc.BOX_CFG["max_dist"])
    faces = ((ijk == 0) | (ijk == kc.BOX_SIDE)).sum(1)
    print("box: points", len(pts), "inside a face", int(inside.sum()), "salient", int((~np.isnan(r["saliency"])).sum()), "keypoints", r["count"],
          "by faces met", np.bincount(faces[r["mask"]], minlength=4).tolist())
    assert inside.sum() > 500 and np.isnan(r["saliency"][inside]).all() and not r["mask"][inside].any()
    assert r["count"] >= 12 and np.all(faces[r["mask"]] == 2)             # every keypoint lies on an edge, none at a corner
    assert np.isnan(r["saliency"][faces == 3]).all()                      # a corner's neighbourhood is symmetric: l1 == l2


def test_what_the_gpu_tests_claim_about_their_scenes():
    """Every count the GPU tests assert on top of the equality with the restatement, shown here with brute-force lists first."""
    pts = fc.scene()
    n = len(pts)
    lists = {nms: {g: kc.brute_knn(pts, pts, nms, g, chunk=256) for g in (INF, kc.SCENE_GATED["nms_max_dist"])} for nms in (2, 16, 17, 64)}
    for k in (16, 17, 64):
        seen = {}
        for tag, cfg in ((None, dict(k=k, min_pts=0)), (12, dict(kc.SCENE_GATED, k=k, min_pts=12)), (25, dict(kc.SCENE_GATED, k=k, min_pts=25))):
            c = kc.full(cfg)
            eig, cnt = kc.cpu_eig(pts, k, c["max_dist"], c["min_pts"])
            seen[tag] = []
            for nms in (2, 16, 17, 64):
                idx, _, ncnt = lists[nms][c["nms_max_dist"]]
                r = kc.restate(eig, cnt, idx, ncnt, dict(cfg, nms_k=nms))
                seen[tag].append((int((~np.isnan(r["saliency"])).sum()), r["count"]))
            assert cnt.min() >= 3 and (tag is not None or np.all(cnt == k))
        print("scene k", k, seen)
        assert kc.scene_counts_hold(k, seen[None], seen[12], seen[25], n), (k, seen)
    for k, nms_k in ((16, 17), (33, 9)):                                  # the configuration of the GPU test of chunks, ranges and cells
        r = kc.cpu_keypoints(pts, dict(k=k, nms_k=nms_k, max_dist=0.5, nms_max_dist=0.3, gamma21=0.9, gamma32=0.9), fast=True)
        assert 0 < r["count"] < (~np.isnan(r["saliency"])).sum() < n
    r = kc.cpu_keypoints(pts, dict(k=16, nms_k=16, nms_max_dist=0.0), fast=True)
    assert r["count"] == (~np.isnan(r["saliency"])).sum() > n // 2           # a suppression gate of 0: empty lists suppress nothing
    r = kc.cpu_keypoints(pts, dict(k=20, nms_k=12, max_dist=1.0, nms_max_dist=0.5, gamma21=0.9), fast=True)
    assert 0 < r["count"] < n
    # the two clusters 300 m apart: a list of 50 covers its own cluster of 40, so each cluster keeps one maximum at most
    two = fc.two_clusters()
    r = kc.cpu_keypoints(two, dict(k=12, nms_k=50, gamma21=1.0, gamma32=1.0))
    assert (~np.isnan(r["saliency"])).sum() > 40 and r["count"] in (1, 2)
    # points metres apart under a gate of 0.5 m: every neighbourhood is the point alone
    sparse = np.ascontiguousarray(fc.scene()[:64] * F(40.0))
    eig, cnt, _, _ = kc.cpu_inputs(sparse, dict(k=8, nms_k=8, max_dist=0.5, min_pts=0))
    assert np.all(cnt == 1) and np.isnan(eig).all()


def test_the_chains_scene_has_keypoints_that_pair_up():
    """The furnished scene: both samplings keep hundreds of keypoints, and dozens of the scan's lie within 0.1 m of one of the map's."""
    mp = kc.chain_scene()
    km = np.flatnonzero(kc.cpu_keypoints(mp, kc.CHAIN_KEYPOINTS, fast=True)["mask"])
    body, world, _ = kc.body_scan(0)
    ks = np.flatnonzero(kc.cpu_keypoints(body, kc.CHAIN_KEYPOINTS, fast=True)["mask"])
    d = np.linalg.norm(world[ks][:, None, :].astype(np.float64) - mp[km][None].astype(np.float64), axis=2).min(1)
    print("chain scene: map", len(mp), "points,", len(km), "keypoints; scan", len(body), "points,", len(ks), "keypoints;", int((d < 0.1).sum()), "repeat within 0.1 m")
    assert len(mp) > 6000 and 100 < len(km) < len(mp) // 4 and 100 < len(ks) < len(body) // 4 and (d < 0.1).sum() >= 50


def test_edge_cases_of_the_restatement():
    # a gate of 0, and neighbourhoods below three points: nothing is salient
    pts = fc.scene()[:200]
    for cfg in (dict(k=8, nms_k=8, max_dist=0.0), dict(k=8, nms_k=8, max_dist=0.02)):
        eig, cnt, idx, ncnt = kc.cpu_inputs(pts, cfg)
        assert np.all(cnt < 3) and (cfg["max_dist"] > 0.0 or not cnt.any())
        r = kc.restate(eig, cnt, idx, ncnt, cfg)
        assert np.isnan(r["saliency"]).all() and r["count"] == 0
    # maps of 1, 2 and 3 points: three points are collinear or span a plane, l0 is 0 up to rounding and never salient on a lattice
    for n in (1, 2, 3):
        p = F([[1.0, 2.0, 3.0], [1.0, 2.5, 3.0], [1.5, 2.0, 3.0]])[:n]
        r = kc.cpu_keypoints(p, dict(k=3, nms_k=2, min_pts=0))
        assert r["cnt"].tolist() == [n] * n
        assert n == 3 or np.isnan(r["saliency"]).all()


# ---- relocalize's plumbing --------------------------------------------------------------------------------------------------------------
class _Ctx:
    """What api.relocalize asks of a context, recorded."""

    def __init__(self, pts, kp):
        self.pts, self.kp, self.log = pts, kp, []
        self.fpfh = np.arange(len(pts) * 33, dtype=F).reshape(-1, 33)

    def map_fpfh(self, want=(), **cfg):
        self.log.append(("map_fpfh", want, cfg))
        return dict(fpfh=self.fpfh)

    def map_keypoints(self, want=(), **cfg):
        self.log.append(("map_keypoints", want, cfg))
        mask = np.zeros(len(self.pts), bool)
        mask[self.kp] = True
        return dict(mask=mask, count=len(self.kp), index=np.int64(self.kp))

    def desc_ref_set(self, desc):
        self.log.append(("desc_ref_set", np.array(desc)))

    def map_points(self):
        return self.pts

    def scan_fitness(self, x26s, max_dist):
        n = len(x26s)
        return np.arange(n, dtype=np.int32), np.zeros(n)

    def scan_size(self):
        return 10


@pytest.fixture
def canned(monkeypatch):
    from fast_limo_amd import api
    rs = np.random.RandomState(2)
    map_obj, scan_obj = _Ctx(rs.rand(50, 3).astype(F), [3, 7, 11, 40, 49]), _Ctx(rs.rand(30, 3).astype(F), [0, 4, 20, 29])
    log = []

    def pairs(ref_obj, qry_obj, q_desc, r_desc, **kw):
        log.append(("pairs", ref_obj, qry_obj, np.array(q_desc), np.array(r_desc), kw))
        return np.int64([0, 1, 3]), np.int64([4, 0, 2])

    def consensus(obj, src, dst, nh, **kw):
        log.append(("consensus", obj, np.array(src), np.array(dst), nh))
        x = np.zeros((2, 26))
        x[:, 6] = x[:, 10] = 1.0
        return dict(x26=x, tri=np.int32([[0, 1, 2], [2, 1, 0]]))
    monkeypatch.setattr(api, "desc_pairs", pairs)
    monkeypatch.setattr(api, "corr_consensus", consensus)
    monkeypatch.setattr(api, "scan_align", lambda obj, x, **k: dict(x26=np.array(x)))
    return map_obj, scan_obj, log


def test_relocalize_without_keypoints_forwards_what_it_forwarded_before(canned):
    from fast_limo_amd import api
    map_obj, scan_obj, log = canned
    for kw in ({}, dict(keypoints=None), dict(keypoints=None, scan_keypoints=dict(k=5))):
        del log[:], map_obj.log[:], scan_obj.log[:]
        out = api.relocalize(map_obj, scan_obj, nh=64, fpfh=dict(k=12), ratio=0.8, **kw)
        assert sorted(out) == ["align", "consensus", "dst", "fitness", "fpfh", "pairs", "src", "x26"]
        for obj in (map_obj, scan_obj):                                   # FPFH of every point, all of it resident, nothing else asked
            assert [e[0] for e in obj.log] == ["map_fpfh", "desc_ref_set"] and obj.log[0][1:] == ((), dict(k=12))
            assert obj.log[1][1].tobytes() == obj.fpfh.tobytes()
        stage, ref_obj, qry_obj, q, r, pkw = log[0]
        assert stage == "pairs" and ref_obj is map_obj and qry_obj is scan_obj and pkw == dict(ratio=0.8, mutual=True)
        assert q.tobytes() == scan_obj.fpfh.tobytes() and r.tobytes() == map_obj.fpfh.tobytes()
        qi, rj = np.int64([0, 1, 3]), np.int64([4, 0, 2])
        assert np.array_equal(out["pairs"][0], qi) and np.array_equal(out["pairs"][1], rj)
        assert np.array_equal(out["src"], scan_obj.pts[qi]) and np.array_equal(out["dst"], map_obj.pts[rj])
        assert log[1][0] == "consensus" and np.array_equal(log[1][2], scan_obj.pts[qi]) and np.array_equal(log[1][3], map_obj.pts[rj])


def test_relocalize_with_keypoints_matches_their_rows_and_answers_in_original_indices(canned):
    from fast_limo_amd import api
    map_obj, scan_obj, log = canned
    out = api.relocalize(map_obj, scan_obj, nh=64, fpfh=dict(k=12), keypoints=dict(k=20, nms_k=9), scan_keypoints=dict(k=21, gamma21=0.5))
    ks, km = np.int64(scan_obj.kp), np.int64(map_obj.kp)
    assert [e[0] for e in map_obj.log] == ["map_fpfh", "map_keypoints", "desc_ref_set"] and map_obj.log[1][1:] == ((), dict(k=20, nms_k=9))
    assert [e[0] for e in scan_obj.log] == ["map_fpfh", "map_keypoints", "desc_ref_set"] and scan_obj.log[1][1:] == ((), dict(k=21, gamma21=0.5))
    assert map_obj.log[0][1:] == ((), dict(k=12))                         # FPFH is still formed for every point
    assert map_obj.log[2][1].tobytes() == map_obj.fpfh[km].tobytes() and scan_obj.log[2][1].tobytes() == scan_obj.fpfh[ks].tobytes()
    assert log[0][3].tobytes() == scan_obj.fpfh[ks].tobytes() and log[0][4].tobytes() == map_obj.fpfh[km].tobytes()
    qi, rj = ks[[0, 1, 3]], km[[4, 0, 2]]
    assert np.array_equal(out["pairs"][0], qi) and np.array_equal(out["pairs"][1], rj) and out["pairs"][0].dtype == np.int64
    assert np.array_equal(out["src"], scan_obj.pts[qi]) and np.array_equal(out["dst"], map_obj.pts[rj])
    assert np.array_equal(log[1][2], scan_obj.pts[qi]) and np.array_equal(log[1][3], map_obj.pts[rj])
    assert np.array_equal(out["keypoints"][0], ks) and np.array_equal(out["keypoints"][1], km)
    assert out["fpfh"][0] is scan_obj.fpfh and out["fpfh"][1] is map_obj.fpfh
    # without scan_keypoints both sides take the same fields
    del map_obj.log[:], scan_obj.log[:]
    api.relocalize(map_obj, scan_obj, nh=64, keypoints={})
    assert map_obj.log[1][1:] == ((), {}) and scan_obj.log[1][1:] == ((), {})


def test_mirror_header_declares_keypoints(tmp_path):
    """The mirror's Mapper carries keypoints (compile-only)."""
    import subprocess
    tu ="""#include "fast_limo/Modules/Mapper.hpp"
int f(fast_limo::Mapper& map, std::vector<unsigned char>& mask, std::vector<double>& sal, std::vector<int32_t>& cnt, size_t* count) {
  flimo_keypoint_cfg cfg{32, 0.5f, 5, 0.975f, 0.975f, 32, 0.4f};
  int rc = map.keypoints(0, 10, cfg, mask);
  rc += map.keypoints(0, 10, cfg, mask, &sal, &cnt, count);
  return rc;
}
"""
    src = tmp_path / "keypoints.cpp"
    src.write_text(tu)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
