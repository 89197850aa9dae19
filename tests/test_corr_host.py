"""Pose hypotheses from point correspondences (flimo_corr_poses) as far as they can be checked without a GPU: the entry points are
exported, declared and listed; a NULL context is rejected by both libraries; flimo_corr_pose_host -- the host / device function the
solve kernel calls, run on the host -- against the numpy restatement of include/flimo_c.h (tests/corr_common.py): status, the bits
of pose7 and the bits of the float32 matrix with no tolerance; and the premise of the GPU recovery test for the restatement itself.
The call itself runs on the GPU: tests/test_gpu_corr.py."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import corr_common as cc
import scan_fitness_common as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def host(api, S, D, **cfg):
    """api.corr_pose_host per triangle of S, D [nh, 3, 3]: (status [nh], pose [nh, 7], rt [nh, 3, 4])."""
    got = [api.corr_pose_host(s, d, **cfg) for s, d in zip(S, D)]
    return (np.int32([g[0] for g in got]), np.stack([g[1] for g in got]), np.stack([g[2] for g in got]))


def equal_bits(got, ref, tag=""):
    """status, and the bits of pose7 and rt with no tolerance (every NaN pattern counts as NaN)."""
    status, pose, rt = got
    r_status, r_pose, r_rt = ref[:3]
    np.testing.assert_array_equal(status, r_status, err_msg=f"{tag}: status")
    bad = r_status != cc.OK
    assert np.isnan(pose[bad]).all() and np.isnan(rt[bad]).all(), f"{tag}: a hypothesis that is not OK has NaN results"
    np.testing.assert_array_equal(pose[~bad].view(np.uint64), r_pose[~bad].view(np.uint64), err_msg=f"{tag}: pose7 bits")
    np.testing.assert_array_equal(rt[~bad].view(np.uint32), r_rt[~bad].view(np.uint32), err_msg=f"{tag}: rt bits")


def rot(axis, deg):
    """Rodrigues' rotation matrix, float64."""
    a = np.float64(axis) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(deg)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def test_corr_entry_points_are_exported_declared_and_listed(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    for name in ("flimo_corr_poses", "flimo_corr_pose_host"):
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS and name + "(" in pub, name
    for word in ("flimo_corr_cfg", "FLIMO_CORR_OK 0", "FLIMO_CORR_DEGENERATE 1", "FLIMO_CORR_REJECTED 2", "SampleConsensusPrerejective"):
        assert word in pub, word
    assert hasattr(L, "flimo_set_corr_chunk") and "flimo_set_corr_chunk" in _lib.HIP_SYMBOLS
    assert "flimo_set_corr_chunk(" in open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    H = api.load_host()
    assert hasattr(H, "flimo_loc_corr_poses") and "flimo_loc_corr_poses" in api.HOST_SYMBOLS
    assert "flimo_loc_corr_poses(" in open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for cls, names in ((_lib.HipCtx, ("corr_poses", "set_corr_chunk")), (api.Localizer, ("corr_poses",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    for name in ("corr_triplets", "corr_pose_host", "corr_consensus"):
        assert callable(getattr(api, name)), name
    assert callable(_lib.corr_cfg) and _lib.HipCtx.corr_poses is api.Localizer.corr_poses      # (one method, two symbols)
    assert C.sizeof(_lib.CorrCfg) == 12
    assert (_lib.CORR_OK, _lib.CORR_DEGENERATE, _lib.CORR_REJECTED) == (cc.OK, cc.DEGENERATE, cc.REJECTED) == (0, 1, 2)


def test_corr_poses_rejects_a_null_context_and_the_host_function_its_bad_arguments(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    src = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    tri = np.int32([[0, 1, 2]])
    k = _lib.corr_cfg(0.9, 0.1, 1.0)
    status, inl, s = np.full(1, 7, np.int32), np.full(1, 7, np.int32), np.full(1, 7.0)
    pose, pairs = np.full((1, 7), 7.0), np.full((1, 3), 7, np.float32)
    args = (src.ctypes.data, src.ctypes.data, 3, tri.ctypes.data, 1, C.byref(k), status.ctypes.data, inl.ctypes.data, s.ctypes.data,
            pose.ctypes.data, pairs.ctypes.data)
    assert L.flimo_corr_poses(None, *args) == -2      # FLIMO_ERR_INVALID
    assert L.flimo_set_corr_chunk(None, 8) == -2
    assert api.load_host().flimo_loc_corr_poses(None, *args) == -2
    for a in (status, inl, s, pose, pairs):
        assert np.all(a == 7)
    p7, rt = np.full(7, 7.0), np.full(12, 7, np.float32)
    fn = L.flimo_corr_pose_host
    assert fn(None, src.ctypes.data, C.byref(k), p7.ctypes.data, rt.ctypes.data) == -2
    assert fn(src.ctypes.data, None, C.byref(k), p7.ctypes.data, rt.ctypes.data) == -2
    assert fn(src.ctypes.data, src.ctypes.data, None, p7.ctypes.data, rt.ctypes.data) == -2
    assert fn(src.ctypes.data, src.ctypes.data, C.byref(k), None, rt.ctypes.data) == -2
    assert fn(src.ctypes.data, src.ctypes.data, C.byref(k), p7.ctypes.data, None) == -2
    for bad in ((-0.1, 0.1, 1.0), (1.5, 0.1, 1.0), (float("nan"), 0.1, 1.0), (0.9, -1.0, 1.0), (0.9, float("nan"), 1.0), (0.9, 0.1, -1.0),
                (0.9, 0.1, float("nan"))):
        kb = _lib.corr_cfg(*bad)
        assert fn(src.ctypes.data, src.ctypes.data, C.byref(kb), p7.ctypes.data, rt.ctypes.data) == -2, bad
    assert np.all(p7 == 7) and np.all(rt == 7)
    assert fn(src.ctypes.data, src.ctypes.data, C.byref(_lib.corr_cfg(1.0, 0.0, INF)), p7.ctypes.data, rt.ctypes.data) == 0


def test_corr_triplets_are_distinct_seeded_and_cover_every_index():
    from fast_limo_amd import api
    t = api.corr_triplets(5, 20000, 3)
    assert t.shape == (20000, 3) and t.dtype == np.int32 and t.min() == 0 and t.max() == 4
    assert np.all((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2]))
    uniq, count = np.unique(t, axis=0, return_counts=True)
    assert uniq.shape[0] == 60 and count.min() > 0.7 * 20000 / 60 and count.max() < 1.3 * 20000 / 60      # ordered triples, evenly
    assert np.array_equal(t, api.corr_triplets(5, 20000, 3)) and not np.array_equal(t, api.corr_triplets(5, 20000, 4))
    assert np.array_equal(np.sort(api.corr_triplets(3, 50, 0), axis=1), np.tile(np.int32([0, 1, 2]), (50, 1)))
    with pytest.raises(ValueError):
        api.corr_triplets(2, 1)


def test_host_pose_equals_the_restatement_on_random_triplets_of_a_scene(built):
    """2 000 triplets of the recovery scene (about 30 % true pairs among random ones), at the recovery test's thresholds and without
    pre-rejection: all three statuses occur, and every OK pose and matrix is the restatement's, bit for bit."""
    from fast_limo_amd import api
    src, dst, _ = cc.scene(0, np.concatenate(sf.standard_batches()))
    tri = api.corr_triplets(src.shape[0], 2000, 11)
    for cfg in (dict(edge_sim=0.9, min_edge=0.5), dict(edge_sim=0.0, min_edge=0.0), dict(edge_sim=0.5, min_edge=2.0)):
        ref = cc.solve_points(src[tri], dst[tri], **cfg)
        equal_bits(host(api, src[tri], dst[tri], max_dist=0.15, **cfg), ref, str(cfg))
        counts = [int((ref[0] == s).sum()) for s in (cc.OK, cc.DEGENERATE, cc.REJECTED)]
        print(cfg, "OK / DEGENERATE / REJECTED:", counts, "branches:", np.bincount(ref[3][ref[0] == cc.OK], minlength=4))
        assert counts[0] > 0
    assert counts[1] > 0 and counts[2] > 0


def test_host_pose_of_a_triangle_worked_by_hand(built):
    """A yaw of 90 degrees and a shift of (1, 2, 3).  src a, b, c = (0,0,0), (1,0,0), (0,2,0): u1 = x, u1 x e2 = (0,0,2) so u3 = z and
    u2 = y.  dst = Rz(90) src + t = (1,2,3), (1,3,3), (-1,2,3): u1 = y, u3 = z, u2 = -x.  R = y x^T - x y^T + z z^T = Rz(90) exactly;
    trace = 1 is the largest of (1, 0, 0, 1) by the first-on-a-tie rule, so w = 0.5 sqrt(2), z = (R10 - R01) 0.25 / w, x = y = 0;
    cs = (1/3, 2/3, 0), cd = (1/3, 7/3, 3) and t = cd - R cs rounds to (1, 2, 3)."""
    from fast_limo_amd import api
    src = np.float32([[0, 0, 0], [1, 0, 0], [0, 2, 0]])
    dst = np.float32([[1, 2, 3], [1, 3, 3], [-1, 2, 3]])
    status, pose, rt = api.corr_pose_host(src, dst, edge_sim=0.9, min_edge=0.5, max_dist=0.1)
    assert status == cc.OK
    assert list(pose[0:5]) == [1.0, 2.0, 3.0, 0.0, 0.0]
    assert abs(pose[5] - math.sqrt(0.5)) <= 2.0 ** -52 and abs(pose[6] - math.sqrt(0.5)) <= 2.0 ** -52
    assert pose[6] == 0.5 * math.sqrt(2.0) and pose[5] == 2.0 * (0.25 / pose[6])
    equal_bits(host(api, src[None], dst[None], edge_sim=0.9, min_edge=0.5), cc.solve_points(src[None], dst[None], 0.9, 0.5), "by hand")
    assert np.array_equal(rt, sf.pose_rt(pose)) and np.array_equal(rt[:, 3], np.float32([1, 2, 3]))
    # the matrix moves the three points onto their mates to float32 rounding
    w = sf.world_points(np.concatenate([pose, np.zeros(19)]), src)
    assert np.abs(w - dst).max() <= 4 * 2.0 ** -23


@pytest.mark.parametrize("axis, deg, branch", [((0, 0, 1), 0.0, 0), ((1, 0, 0), 179.0, 1), ((0, 1, 0), 179.0, 2), ((0, 0, 1), 179.0, 3),
                                               ((1, 0, 0), 180.0, 1), ((0, 1, 0), 180.0, 2), ((0, 0, 1), 180.0, 3), ((1, 2, 3), 120.0, None)])
def test_host_pose_on_each_of_shepperds_branches(built, axis, deg, branch):
    """Rotations of 0 degrees (the trace is the largest) and of about 180 degrees about x, y, z (R00, R11, R22 are): the restatement
    takes the branch meant, and the host function equals it bit for bit; the quaternion is the rotation's up to sign."""
    from fast_limo_amd import api
    rs = np.random.RandomState(5)
    S = (rs.rand(40, 3, 3) * 10 - 5).astype(np.float32)
    R = rot(axis, deg)
    D = (S.astype(np.float64) @ R.T + np.float64([3.0, -2.0, 0.5])).astype(np.float32)
    ref = cc.solve_points(S, D, 0.9, 0.5)
    ok = ref[0] == cc.OK
    assert ok.sum() >= 30
    if branch is not None:
        assert np.all(ref[3][ok] == branch)
    equal_bits(host(api, S, D, edge_sim=0.9, min_edge=0.5), ref, f"{axis} {deg}")
    a = np.float64(axis) / np.linalg.norm(axis)
    q_true = np.concatenate([a * math.sin(math.radians(deg) / 2), [math.cos(math.radians(deg) / 2)]])
    q = ref[1][ok][:, 3:7]
    assert np.abs(np.abs(q @ q_true) - 1.0).max() < 1e-5 and np.abs(ref[1][ok][:, 0:3] - [3.0, -2.0, 0.5]).max() < 1e-4


def test_host_pose_of_degenerate_and_threshold_triangles(built):
    from fast_limo_amd import api
    f = np.float32
    tri = f([[0, 0, 0], [0.5, 0, 0], [0, 1, 0]])

    def both(S, D, want, tag, **cfg):
        ref = cc.solve_points(f(S)[None], f(D)[None], cfg["edge_sim"], cfg["min_edge"])
        equal_bits(host(api, f(S)[None], f(D)[None], **cfg), ref, tag)
        assert ref[0][0] == want, tag
    # repeated indices: the same point twice (and three times), with and without a shortest edge
    for pts in ([[1, 2, 3], [1, 2, 3], [4, 5, 6]], [[1, 2, 3], [4, 5, 6], [1, 2, 3]], [[4, 5, 6], [1, 2, 3], [1, 2, 3]], [[1, 2, 3]] * 3):
        both(pts, pts, cc.DEGENERATE, "repeated point", edge_sim=0.0, min_edge=0.0)
        both(pts, pts, cc.DEGENERATE, "repeated point, min_edge", edge_sim=0.9, min_edge=0.5)
    # a collinear triangle passes both edge tests and fails in the solve: 0 / 0
    line = [[0, 0, 0], [1, 1, 1], [3, 3, 3]]
    both(line, line, cc.DEGENERATE, "collinear", edge_sim=0.9, min_edge=0.5)
    both(tri, line, cc.DEGENERATE, "collinear dst", edge_sim=0.0, min_edge=0.1)
    # a NaN coordinate, in either cloud
    for at in range(9):
        bad = tri.copy()
        bad.reshape(-1)[at] = np.nan
        both(bad, tri, cc.DEGENERATE, "NaN in src", edge_sim=0.0, min_edge=0.0)
        both(tri, bad, cc.DEGENERATE, "NaN in dst", edge_sim=0.0, min_edge=0.0)
    # an edge exactly at min_edge passes (e = 0.25 >= 0.5 * 0.5); one float32 step shorter it does not
    both(tri, tri, cc.OK, "edge at min_edge", edge_sim=0.9, min_edge=0.5)
    short = tri.copy()
    short[1, 0] = np.nextafter(f(0.5), f(0))
    both(short, tri, cc.DEGENERATE, "edge below min_edge in src", edge_sim=0.0, min_edge=0.5)
    both(tri, short, cc.DEGENERATE, "edge below min_edge in dst", edge_sim=0.0, min_edge=0.5)
    both(short, tri, cc.OK, "no shortest edge", edge_sim=0.9, min_edge=0.0)
    # a similarity exactly at the threshold passes (edges 1 and 2 m: 1 >= 0.5^2 * 4); one float32 step longer it does not
    S, D = [[0, 0, 0], [1, 0, 0], [0, 4, 0]], f([[0, 0, 0], [2, 0, 0], [0, 4, 0]])
    both(S, D, cc.OK, "similarity at the threshold", edge_sim=0.5, min_edge=0.5)
    both(D, S, cc.OK, "similarity at the threshold, clouds exchanged", edge_sim=0.5, min_edge=0.5)
    longer = D.copy()
    longer[1, 0] = np.nextafter(f(2), f(3))
    both(S, longer, cc.REJECTED, "similarity below the threshold", edge_sim=0.5, min_edge=0.5)
    both(longer, S, cc.REJECTED, "similarity below the threshold, clouds exchanged", edge_sim=0.5, min_edge=0.5)
    both(S, longer, cc.OK, "no pre-rejection", edge_sim=0.0, min_edge=0.5)
    both(tri, tri, cc.OK, "edge_sim 1 keeps congruent triangles", edge_sim=1.0, min_edge=0.0)


def test_mirror_header_declares_corr_poses():
    """The mirror's Mapper carries corr_poses (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
int f(fast_limo::Mapper& map, const float* src, const float* dst, const int32_t* tri, int32_t* status, int32_t* inliers, double* sum, double* pose,
      float* pairs) {
  flimo_corr_cfg cfg{0.9f, 0.5f, INFINITY};
  int rc = map.corr_poses(src, dst, 512, tri, 2048, &cfg, status, inliers, sum);
  rc += map.corr_poses(src, dst, 512, tri, 2048, &cfg, status, inliers, sum, pose, pairs);
  return rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corr.cpp")
        open(path, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


class _Restated:
    """``corr_poses`` by the restatement: what api.corr_consensus ranks when no GPU is there."""

    def corr_poses(self, src, dst, tri, want=("pose",), **cfg):
        return cc.reference(src, dst, tri, **cfg)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_premise_of_the_recovery_test_holds_for_the_restatement(oracle, seed):
    """The GPU recovery test's first bar for the numpy restatement over the oracle octree's stored points: 512 pairs of which about
    30 % are true (noise 0.01 m), 2048 samples, edge_sim 0.9, min_edge 0.5 m, max_dist 0.15 m -- the first row of
    api.corr_consensus lies within 0.05 m and 0.5 degrees of the true pose."""
    from fast_limo_amd import api
    oc = oracle.Octree()
    for b in sf.standard_batches():
        oc.update(b)
    src, dst, true = cc.scene(seed, oc.points())
    best = api.corr_consensus(_Restated(), src, dst, 2048, seed=seed, edge_sim=0.9, min_edge=0.5, max_dist=0.15)
    dt, dr = cc.pose_error(best["x26"][0], sf.x26_of())
    print(f"seed {seed}: {int(true.sum())} true pairs, {best['survivors']} survivors, best has {best['inliers'][0]} inliers, off by {dt:.4f} m, {dr:.3f} deg")
    assert best["x26"].shape == (8, 26) and np.all(best["x26"][:, 10] == 1.0) and np.all(np.diff(best["inliers"]) <= 0)
    assert dt <= 0.05 and dr <= 0.5
