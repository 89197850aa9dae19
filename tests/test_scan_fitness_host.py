"""Scoring pose hypotheses of the resident scan against the map (flimo_scan_fitness) as far as it can be checked without a GPU: the
entry points are exported and declared, a NULL context is rejected by both libraries, the mirror header carries Mapper::fitness, and
the premise of the GPU ranking test holds for the yardstick itself: on the standard scene the undisplaced pose wins clearly.  The
call itself runs on the GPU: tests/test_gpu_scan_fitness.py."""
import os
import subprocess
import tempfile

import numpy as np

import scan_fitness_common as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_fitness_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    assert hasattr(L, "flimo_scan_fitness") and "flimo_scan_fitness" in _lib.HIP_SYMBOLS
    assert hasattr(L, "flimo_set_fitness_chunk") and "flimo_set_fitness_chunk" in _lib.HIP_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    assert "flimo_scan_fitness(" in hdr and "Mapper.cpp:72" in hdr and "getFitnessScore" in hdr
    assert "flimo_set_fitness_chunk(" in open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    H = api.load_host()
    assert hasattr(H, "flimo_loc_scan_fitness") and "flimo_loc_scan_fitness" in api.HOST_SYMBOLS
    assert "flimo_loc_scan_fitness(" in open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for cls, names in ((_lib.HipCtx, ("scan_fitness", "set_fitness_chunk")), (api.Localizer, ("scan_fitness",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert callable(api.fitness_cost)


def test_scan_fitness_rejects_a_null_context(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    x = sf.standard_poses()[:2].copy()
    inl, s = np.full(2, 7, np.int32), np.full(2, 7.0)
    sqd, idx = np.full((2, 4), 7, np.float32), np.full((2, 4), 7, np.int32)
    assert L.flimo_scan_fitness(None, x.ctypes.data, 2, 1.0, inl.ctypes.data, s.ctypes.data, sqd.ctypes.data, idx.ctypes.data) == -2      # FLIMO_ERR_INVALID
    assert L.flimo_set_fitness_chunk(None, 128) == -2
    H = api.load_host()
    assert H.flimo_loc_scan_fitness(None, x.ctypes.data, 2, 1.0, inl.ctypes.data, s.ctypes.data, sqd.ctypes.data, idx.ctypes.data) == -2
    assert np.all(inl == 7) and np.all(s == 7) and np.all(sqd == 7) and np.all(idx == 7)


def test_fitness_cost_is_the_truncated_least_squares_cost():
    from fast_limo_amd import api
    c = api.fitness_cost(np.int32([10, 7, 0]), np.float64([1.5, 0.25, 0.0]), 10, 0.5)
    assert c.dtype == np.float64 and list(c) == [1.5, 0.25 + 3 * 0.25, 10 * 0.25]
    assert float(api.fitness_cost(3, 2.0, 5, 2.0)) == 2.0 + 2 * 4.0


def test_mirror_header_declares_fitness():
    """The mirror's Mapper carries fitness in both forms (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
int f(fast_limo::Mapper& map, const double* x26) {
  std::vector<int32_t> inliers, nn_idx;
  std::vector<double> sum_sqd;
  std::vector<float> nn_sqd;
  int rc = map.fitness(x26, 64, 1.0f, inliers, sum_sqd);
  rc += map.fitness(x26, 64, INFINITY, inliers, sum_sqd, &nn_sqd, &nn_idx);
  return rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "fitness.cpp")
        open(src, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_undisplaced_pose_wins_clearly_on_the_standard_scene(oracle):
    """The premise of the GPU ranking test, for the numpy restatement over the oracle octree's points at gate 0.5 m: the true pose
    has strictly the most inliers and strictly the lowest fitness_cost, and the runner-up's cost is at least 1.5 times the
    winner's.  (A float64 k-d tree gave 1008 inliers against 838 and a cost of 34.6 against about 71.)"""
    from fast_limo_amd import api
    oc = oracle.Octree()
    for b in sf.standard_batches():
        oc.update(b)
    mp = oc.points()
    assert 0 < mp.shape[0] == oc.size() <= sf.N_MAP
    scan, poses = sf.standard_scan(), sf.standard_poses()
    assert poses.shape == (125, 26) and np.array_equal(poses[sf.TRUE_POSE], sf.x26_of())
    gate = 0.5
    inl, s, nn_sqd, _ = sf.yardstick([sf.world_points(x, scan) for x in poses], mp, gate)
    cost = api.fitness_cost(inl, s, scan.shape[0], gate)
    others = np.arange(125) != sf.TRUE_POSE
    print(f"inliers {inl[sf.TRUE_POSE]} against {inl[others].max()}, cost {cost[sf.TRUE_POSE]:.3f} against {cost[others].min():.3f}")
    assert inl[sf.TRUE_POSE] > inl[others].max()
    assert cost[sf.TRUE_POSE] < cost[others].min()
    assert cost[others].min() >= 1.5 * cost[sf.TRUE_POSE]
    # the yardstick's own consistency: a gated-out query is -1 and pays the gate's square
    assert np.all((nn_sqd >= 0).sum(1) == inl) and np.all(nn_sqd[nn_sqd >= 0] < np.float32(gate) * np.float32(gate))
