"""k-NN for k up to 64 with a distance gate (flimo_knn_k; Octree::knn, reference Objects/Octree.hpp:526-555) as far as it can be
checked without a GPU: the entry points are exported and declared, the mirror header carries Mapper::knn with the template's
signature, and the yardstick of the GPU tests -- a numpy brute force in the order (float32 distance bits, index) -- gives bit for
bit the distances of the oracle octree's knn for every k.  The search itself runs on the GPU: tests/test_gpu_knn_k.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from knn_k_common import brute_knn
from radius_common import bits, box_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_k_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    assert hasattr(L, "flimo_knn_k") and "flimo_knn_k" in _lib.HIP_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    assert "flimo_knn_k" in hdr and "FLIMO_KNN_MAX_K" in hdr and "Octree.hpp:526-555" in hdr
    H = api.load_host()
    assert hasattr(H, "flimo_loc_map_knn") and "flimo_loc_map_knn" in api.HOST_SYMBOLS
    assert "flimo_loc_map_knn" in open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    assert hasattr(_lib.HipCtx, "knn_k") and hasattr(api.Localizer, "map_knn")


def test_knn_k_rejects_a_null_context(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    q = np.zeros(3, np.float32)
    idx, sqd, cnt = np.full(8, 7, np.int32), np.full(8, 7, np.float32), np.full(1, 7, np.int32)
    assert L.flimo_knn_k(None, q.ctypes.data, 1, 8, float("inf"), idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data) == -2      # FLIMO_ERR_INVALID
    H = api.load_host()
    assert H.flimo_loc_map_knn(None, q.ctypes.data, 1, 8, float("inf"), idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data) == -2
    assert np.all(idx == 7) and np.all(cnt == 7)


def test_mirror_header_declares_knn():
    """The mirror's Mapper carries knn with the template's signature, and the batch form (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
void f(fast_limo::Mapper& map, const PointType& query) {
  std::vector<PointType> neighbors;
  std::vector<float> distances;
  map.knn(query, 20, neighbors, distances);
  const float q[6] = {0, 0, 0, 1, 1, 1};
  std::vector<int32_t> idx, cnt; std::vector<float> sqd, xyz;
  int rc = map.knn(q, 2, 64, 1.5f, idx, sqd, cnt, &xyz); (void)rc;
  rc = map.knn(q, 2, FLIMO_KNN_MAX_K, INFINITY, idx, sqd, cnt); (void)rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "knn.cpp")
        open(src, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_brute_force_yardstick_equals_the_oracle_octree(oracle):
    """For k in (1, 5, 6, 8, 16, 33, 64) the first k distances of the brute force (sqdist_f32, sorted by (bits, index)) are bit-equal
    to oracle_py.Octree.knn(q, k), on the box world fed in 12 batches of 3 000 points."""
    batches = box_batches(12, 3000)
    oc = oracle.Octree()
    for b in batches:
        oc.update(b)
    pts = oc.points()
    assert 0 < pts.shape[0] == oc.size() < sum(b.shape[0] for b in batches)
    rs = np.random.RandomState(21)
    q = np.concatenate([pts[rs.choice(pts.shape[0], 1200)] + rs.normal(0, 0.2, (1200, 3)).astype(np.float32),
                        rs.uniform(-27, 27, (700, 3)).astype(np.float32), pts[:60],
                        rs.uniform(-25, 25, (20, 3)).astype(np.float32) + np.float32(500.0)]).astype(np.float32)
    for k in (1, 5, 6, 8, 16, 33, 64):
        _, osqd, ocnt, _ = oc.knn(q, k, num_threads=8)
        bidx, bsqd, bcnt = brute_knn(q, pts, k)
        assert np.all(ocnt == k) and np.all(bcnt == k)
        np.testing.assert_array_equal(bits(bsqd), bits(osqd), err_msg=f"k = {k}")
        assert np.all(np.diff(bsqd.astype(np.float64), axis=1) >= 0)
    # the gate of the brute force is the radius search's predicate
    bidx, bsqd, bcnt = brute_knn(q[:200], pts, 16, 1.0)
    d = np.float32(1.0) * np.float32(1.0)
    full = brute_knn(q[:200], pts, 16)
    for i in range(200):
        n = int((full[1][i] < d).sum())
        assert bcnt[i] == n and np.array_equal(bidx[i, :n], full[0][i, :n]) and np.all(bidx[i, n:] == -1) and np.all(bsqd[i, n:] == 0)
