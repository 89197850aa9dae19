"""Radius search (Octree::radiusSearch, reference Objects/Octree.hpp:453-523) as far as it can be checked without a GPU: the entry
points are exported and declared, and the reference's traversal -- restated over the oracle's octree in tests/radius_ref -- returns
exactly the points of the plain predicate `float32 squared distance < float32 radius squared`, although it hands whole octants over
without testing their points.  That is what lets flimo_radius_search promise the predicate and still be "the same answer as
Octree::radiusSearch".  The search itself runs on the GPU: tests/test_gpu_radius_search.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from radius_common import RADII, PointIds, RadiusRef, box_batches, brute_force, disagreeing_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radius_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    assert hasattr(L, "flimo_radius_search") and "flimo_radius_search" in _lib.HIP_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    assert "flimo_radius_search" in hdr and "FLIMO_RADIUS_SORTED" in hdr and "Octree.hpp:453-523" in hdr
    H = api.load_host()
    assert hasattr(H, "flimo_loc_map_radius_search") and "flimo_loc_map_radius_search" in api.HOST_SYMBOLS
    assert "flimo_loc_map_radius_search" in open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    assert hasattr(_lib.HipCtx, "radius_search") and hasattr(_lib.HipCtx, "radius_count") and hasattr(api.Localizer, "map_radius_search")
    assert _lib.RADIUS_SORTED == 1


def test_radius_search_rejects_a_null_context(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    q = np.zeros(3, np.float32)
    off = np.full(2, 7, np.uint64)
    total = C.c_uint64(9)
    assert L.flimo_radius_search(None, q.ctypes.data, 1, 1.0, 0, off.ctypes.data, None, None, None, 0, C.byref(total)) == -2      # FLIMO_ERR_INVALID
    H = api.load_host()
    assert H.flimo_loc_map_radius_search(None, q.ctypes.data, 1, 1.0, 0, off.ctypes.data, None, None, None, 0, C.byref(total)) == -2


def test_the_references_traversal_equals_the_plain_predicate():
    """Condition (set with the feature): ZERO disagreeing queries, and at least a tenth of all results through the whole-octant
    shortcut, so that the branch that takes points without testing them is really exercised."""
    batches = box_batches(12, 3000)
    ref = RadiusRef()
    for b in batches:
        ref.update(b)
    pts = ref.points()
    assert ref.size() == pts.shape[0] and 0 < pts.shape[0] < sum(b.shape[0] for b in batches)      # the insert rule dropped points
    ids = PointIds(pts)
    rs = np.random.RandomState(11)
    near = pts[rs.choice(pts.shape[0], 300)] + rs.normal(0, 0.01, (300, 3)).astype(np.float32)     # within centimetres of stored points
    q = np.concatenate([near, pts[rs.choice(pts.shape[0], 300)] + rs.normal(0, 0.3, (300, 3)).astype(np.float32),
                        rs.uniform(-27, 27, (500, 3)).astype(np.float32), pts[:40],
                        rs.uniform(-25, 25, (10, 3)).astype(np.float32) + np.float32(300.0)]).astype(np.float32)
    assert q.shape[0] >= 1000 and (near.shape[0] + 40) * 4 >= q.shape[0]
    diameter = float(np.linalg.norm(pts.max(0).astype(np.float64) - pts.min(0)))
    results = shortcut = disagree = 0
    for radius in RADII + (2.0 * diameter + 700.0,):                # the last: larger than the map, from every query
        for a in range(0, q.shape[0], 128):                         # (in slices: the largest radius returns the map per query)
            qa = q[a:a + 128]
            off_r, xyz_r, sqd_r, sc = ref.radius_search(qa, radius)
            off_b, idx_b, sqd_b = brute_force(qa, pts, radius)
            disagree += disagreeing_queries(ids, off_r, xyz_r, sqd_r, off_b, pts[idx_b], sqd_b)
            results += int(off_r[-1])
            shortcut += sc
        if radius == 0.0:
            assert results == 0
    print(f"radius_ref vs brute force: {q.shape[0]} queries x {len(RADII) + 1} radii over {pts.shape[0]} stored points: "
          f"{results} results, {shortcut} through the shortcut, {disagree} disagreeing queries")
    assert disagree == 0
    assert shortcut * 10 >= results > 0


def test_mirror_header_declares_radius_search():
    """The mirror's Mapper carries the addition with the template's signature (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
void f(fast_limo::Mapper& map, const PointType& query) {
  std::vector<PointType> neighbors;
  std::vector<float> distances;
  map.radiusSearch(query, 2.0f, neighbors, distances);
  const float q[6] = {0, 0, 0, 1, 1, 1};
  std::vector<uint64_t> offsets; std::vector<int32_t> idx; std::vector<float> sqd, xyz;
  int rc = map.radiusSearch(q, 2, 0.5f, true, offsets, idx, sqd, &xyz); (void)rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "radius.cpp")
        open(src, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
