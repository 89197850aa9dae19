"""The local map (forget map points outside a box) as far as it can be checked without a GPU: both libraries export the new entry
points, and the policy's rule -- flimo_local_map_rule, the pure host function Localizer::set_local_map applies after every map
insert -- decides as INTEGRATION.md states it.  The crop itself runs on the GPU: tests/test_gpu_local_map.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule(L, p, half, recentre, centre, have):
    lo = np.full(3, -77.0, np.float32)
    hi = np.full(3, -77.0, np.float32)
    rc = L.flimo_local_map_rule(np.asarray(p, np.float64), np.asarray(half, np.float32), float(recentre), centre, C.byref(have), lo, hi)
    return rc, lo, hi


def test_new_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    for name in ("flimo_map_crop_box", "flimo_map_crop_stats"):
        assert hasattr(L, name), name
        assert name in _lib.HIP_SYMBOLS
    assert "flimo_map_crop_box" in open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    assert "flimo_map_crop_stats" in open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    H = api.load_host()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in ("flimo_loc_set_local_map", "flimo_local_map_rule"):
        assert hasattr(H, name), name
        assert name in api.HOST_SYMBOLS and name in decl
    assert hasattr(_lib.HipCtx, "map_crop_box") and hasattr(api.Localizer, "set_local_map")


def test_crop_box_rejects_a_null_context(built):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    lo = np.zeros(3, np.float32)
    hi = np.ones(3, np.float32)
    removed = C.c_size_t(5)
    assert L.flimo_map_crop_box(None, lo.ctypes.data, hi.ctypes.data, C.byref(removed)) == -2      # FLIMO_ERR_INVALID
    assert removed.value == 0


def test_rule_first_call_sets_the_centre_and_the_box_is_float_of_centre_plus_minus_half(built):
    from fast_limo_amd import api
    L = api.load_host()
    centre = np.zeros(3, np.float64)
    have = C.c_int(0)
    # a position that float32 cannot hold: the box is rounded once, from the float64 sum
    p = np.array([1000.0 + 1e-7, -3.25, 0.1], np.float64)
    half = np.array([60.3, 60.3, 20.7], np.float32)
    rc, lo, hi = _rule(L, p, half, 5.0, centre, have)
    assert rc == 1 and have.value == 1
    assert np.array_equal(centre, p)
    assert np.array_equal(lo, (p - half.astype(np.float64)).astype(np.float32))
    assert np.array_equal(hi, (p + half.astype(np.float64)).astype(np.float32))


def test_rule_recentres_strictly_beyond_the_distance(built):
    from fast_limo_amd import api
    L = api.load_host()
    half = np.array([50.0, 50.0, 10.0], np.float32)
    d = np.float32(5.0)
    centre = np.zeros(3, np.float64)
    have = C.c_int(0)
    assert _rule(L, [0.0, 0.0, 0.0], half, d, centre, have)[0] == 1
    # exactly recentre_dist: stays; nothing is written
    rc, lo, hi = _rule(L, [float(d), 0.0, 0.0], half, d, centre, have)
    assert rc == 0 and np.array_equal(centre, np.zeros(3)) and np.all(lo == -77.0) and np.all(hi == -77.0)
    rc, _, _ = _rule(L, [0.0, -float(d), 0.0], half, d, centre, have)
    assert rc == 0
    # the next float above: re-centres there
    up = float(np.nextafter(d, np.float32(np.inf)))
    rc, lo, hi = _rule(L, [0.0, 0.0, up], half, d, centre, have)
    assert rc == 1 and np.array_equal(centre, [0.0, 0.0, up])
    assert np.array_equal(lo, (centre - half.astype(np.float64)).astype(np.float32))
    assert np.array_equal(hi, (centre + half.astype(np.float64)).astype(np.float32))
    # from the new centre the distance counts afresh
    assert _rule(L, [0.0, 0.0, up + 4.0], half, d, centre, have)[0] == 0


def test_rule_uses_the_per_axis_maximum_not_the_euclidean_norm(built):
    from fast_limo_amd import api
    L = api.load_host()
    half = np.array([50.0, 50.0, 10.0], np.float32)
    centre = np.zeros(3, np.float64)
    have = C.c_int(0)
    assert _rule(L, [10.0, 20.0, 30.0], half, 5.0, centre, have)[0] == 1
    # |d| = (4, 4, 4): norm 6.9 > 5, per-axis maximum 4 <= 5
    assert _rule(L, [14.0, 24.0, 34.0], half, 5.0, centre, have)[0] == 0
    assert np.array_equal(centre, [10.0, 20.0, 30.0])
    # one axis alone beyond the distance is enough
    assert _rule(L, [10.0, 15.5, 30.0], half, 5.0, centre, have)[0] == 0
    assert _rule(L, [10.0, 15.5, 24.5], half, 5.0, centre, have)[0] == 1
    assert np.array_equal(centre, [10.0, 15.5, 24.5])


def test_rule_non_positive_or_non_finite_arguments_switch_the_policy_off(built):
    from fast_limo_amd import api
    L = api.load_host()
    for half, dist in (([50.0, 0.0, 10.0], 5.0), ([50.0, 50.0, -1.0], 5.0), ([np.nan, 50.0, 10.0], 5.0), ([50.0, np.inf, 10.0], 5.0),
                       ([50.0, 50.0, 10.0], np.nan), ([50.0, 50.0, 10.0], np.inf)):
        centre = np.full(3, 9.0, np.float64)
        have = C.c_int(0)
        rc, lo, hi = _rule(L, [1.0, 2.0, 3.0], half, dist, centre, have)
        assert rc == -1 and have.value == 0, (half, dist)
        assert np.array_equal(centre, [9.0, 9.0, 9.0]) and np.all(lo == -77.0) and np.all(hi == -77.0)
    # a position that is not finite is no centre: no crop, state untouched
    centre = np.zeros(3, np.float64)
    have = C.c_int(0)
    assert _rule(L, [np.nan, 0.0, 0.0], [50.0, 50.0, 10.0], 5.0, centre, have)[0] == 0 and have.value == 0


def test_python_rule_object_follows_the_c_function(built):
    from fast_limo_amd import api
    r = api.LocalMapRule([30.0, 30.0, 10.0], 5.0)
    box = r.step([1.0, 2.0, 3.0])
    assert box is not None and np.array_equal(box[0], np.array([-29.0, -28.0, -7.0], np.float32))
    assert r.step([5.0, 2.0, 3.0]) is None and not r.off
    assert r.step([7.0, 2.0, 3.0]) is not None
    off = api.LocalMapRule([30.0, 0.0, 10.0], 5.0)
    assert off.step([0.0, 0.0, 0.0]) is None and off.off


def test_mirror_headers_declare_the_local_map_calls():
    """The mirror's C++ headers carry the additions (compile-only, like the drop-in call-site check)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
#include "fast_limo/Modules/Localizer.hpp"
void f(fast_limo::Localizer& loc, fast_limo::Mapper& map) {
  const float half[3] = {60.f, 60.f, 20.f}, lo[3] = {0.f, 0.f, 0.f}, hi[3] = {1.f, 1.f, 1.f};
  loc.set_local_map(half, 5.0f);
  map.crop_box(lo, hi);
  size_t n = map.last_crop_removed(); (void)n;
  double p[3] = {0, 0, 0}, c[3]; int have = 0; float a[3], b[3];
  int rc = fast_limo::Localizer::local_map_rule(p, half, 5.0f, c, &have, a, b); (void)rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "local_map.cpp")
        open(src, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
