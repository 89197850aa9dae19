"""GPU suite: the range rule of the map entries.  Every entry that takes a range [first, first + n) of the stored points refuses one
that ends beyond the map with FLIMO_ERR_INVALID and a message that names the entry, the range and the map's size, before it looks at
anything else of the range and without touching the map; first == the map's size with n == 0 is the empty range at the end and
succeeds.  The rule is written once (check_range in flimo_capi_query.hip): this file holds that one copy to what each entry did when it
had its own.  Every case is a call that launches nothing."""
import ctypes as C

import numpy as np
import pytest

from common import CAPS

pytestmark = pytest.mark.gpu

OK, ERR_INVALID = 0, -2
N = 5
# (first, n): beyond the end with nothing to read, over the end, and a first + n that wraps to 1
BAD_RANGES = [(6, 0), (3, 3), (2 ** 64 - 1, 2)]


def _message(name, first, n, size):
    return f"{name}: the range [{first}, {first} + {n}) ends beyond the map's {size} points"


@pytest.fixture(scope="module")
def ctx(built):
    from fast_limo_amd import _lib
    c = _lib.HipCtx(0)
    c.map_config(0.2, 2, True, 0.0)
    c.map_add(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 3, 3]]), stamp=0.5)
    assert c.map_size() == N
    yield c
    c.close()


def _entries():
    """name in the messages -> call(L, h, first, n): the entry through ctypes, valid arguments but the range, room for 8 points"""
    from fast_limo_amd import _lib
    buf = {k: np.zeros(8 * 33, np.float64) for k in "abcde"}
    a, b, c, d, e = (buf[k].ctypes.data for k in "abcde")
    keep = [buf]                                                       # (the closures below hold the addresses only)
    oc, fc, kc = _lib.outlier_cfg(k=3), _lib.fpfh_cfg(k=3, normal_k=3), _lib.keypoint_cfg(k=3, nms_k=3)
    cc, vc = _lib.cluster_cfg(), _lib.voxel_cfg()
    sel = _lib.plane_sel(normal=(0, 0, 1), anchor=(0, 0, 0))
    removed = C.c_size_t(0)
    R = C.byref(removed)
    return keep, {
        "map normals": lambda L, h, f, n: L.flimo_map_normals_range(h, f, n, 3, float("inf"), 3, None, a, b, c, d, e),
        "map outliers": lambda L, h, f, n: L.flimo_map_outliers(h, f, n, C.byref(oc), a, b, c, None),
        "remove outliers": lambda L, h, f, n: L.flimo_map_remove_outliers(h, f, n, C.byref(oc), R, None),
        "map fpfh": lambda L, h, f, n: L.flimo_map_fpfh(h, f, n, C.byref(fc), a, b, c),
        "map keypoints": lambda L, h, f, n: L.flimo_map_keypoints(h, f, n, C.byref(kc), a, b, c, R),
        "map clusters": lambda L, h, f, n: L.flimo_map_clusters(h, f, n, C.byref(cc), a, b, c, None),
        "remove clusters": lambda L, h, f, n: L.flimo_map_remove_clusters(h, f, n, C.byref(cc), R, None),
        "plane mask": lambda L, h, f, n: L.flimo_map_plane_mask(h, f, n, C.byref(sel), a, R),
        "remove plane": lambda L, h, f, n: L.flimo_map_remove_plane(h, f, n, C.byref(sel), R),
        "voxel mask": lambda L, h, f, n: L.flimo_map_voxel_mask(h, f, n, C.byref(vc), a, b, None),
        "map thin": lambda L, h, f, n: L.flimo_map_thin(h, f, n, C.byref(vc), R, None),
    }


RANGE_ENTRIES = ["map normals", "map outliers", "remove outliers", "map fpfh", "map keypoints", "map clusters", "remove clusters",
                 "plane mask", "remove plane", "voxel mask", "map thin"]


@pytest.mark.parametrize("name", RANGE_ENTRIES)
def test_a_range_beyond_the_map_is_refused_by_name_and_the_empty_range_at_the_end_is_not(ctx, name):
    keep, entries = _entries()
    assert sorted(entries) == sorted(RANGE_ENTRIES)
    call, L, h = entries[name], ctx._L, ctx._h
    pts = ctx.map_points().copy()
    assert call(L, h, N, 0) == OK, L.flimo_last_error(h).decode()
    for first, n in BAD_RANGES:
        assert call(L, h, first, n) == ERR_INVALID, (first, n)
        assert L.flimo_last_error(h).decode() == _message(name, first, n, N)
        assert ctx.map_size() == N
    np.testing.assert_array_equal(ctx.map_points(), pts)


def test_map_voxels_has_no_range_to_refuse(ctx):
    """The control: the entry without a range goes through the same argument check (with the range 0, 0) and succeeds."""
    out = ctx.map_voxels(want=("count",), leaf=0.25)
    assert out["nv"] == N and out["stats"]["voxels"] == N and ctx.map_size() == N


def test_the_localizer_forwards_the_range_to_the_contexts_own_check(built):
    """A fresh Localizer's map is empty: the message names 0 points, and it is the context that wrote it."""
    from fast_limo_amd import _lib, api
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        H, lh, hip = loc._L, loc._h, loc.hip
        oc, vc = _lib.outlier_cfg(k=3), _lib.voxel_cfg()
        removed = C.c_size_t(7)
        assert H.flimo_loc_map_outliers(lh, 6, 0, C.byref(oc), None, None, None, None) == ERR_INVALID
        assert hip._L.flimo_last_error(hip._h).decode() == _message("map outliers", 6, 0, 0)
        assert H.flimo_loc_map_thin(lh, 6, 0, C.byref(vc), C.byref(removed), None) == ERR_INVALID
        assert hip._L.flimo_last_error(hip._h).decode() == _message("map thin", 6, 0, 0)
        assert removed.value == 7 and loc.map_size() == 0
        assert H.flimo_loc_map_outliers(lh, 0, 0, C.byref(oc), None, None, None, None) == OK      # the empty range of the empty map
    finally:
        loc.close()
