"""Voxel statistics and thinning of the stored points (flimo_map_voxels, flimo_map_voxel_mask, flimo_map_thin) as far as they can be
checked without a GPU: both libraries export and declare the new entry points, the calls reject a null context,
flimo_voxel_key_host -- the function the key kernel calls -- equals the restatement of the lattice (tests/voxels_common.py) bit for
bit on random points, negative coordinates, -0.0, cell boundaries one float32 step either side, rounded inverse leaves and the edge
of the lattice, the numpy form of the sum's shape equals the shape written in plain Python floats, the grouping equals
np.unique(axis=0), and both thinning rules are idempotent on the restatement.  The kernels run on the GPU: tests/test_gpu_voxels.py."""
import ctypes as C
import os

import numpy as np
import pytest

import voxels_common as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
F = np.float32
D = np.float64

HIP_NAMES = ("flimo_map_voxels", "flimo_map_voxel_mask", "flimo_map_thin", "flimo_voxel_key_host", "flimo_set_voxel_plan")
HOST_NAMES = ("flimo_loc_map_voxels", "flimo_loc_map_voxel_mask", "flimo_loc_map_thin")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in HIP_NAMES:
        getattr(L, name)
    for name in HOST_NAMES:
        getattr(H, name)
    api.voxel_key_host, api.Localizer.voxel_cloud


def test_new_entry_points_are_exported_and_declared():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    dev = open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in HIP_NAMES:
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS, name
    assert "int flimo_map_voxels(flimo_ctx* ctx, const flimo_voxel_cfg* cfg, size_t cap, size_t* nv, int32_t* ijk" in pub
    assert "int flimo_map_voxel_mask(flimo_ctx* ctx, size_t first, size_t n, const flimo_voxel_cfg* cfg, int32_t* voxel" in pub
    assert "int flimo_map_thin(flimo_ctx* ctx, size_t first, size_t n, const flimo_voxel_cfg* cfg, size_t* removed, flimo_voxel_stats* stats);" in pub
    assert "int flimo_voxel_key_host(const float p[3], float leaf, int32_t ijk[3], uint64_t* key);" in pub
    assert "} flimo_voxel_cfg;" in pub and "} flimo_voxel_stats;" in pub and "tests/voxels_common.py" in pub
    for text in ("#define FLIMO_VOXEL_KEEP_FIRST 0", "#define FLIMO_VOXEL_KEEP_NEAREST 1", "#define FLIMO_VOXEL_RUN 64",
                 "#define FLIMO_VOXEL_HALF 1048576"):
        assert text in pub, text
    assert "flimo_set_voxel_plan(" in dev
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for name in ("map_voxels", "map_voxel_mask", "map_thin", "set_voxel_plan"):
        assert hasattr(_lib.HipCtx, name), name
    for name in ("map_voxels", "map_voxel_mask", "map_thin", "voxel_cloud"):
        assert hasattr(api.Localizer, name), name
    assert (_lib.VOXEL_KEEP_FIRST, _lib.VOXEL_KEEP_NEAREST, _lib.VOXEL_RUN, _lib.VOXEL_HALF) == (vc.KEEP_FIRST, vc.KEEP_NEAREST, vc.RUN, vc.HALF)
    # the structs as the header lays them out, and the wrapper's defaults as the restatement's
    assert C.sizeof(_lib.VoxelCfg) == 12 and C.sizeof(_lib.VoxelStats) == 40
    assert [f[0] for f in _lib.VoxelCfg._fields_] == ["leaf", "keep", "max_pts"]
    assert [f[0] for f in _lib.VoxelStats._fields_] == ["n", "voxels", "largest", "outside", "sel_points"]
    assert all(f[1] is C.c_uint64 for f in _lib.VoxelStats._fields_)
    k = _lib.voxel_cfg()
    assert (k.leaf, k.keep, k.max_pts) == (float(F(vc.DEFAULTS["leaf"])), vc.DEFAULTS["keep"], vc.DEFAULTS["max_pts"])
    k = _lib.voxel_cfg(leaf=0.3, keep=1)
    assert (k.leaf, k.keep, k.max_pts) == (float(F(0.3)), 1, 1)


def test_the_calls_reject_a_null_context_and_leave_their_outputs():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k = _lib.voxel_cfg()
    nv, removed, st = C.c_size_t(7), C.c_size_t(7), _lib.VoxelStats(7, 7, 7, 7, 7)
    i3, i1, d3, d6 = np.full(6, 7, np.int32), np.full(2, 7, np.int32), np.full(6, 7.0), np.full(12, 7.0)
    mask = np.full(2, 7, np.uint8)
    args = (C.byref(k), 2, C.byref(nv), i3.ctypes.data, i1.ctypes.data, i1.ctypes.data, i1.ctypes.data, d3.ctypes.data, d6.ctypes.data, C.byref(st))
    assert L.flimo_map_voxels(None, *args) == ERR_INVALID
    assert H.flimo_loc_map_voxels(None, *args) == ERR_INVALID
    assert L.flimo_map_voxel_mask(None, 0, 2, C.byref(k), i1.ctypes.data, mask.ctypes.data, C.byref(st)) == ERR_INVALID
    assert H.flimo_loc_map_voxel_mask(None, 0, 2, C.byref(k), i1.ctypes.data, mask.ctypes.data, C.byref(st)) == ERR_INVALID
    assert L.flimo_map_thin(None, 0, 2, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert H.flimo_loc_map_thin(None, 0, 2, C.byref(k), C.byref(removed), C.byref(st)) == ERR_INVALID
    assert L.flimo_set_voxel_plan(None, 1) == ERR_INVALID
    assert np.all(i3 == 7) and np.all(i1 == 7) and np.all(d3 == 7) and np.all(d6 == 7) and np.all(mask == 7)
    assert nv.value == 7 and removed.value == 7 and st.as_dict() == dict(n=7, voxels=7, largest=7, outside=7, sel_points=7)


# ---- flimo_voxel_key_host against the restatement -------------------------------------------------------------------------------------
def _host_equals_restatement(pts, leaf, what=""):
    from fast_limo_amd import api
    p = np.asarray(pts, F).reshape(-1, 3)
    ijk, key, inside = vc.keys(p, leaf)
    for i in range(len(p)):
        got_in, got_ijk, got_key = api.voxel_key_host(p[i], leaf)
        assert got_in == bool(inside[i]) and got_ijk.tolist() == ijk[i].tolist() and got_key == int(key[i]), \
            (what, leaf, p[i], got_in, got_ijk, hex(got_key), ijk[i], hex(int(key[i])))
    return ijk, key, inside


def test_random_points_bit_for_bit():
    rs = np.random.RandomState(2)
    for leaf in (0.1, 0.25, 0.3, 1.0, 7.5):
        pts = (rs.uniform(-1, 1, (400, 3)) * 10.0 ** rs.uniform(-2, 3, (400, 1))).astype(F)
        ijk, key, inside = _host_equals_restatement(pts, leaf, "random")
        assert inside.all()
        # the key orders like (cz, cy, cx)
        o = np.argsort(key, kind="stable")
        c = ijk[o].astype(np.int64)
        tup = [tuple(r) for r in c[:, ::-1]]
        assert tup == sorted(tup)


def test_negative_coordinates_floor_and_do_not_truncate():
    from fast_limo_amd import api
    inside, ijk, _ = api.voxel_key_host((-0.1, -0.25, -0.26), 0.25)
    assert inside and ijk.tolist() == [-1, -1, -2]
    inside, ijk, key = api.voxel_key_host((0.1, 0.25, 0.26), 0.25)
    assert inside and ijk.tolist() == [0, 1, 1] and key == ((1 + vc.HALF) << 42) | ((1 + vc.HALF) << 21) | vc.HALF
    # -0.0 lies in cell 0 like +0.0: floorf(-0.0) is -0.0, and (int)-0.0 is 0
    a, b = api.voxel_key_host((-0.0, -0.0, -0.0), 0.5), api.voxel_key_host((0.0, 0.0, 0.0), 0.5)
    assert a[0] and b[0] and a[1].tolist() == b[1].tolist() == [0, 0, 0] and a[2] == b[2]
    _host_equals_restatement(F([[-0.0, 0.0, -0.0], [-1e-30, 1e-30, -1e-45]]), 0.5, "zeros")


@pytest.mark.parametrize("leaf", [0.25, 0.5])
def test_cell_boundaries_of_dyadic_leaves_one_step_either_side(leaf):
    """x = k * leaf is exact and 1 / leaf is exact: the point itself opens cell k, one float32 step below lies in cell k - 1."""
    from fast_limo_amd import api
    for k in (-1000, -3, -1, 0, 1, 2, 77, 4096, 100001):
        x = F(k * leaf)
        steps = [vc.down(vc.down(x)), vc.down(x), x, vc.up(x), vc.up(vc.up(x))]
        pts = F([[s, 0.0, 0.0] for s in steps])
        ijk, _, _ = _host_equals_restatement(pts, leaf, "boundary %d" % k)
        assert ijk[:, 0].tolist() == [k - 1, k - 1, k, k, k], (k, ijk[:, 0])
        for a in (1, 2):                                     # the same on the other axes
            q = np.zeros((5, 3), F)
            q[:, a] = steps
            assert _host_equals_restatement(q, leaf)[0][:, a].tolist() == [k - 1, k - 1, k, k, k]


@pytest.mark.parametrize("leaf", [0.3, 0.1])
def test_rounded_inverse_leaves_follow_the_float32_product(leaf):
    """1 / leaf is rounded: the cell is floorf of the float32 product, whatever the real quotient says."""
    inv = F(1.0) / F(leaf)
    rs = np.random.RandomState(4)
    differs = 0
    for k in list(range(-50, 50)) + rs.randint(-10**5, 10**5, 300).tolist():
        x = F(k * float(F(leaf)))
        steps = F([vc.down(x), x, vc.up(x)])
        pts = np.zeros((3, 3), F)
        pts[:, 1] = steps
        ijk, _, _ = _host_equals_restatement(pts, leaf, "rounded %d" % k)
        assert ijk[:, 1].tolist() == [int(np.floor(s * inv)) for s in steps]
        differs += int(ijk[1, 1] != int(np.floor(float(x) / float(F(leaf)))))
    assert differs > 0                                       # (the cases were worth having: somewhere the product and the quotient disagree)


def test_the_edge_of_the_lattice():
    from fast_limo_amd import api
    leaf = 0.5
    edge = F(vc.HALF * leaf)                                 # the cell 2^20 begins here: outside
    for a in range(3):
        for sign in (1.0, -1.0):
            pts = np.zeros((4, 3), F)
            pts[:, a] = F(sign) * F([vc.down(vc.down(edge)), vc.down(edge), edge, vc.up(edge)])
            ijk, key, inside = _host_equals_restatement(pts, leaf, "edge")
            if sign > 0:
                assert inside.tolist() == [True, True, False, False] and ijk[1, a] == vc.HALF - 1
            else:                                            # floor: everything below -(2^20 - 1) cells lies in cell -2^20 or beyond
                assert inside.tolist() == [False, False, False, False]
            assert np.all(key[~inside] == np.uint64(vc.OUTSIDE_KEY)) and np.all(ijk[~inside] == 0)
        low = F(-(vc.HALF - 1) * leaf)                       # the cell -(2^20 - 1) begins here: the lowest one inside
        pts = np.zeros((3, 3), F)
        pts[:, a] = [vc.down(low), low, vc.up(low)]
        ijk, key, inside = _host_equals_restatement(pts, leaf, "low edge")
        assert inside.tolist() == [False, True, True] and ijk[1:, a].tolist() == [-vc.HALF + 1] * 2
    # the largest key of the lattice is below all ones
    inside, ijk, key = api.voxel_key_host([float(vc.down(edge))] * 3, leaf)
    assert inside and ijk.tolist() == [vc.HALF - 1] * 3 and key == (1 << 63) - 1 and key < vc.OUTSIDE_KEY
    inside, ijk, key = api.voxel_key_host([-(vc.HALF - 1) * leaf] * 3, leaf)
    assert inside and ijk.tolist() == [-vc.HALF + 1] * 3 and key == (1 << 42) | (1 << 21) | 1
    # non-finite coordinates never reach the map; the host function still calls them outside
    for bad in (np.nan, np.inf, -np.inf, 3e38):
        inside, ijk, key = api.voxel_key_host((0.0, bad, 0.0), 0.001)
        assert not inside and ijk.tolist() == [0, 0, 0] and key == vc.OUTSIDE_KEY


def test_the_host_function_rejects_a_bad_leaf_and_a_null_point():
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    p = F([1.0, 2.0, 3.0])
    ijk, key = np.full(3, 7, np.int32), C.c_uint64(7)
    for bad in vc.BAD_CFGS:
        if "leaf" in bad:
            assert L.flimo_voxel_key_host(p.ctypes.data, bad["leaf"], ijk.ctypes.data, C.byref(key)) == ERR_INVALID, bad
    assert L.flimo_voxel_key_host(None, 0.5, ijk.ctypes.data, C.byref(key)) == ERR_INVALID
    assert np.all(ijk == 7) and key.value == 7
    assert L.flimo_voxel_key_host(p.ctypes.data, 0.5, None, None) == 0      # the outputs may be NULL


# ---- the sum's shape -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 128, 129, 4097])
def test_the_sums_restatement_equals_the_shape_in_plain_python_floats(c):
    rs = np.random.RandomState(c)
    u = rs.normal(0, 1, c) * 10.0 ** rs.uniform(-6, 6, c)
    got, want = vc.sum_shape(u), vc.sum_shape_plain(u)
    assert D(got).tobytes() == D(want).tobytes(), (c, got, want)
    assert D(vc.sum_shape_butterfly(u)).tobytes() == D(want).tobytes()
    if c > 64:                                               # the shape matters: it is not the running sum
        assert abs(got - float(np.sum(u))) <= 1e-9 * np.abs(u).sum()
    # all (-0.0): the leading +0.0 fixes the sign
    z = np.full(c, -0.0)
    for s in (vc.sum_shape(z), vc.sum_shape_plain(z), vc.sum_shape_butterfly(z)):
        assert s == 0.0 and not np.signbit(s)
    # many voxels at once equal the voxels one by one
    cuts = sorted(set([0, c // 3, c // 2, c]))
    start, count = np.array(cuts[:-1]), np.diff(cuts)
    keep = count > 0
    many = vc.sum_shape(u, start[keep], count[keep])
    np.testing.assert_array_equal(vc.bits(many), vc.bits([vc.sum_shape_plain(u[s:s + n]) for s, n in zip(start[keep], count[keep])]))


def test_a_small_group_gives_the_bits_of_the_full_tree():
    """Eight or sixteen lanes serve a voxel of at most that many points with the tree over their own slots; the upper levels of the
    64-slot tree would only add +0.0."""
    rs = np.random.RandomState(7)
    for c in range(1, 17):
        for trial in range(20):
            u = (rs.normal(0, 1, c) * 10.0 ** rs.uniform(-3, 3, c)).tolist()
            if trial == 0:
                u = [-0.0] * c
            for G in (8, 16):
                if c > G:
                    continue
                t = u + [0.0] * (G - c)
                while len(t) > 1:
                    t = [t[i] + t[i + 1] for i in range(0, len(t), 2)]
                assert D(0.0 + t[0]).tobytes() == D(vc.sum_shape_plain(u)).tobytes()


# ---- grouping and selection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", vc.SCENE_LEAVES)
def test_grouping_equals_numpy_unique(leaf):
    pts = vc.scene()
    g = vc.group(pts, leaf)
    c, inside = vc.cells(pts, leaf)
    assert inside.all()
    uniq, inv, cnt = np.unique(c.astype(np.int64)[:, ::-1], axis=0, return_inverse=True, return_counts=True)      # rows (cz, cy, cx), ascending
    np.testing.assert_array_equal(g["ijk"], uniq[:, ::-1])
    np.testing.assert_array_equal(g["count"], cnt)
    voxel = np.empty(len(pts), np.int64)
    voxel[g["order"]] = g["vid"]
    np.testing.assert_array_equal(voxel, inv.reshape(-1))
    for s, n in zip(g["start"][:50], g["count"][:50]):      # members in ascending insertion index
        assert np.all(np.diff(g["order"][s:s + n]) > 0)
    r = vc.restate(pts, leaf=leaf)
    np.testing.assert_array_equal(r["first"], [np.flatnonzero(inv.reshape(-1) == v)[0] for v in range(len(uniq))])
    if leaf == 1.0:
        cen, cov, near = vc.restate_plain(pts, leaf)
        np.testing.assert_array_equal(vc.bits(r["centroid"]), vc.bits(cen))
        np.testing.assert_array_equal(vc.bits(r["cov"]), vc.bits(cov))
        np.testing.assert_array_equal(r["nearest"], near)
        assert r["stats"]["largest"] > 64                   # (voxels of several runs are among them)


@pytest.mark.parametrize("cfg", [dict(keep=vc.KEEP_FIRST, max_pts=1), dict(keep=vc.KEEP_FIRST, max_pts=3), dict(keep=vc.KEEP_NEAREST, max_pts=1)])
def test_both_rules_are_idempotent_on_the_restatement(cfg):
    for pts, leaf in ((vc.scene(), 0.25), (vc.duplicates(), 0.5), (vc.hand_voxels()[0], 0.5)):
        r = vc.restate(pts, leaf=leaf, **cfg)
        assert r["stats"]["sel_points"] > 0
        kept = np.asarray(pts)[~r["mask"]]
        r2 = vc.restate(kept, leaf=leaf, **cfg)
        assert r2["stats"]["sel_points"] == 0 and r2["stats"]["voxels"] == r["stats"]["voxels"]
        assert r2["stats"]["largest"] <= cfg["max_pts"]
        np.testing.assert_array_equal(r2["ijk"], r["ijk"])
        if cfg["keep"] == vc.KEEP_FIRST:                     # the oldest m of every voxel stay
            np.testing.assert_array_equal(r2["count"], np.minimum(r["count"], cfg["max_pts"]))
        else:                                                # the kept point is its voxel's rep, and a voxel of one point is its own centroid
            np.testing.assert_array_equal(kept, np.asarray(pts)[np.sort(r["rep"])])


def test_the_dyadic_lattice_by_hand():
    r = vc.restate(vc.dyadic_lattice(), leaf=1.0, keep=vc.KEEP_NEAREST)
    assert r["ijk"].tolist() == [[0, 0, 0], [1, 0, 0]] and r["count"].tolist() == [8, 4]
    assert r["centroid"].tolist() == [[0.5, 0.5, 0.5], [1.4375, 0.4375, 0.5]]
    assert r["cov"].tolist() == [[0.0625, 0.0, 0.0, 0.0625, 0.0, 0.0625], [0.04296875, -0.01953125, 0.0, 0.04296875, 0.0, 0.0]]
    assert r["rep"].tolist() == [0, 11]                      # eight equidistant members: the smallest index; the point nearest the centroid
    assert len(set(r["q"][:8].tolist())) == 1
