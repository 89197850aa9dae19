"""RANSAC planes of the stored points (flimo_map_planes) as far as they can be checked without a GPU: both libraries export and declare
the new entry points, the calls reject a null context, flimo_plane_solve_host -- the function the solve kernel calls -- equals the
restatement of the definition (tests/planes_common.py) bit for bit on random, hand-worked, degenerate and far-away triangles and one
float32 step either side of every threshold, the numpy form of the sum's shape equals the shape written in plain Python floats, and
the recovery bars the GPU test asserts hold for the restatement first.  The kernels run on the GPU: tests/test_gpu_planes.py."""
import ctypes as C
import os

import numpy as np
import pytest

import planes_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
F = np.float32
D = np.float64

HIP_NAMES = ("flimo_map_planes", "flimo_plane_solve_host", "flimo_map_plane_mask", "flimo_map_remove_plane", "flimo_set_plane_chunk")
HOST_NAMES = ("flimo_loc_map_planes", "flimo_loc_map_plane_mask", "flimo_loc_map_remove_plane")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in HIP_NAMES:
        getattr(L, name)
    for name in HOST_NAMES:
        getattr(H, name)
    api.plane_consensus, api.plane_solve_host


def test_new_entry_points_are_exported_and_declared():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    dev = open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in HIP_NAMES:
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS, name
    assert "int flimo_map_planes(flimo_ctx* ctx, const int32_t* tri /* [nh][3] insertion indices */, size_t nh, const flimo_plane_cfg* cfg," in pub
    assert "int flimo_plane_solve_host(const float p3[9], const flimo_plane_cfg* cfg, double plane4[4], float nf[3]);" in pub
    assert "int flimo_map_plane_mask(flimo_ctx* ctx, size_t first, size_t n, const flimo_plane_sel* sel," in pub
    assert "int flimo_map_remove_plane(flimo_ctx* ctx, size_t first, size_t n, const flimo_plane_sel* sel, size_t* removed);" in pub
    assert "} flimo_plane_cfg;" in pub and "} flimo_plane_sel;" in pub and "tests/planes_common.py" in pub
    for text in ("#define FLIMO_PLANE_OK 0", "#define FLIMO_PLANE_DEGENERATE 1", "#define FLIMO_PLANE_REJECTED 2", "#define FLIMO_PLANE_SLAB 8192"):
        assert text in pub, text
    assert "flimo_set_plane_chunk(" in dev
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for name in ("map_planes", "map_plane_mask", "map_remove_plane", "set_plane_chunk"):
        assert hasattr(_lib.HipCtx, name), name
    for name in ("map_planes", "map_plane_mask", "map_remove_plane"):
        assert hasattr(api.Localizer, name), name
    assert (_lib.PLANE_OK, _lib.PLANE_DEGENERATE, _lib.PLANE_REJECTED, _lib.PLANE_SLAB) == (pc.OK, pc.DEGENERATE, pc.REJECTED, pc.SLAB)
    # the structs as the header lays them out, and the wrapper's defaults as the restatement's
    assert C.sizeof(_lib.PlaneCfg) == 28 and C.sizeof(_lib.PlaneSel) == 32
    assert [f[0] for f in _lib.PlaneCfg._fields_] == ["dist", "min_edge", "min_sin", "axis", "min_cos"]
    assert [f[0] for f in _lib.PlaneSel._fields_] == ["normal", "anchor", "dist", "side"]
    k = _lib.plane_cfg()
    for name, v in pc.DEFAULTS.items():
        got = getattr(k, name)
        assert (list(got) == [float(F(x)) for x in v]) if name == "axis" else (float(got) == float(F(v))), name
    k = _lib.plane_cfg(dist=0.3, axis=(1, 2, 3), min_cos=0.5)
    assert (k.dist, list(k.axis), k.min_cos, k.min_edge) == (float(F(0.3)), [1.0, 2.0, 3.0], 0.5, 0.0)
    s = _lib.plane_sel((0, 0, 1), (1, 2, 3), 0.25, -1)
    assert (list(s.normal), list(s.anchor), s.dist, s.side) == ([0.0, 0.0, 1.0], [1.0, 2.0, 3.0], 0.25, -1)


def test_the_calls_reject_a_null_context_and_leave_their_outputs():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k, s = _lib.plane_cfg(), _lib.plane_sel((0, 0, 1), (0, 0, 0))
    tri = np.array([[0, 1, 2]], np.int32)
    status, inliers, ssq, plane = np.full(1, 7, np.int32), np.full(1, 7, np.int32), np.full(1, 7.0), np.full(4, 7.0)
    mask, count, removed = np.full(2, 7, np.uint8), C.c_size_t(7), C.c_size_t(7)
    args = (tri.ctypes.data, 1, C.byref(k), status.ctypes.data, inliers.ctypes.data, ssq.ctypes.data, plane.ctypes.data)
    assert L.flimo_map_planes(None, *args) == ERR_INVALID
    assert H.flimo_loc_map_planes(None, *args) == ERR_INVALID
    assert L.flimo_map_plane_mask(None, 0, 2, C.byref(s), mask.ctypes.data, C.byref(count)) == ERR_INVALID
    assert H.flimo_loc_map_plane_mask(None, 0, 2, C.byref(s), mask.ctypes.data, C.byref(count)) == ERR_INVALID
    assert L.flimo_map_remove_plane(None, 0, 2, C.byref(s), C.byref(removed)) == ERR_INVALID
    assert H.flimo_loc_map_remove_plane(None, 0, 2, C.byref(s), C.byref(removed)) == ERR_INVALID
    assert L.flimo_set_plane_chunk(None, 5) == ERR_INVALID
    assert np.all(status == 7) and np.all(inliers == 7) and np.all(ssq == 7) and np.all(plane == 7) and np.all(mask == 7)
    assert count.value == 7 and removed.value == 7


# ---- flimo_plane_solve_host against the restatement -----------------------------------------------------------------------------------
def _host_equals_restatement(p3, what="", **cfg):
    from fast_limo_amd import api
    kw = {k: v for k, v in pc.cfg_of(**cfg).items()}
    st, plane, nf = api.plane_solve_host(p3, **kw)
    wst, wplane, wnf = pc.solve(p3, **kw)
    assert st == wst, (what, st, wst)
    if st == pc.OK:
        assert plane.tobytes() == wplane.tobytes() and nf.tobytes() == wnf.tobytes(), (what, plane, wplane, nf, wnf)
        assert abs(pc.sq(*plane[:3]) - 1.0) < 1e-14
    else:
        assert np.all(np.isnan(plane)) and np.all(np.isnan(nf)), what
    return st, plane, nf


def test_random_triangles_bit_for_bit():
    rs = np.random.RandomState(3)
    seen = set()
    for i in range(600):
        scale = 10.0 ** rs.uniform(-2, 3)
        p3 = (rs.uniform(-1, 1, (3, 3)) * scale + rs.uniform(-50, 50, 3)).astype(F)
        cfg = dict(min_edge=0.3 * scale * (i % 3 == 0), min_sin=0.3 * (i % 2), axis=rs.normal(0, 1, 3), min_cos=0.5 * (i % 5 < 2))
        st, plane, nf = _host_equals_restatement(p3, "random %d" % i, **cfg)
        seen.add(st)
        if st == pc.OK:                                      # the three points lie on their plane, the sign rule holds
            k = int(np.argmax(np.abs(plane[:3])))
            assert plane[k] > 0
            assert np.all(np.abs(p3.astype(D) @ plane[:3] + plane[3]) < 1e-9 * max(1.0, np.abs(p3).max()))
    assert seen == {pc.OK, pc.DEGENERATE, pc.REJECTED}


def test_a_lattice_triangle_worked_by_hand_and_its_swap():
    a, b, c = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    st, plane, nf = _host_equals_restatement(F([a, b, c]), "hand")
    assert st == pc.OK and plane.tolist() == [0.0, 0.0, 1.0, 0.0] and nf.tolist() == [0.0, 0.0, 1.0]
    assert not np.signbit(plane[:3]).any()
    st2, plane2, nf2 = _host_equals_restatement(F([a, c, b]), "hand swapped")      # e2 x e1 = -(e1 x e2): the sign rule undoes it
    assert st2 == pc.OK and plane2[2] == 1.0 and plane2[3] == 0.0 and nf2[2] == 1.0
    # a general triangle: swapping b and c negates the cross product exactly, so every bit of the result is the same
    rs = np.random.RandomState(8)
    for i in range(50):
        p = rs.uniform(-20, 20, (3, 3)).astype(F)
        _, p1, n1 = _host_equals_restatement(p, "swap %d" % i)
        _, p2, n2 = _host_equals_restatement(p[[0, 2, 1]], "swap %d'" % i)
        assert p1.tobytes() == p2.tobytes() and n1.tobytes() == n2.tobytes()
    # equal magnitudes: the lowest axis decides
    st, plane, _ = _host_equals_restatement(F([(0, 0, 0), (1, -1, 0), (0, -1, 1)]), "tie")      # cr = (-1, -1, -1)
    assert st == pc.OK and np.all(plane[:3] > 0) and plane[0] == plane[1] == plane[2]
    st, plane, _ = _host_equals_restatement(F([(0, 0, 0), (1, 1, 0), (0, 1, 1)]), "tie 2")       # cr = (1, -1, 1)
    assert st == pc.OK and plane[0] > 0 and plane[1] < 0 and plane[2] > 0


def test_collinear_repeated_and_far_away_points():
    deg = lambda p, **cfg: _host_equals_restatement(F(p), str(p), **cfg)[0]
    assert deg([(0, 0, 0), (1, 1, 1), (3, 3, 3)]) == pc.DEGENERATE               # collinear on the lattice: q == 0
    assert deg([(1, 2, 3), (1, 2, 3), (4, 5, 6)]) == pc.DEGENERATE               # a repeated point passes min_edge 0 and fails q > 0
    assert deg([(1, 2, 3), (4, 5, 6), (4, 5, 6)]) == pc.DEGENERATE
    assert deg([(1, 2, 3)] * 3) == pc.DEGENERATE
    assert deg([(np.nan, 0, 0), (1, 0, 0), (0, 1, 0)]) == pc.DEGENERATE
    assert deg([(np.inf, 0, 0), (1, 0, 0), (0, 1, 0)]) == pc.DEGENERATE
    assert deg([(0, 0, 0), (3e38, 0, 0), (0, 3e38, 0)]) == pc.OK                 # float64 holds the squares
    # 1 000 km from the origin: the float32 points are what they are, the float64 solve sees them exactly
    base = F([1.0e6, -1.0e6, 1.0e6])
    tri = F([(0, 0, 0), (1, 0, 0), (0, 1, 0)]) + base
    st, plane, nf = _host_equals_restatement(tri, "far")
    assert st == pc.OK and plane[:3].tolist() == [0.0, 0.0, 1.0] and plane[3] == -1.0e6
    rs = np.random.RandomState(5)
    for i in range(50):
        _host_equals_restatement((rs.uniform(-2, 2, (3, 3)) + base.astype(D)).astype(F), "far %d" % i, min_sin=0.1)


def _either_side(p3, field, value, worse_is_up, **cfg):
    """field one float32 step either side of the triangle's own value (float64 ``value``): OK on the lenient side, not on the other,
    and the host function equals the restatement at each of the five steps around it."""
    f = F(value)
    steps = [pc.down(pc.down(f)), pc.down(f), f, pc.up(f), pc.up(pc.up(f))]
    got = [_host_equals_restatement(p3, "%s %r" % (field, float(v)), **dict(cfg, **{field: float(v)}))[0] for v in steps]
    bad = pc.REJECTED if field == "min_cos" else pc.DEGENERATE
    lenient, strict = (got[:2], got[3:]) if worse_is_up else (got[3:], got[:2])
    assert lenient[0 if worse_is_up else 1] == pc.OK and strict[1 if worse_is_up else 0] == bad, (field, got)
    assert got == sorted(got) if worse_is_up else got == sorted(got, reverse=True), (field, got)      # one switch, no return
    return got


def test_each_threshold_one_float32_step_either_side():
    rs = np.random.RandomState(12)
    for i in range(20):
        p3 = rs.uniform(-3, 3, (3, 3)).astype(F)
        p = p3.astype(D)
        e1, e2, e3 = p[1] - p[0], p[2] - p[0], p[2] - p[1]
        shortest = np.sqrt(min(pc.sq(*e1), pc.sq(*e2), pc.sq(*e3)))
        cr = np.cross(e1, e2)
        sine = np.sqrt(pc.sq(*cr) / (pc.sq(*e1) * pc.sq(*e2)))
        n = cr / np.sqrt(pc.sq(*cr))
        axis = F([0.3, -0.5, 2.0])                                               # not a unit vector: used as given
        cosine = abs(float(n @ axis.astype(D)))
        _either_side(p3, "min_edge", shortest, True)
        _either_side(p3, "min_sin", sine, True)
        if cosine <= 1.0:
            _either_side(p3, "min_cos", cosine, True, axis=axis)
    # exact cases: an edge of exactly 0.5 m passes min_edge 0.5 (>=); a right angle passes min_sin 1; a unit axis along n passes 1
    tri = F([(0, 0, 0), (0.5, 0, 0), (0, 2, 0)])
    assert _host_equals_restatement(tri, min_edge=0.5)[0] == pc.OK
    assert _host_equals_restatement(tri, min_edge=float(pc.up(0.5)))[0] == pc.DEGENERATE
    assert _host_equals_restatement(tri, min_sin=1.0)[0] == pc.OK
    assert _host_equals_restatement(tri, min_cos=1.0, axis=(0, 0, 1))[0] == pc.OK
    assert _host_equals_restatement(tri, min_cos=1.0, axis=(0, 0, -1))[0] == pc.OK           # |n . axis|
    assert _host_equals_restatement(tri, min_cos=1.0, axis=(0, 0, float(pc.down(1.0))))[0] == pc.REJECTED


def test_the_axis_is_used_as_given_not_normalised():
    tri = F([(0, 0, 0), (1, 0, 0), (0, 1, 0.25)])                                # n = (0, -0.25, 1) / sqrt(1.0625)
    cos = 1.0 / np.sqrt(1.0625)
    assert _host_equals_restatement(tri, min_cos=0.99, axis=(0, 0, 1))[0] == pc.REJECTED and cos < 0.99
    assert _host_equals_restatement(tri, min_cos=0.99, axis=(0, 0, 2))[0] == pc.OK            # a longer axis passes: not normalised
    assert _host_equals_restatement(tri, min_cos=0.4, axis=(0, 0, 0.5))[0] == pc.OK
    assert _host_equals_restatement(tri, min_cos=0.5, axis=(0, 0, 0.5))[0] == pc.REJECTED
    assert _host_equals_restatement(tri, min_cos=0.0, axis=(np.nan, 0, 0))[0] == pc.OK        # not read at min_cos 0
    assert _host_equals_restatement(tri, min_cos=0.1, axis=(0, 0, 0))[0] == pc.REJECTED


def test_the_host_function_rejects_every_bad_cfg_and_null_argument():
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    tri = F([(0, 0, 0), (1, 0, 0), (0, 1, 0)]).reshape(9)
    plane, nf = np.full(4, 7.0), np.full(3, 7, F)
    for bad in pc.BAD_CFGS:
        k = _lib.plane_cfg(**pc.cfg_of(**bad))
        assert L.flimo_plane_solve_host(tri.ctypes.data, C.byref(k), plane.ctypes.data, nf.ctypes.data) == ERR_INVALID, bad
    k = _lib.plane_cfg()
    assert L.flimo_plane_solve_host(None, C.byref(k), plane.ctypes.data, nf.ctypes.data) == ERR_INVALID
    assert L.flimo_plane_solve_host(tri.ctypes.data, None, plane.ctypes.data, nf.ctypes.data) == ERR_INVALID
    assert L.flimo_plane_solve_host(tri.ctypes.data, C.byref(k), None, nf.ctypes.data) == ERR_INVALID
    assert L.flimo_plane_solve_host(tri.ctypes.data, C.byref(k), plane.ctypes.data, None) == ERR_INVALID
    assert np.all(plane == 7) and np.all(nf == 7)
    k = _lib.plane_cfg(dist=float("inf"), min_sin=1.0, min_cos=1.0)              # the ends of the ranges are valid
    assert L.flimo_plane_solve_host(tri.ctypes.data, C.byref(k), plane.ctypes.data, nf.ctypes.data) == pc.OK


# ---- the sum's shape -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 8191, 8192, 8193, 16385])
def test_the_sums_restatement_equals_the_shape_in_plain_python_floats(N):
    rs = np.random.RandomState(N)
    t = (rs.normal(0, 0.04, N) * 10.0 ** rs.uniform(-3, 0, N)).astype(F)
    inside = np.abs(t) < F(0.03)
    assert 0 < inside.sum() <= N
    tt = np.where(inside, t.astype(D) * t.astype(D), 0.0)
    got, want = pc.sum_shape(tt), pc.sum_shape_plain(t, inside)
    assert D(got).tobytes() == D(want).tobytes(), (N, got, want)
    if N > 4 * pc.RED:                                                             # the shape matters: a plain running sum differs
        assert abs(got - float(np.sum(tt))) <= 1e-12 * got
    # a batch of rows through the numpy form equals the rows one by one
    rows = np.stack([tt, tt[::-1], np.zeros(N)])
    np.testing.assert_array_equal(pc.bits(pc.sum_shape(rows)), pc.bits([pc.sum_shape(r) for r in rows]))
    assert pc.sum_shape(np.zeros(N)) == 0.0 and not np.signbit(pc.sum_shape(np.zeros(N)))


# ---- recovery, restatement only: the bars tests/test_gpu_planes.py asserts ------------------------------------------------------------
def test_hand_made_hypotheses_on_the_scene_get_the_status_the_hand_says():
    pts = pc.scene()
    hand = pc.hand_triplets(pts)
    r = pc.restate(pts, [t for _, t, _ in hand], **pc.REC_CFG)
    for (name, tri, want), st in zip(hand, r["status"]):
        assert st == want, (name, tri, st)
    assert r["inliers"][0] >= 1500 and r["plane"][0].tobytes() == r["plane"][1].tobytes() and r["sum_sq"][0] == r["sum_sq"][1]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_floor_is_recovered_and_the_clusters_fall_apart(seed):
    import clusters_common as cc
    from fast_limo_amd import api
    pts = pc.scene()
    if seed == 0:
        before = np.sort(np.bincount(cc.labels(pts, pc.REC_TOL)))[::-1]
        assert before[0] == 5060                                                   # floor, wall and cylinder are one component
    tri = api.corr_triplets(len(pts), pc.REC_NH, seed)
    r = pc.restate(pts, tri, **pc.REC_CFG)
    best = pc.rank(r)[0]
    print("seed", seed, "survivors", int((r["status"] == pc.OK).sum()), "inliers", int(r["inliers"][best]), "plane", r["plane"][best])
    assert r["inliers"][best] >= 1500 and abs(r["plane"][best, 2]) >= 0.9999
    mask = pc.mask_restate(pts, r["plane"][best, :3].astype(F), pts[tri[best, 0]], pc.REC_REMOVE_DIST)
    print("removed", int(mask.sum()))
    assert 1595 <= mask.sum() <= 1605
    after = np.sort(np.bincount(cc.labels(pts[~mask], pc.REC_TOL)))[::-1]
    assert after[0] == 1860 and after[1] == 1600, after[:4]
    # the cross property on the restatement: the mask at the hypothesis's own gate counts its inliers
    assert pc.mask_restate(pts, r["plane"][best, :3].astype(F), pts[tri[best, 0]], pc.REC_CFG["dist"]).sum() == r["inliers"][best]
