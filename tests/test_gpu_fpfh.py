"""GPU suite: FPFH descriptors of the stored points -- flimo_map_fpfh forms the normals of the whole map, the integer SPFH rows of the
whole map and the weighted, normalised rows of a range, all on the device.  The yardstick is the definition restated in numpy
(tests/fpfh_common.py), fed with the normals and the neighbour lists the same context returns (normals_range, knn_k): the list
lengths, the integer rows and the bits of every float32 of a row are compared exactly on every point the restatement does not mark
as tainted (a pair whose theta lies within 1e-9 of a bin's edge, in the point's own row or in a neighbour's: atan2 is the one
operation numpy cannot pin; tests/test_fpfh_host.py holds the tainted share of every cloud used here to 0.5 %).  A tainted point's
integer row may differ only by one count per ambiguous pair moved to a neighbouring theta bin, and given the device's integer rows the
sums are compared bit for bit on EVERY point.  Chunking, cell size, range form and repetition move no bit at all."""
import ctypes as C

import numpy as np
import pytest

import fpfh_common as fc
from common import CAPS

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -2, -6
INF = float("inf")
F = np.float32


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_map_fpfh", "flimo_set_fpfh_chunk"):
        getattr(L, name)
    getattr(H, "flimo_loc_map_fpfh")


def _ctx(pts, cell=0.0, downsample=True):
    """The whole cloud as the first add: the first build neither drops points nor merges duplicates."""
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, downsample, cell)
    ctx.map_add(pts, stamp=0.5)
    assert ctx.map_size() == len(pts)
    np.testing.assert_array_equal(ctx.map_points(), pts)
    return ctx


@pytest.fixture(scope="module")
def scene_ctx(built):
    ctx = _ctx(fc.scene())
    yield ctx
    ctx.close()


def _restated(ctx, cfg, spfh_rows=None):
    """The restatement fed with this context's own normals and lists."""
    pts = ctx.map_points()
    n = len(pts)
    nrm = ctx.normals_range(0, n, cfg["normal_k"], cfg.get("normal_max_dist", INF), cfg.get("normal_min_pts", 3), cfg.get("viewpoint"), want=())["normal"]
    idx, sqd, cnt = ctx.knn_k(pts, cfg["k"], cfg.get("max_dist", INF))
    return fc.restate(pts, nrm, idx, sqd, cnt, spfh_rows=spfh_rows), nrm


def _same_as_restatement(ctx, cfg, what):
    """cnt, spfh and the bits of fpfh equal the restatement on every untainted point; a tainted point's integer row differs at most by
    its ambiguous pairs' moves; from the device's integer rows the sums are the restatement's on every point.  Returns (out, r)."""
    out = ctx.map_fpfh(**cfg)
    r, _ = _restated(ctx, cfg)
    t = r["tainted"]
    differ = (out["spfh"] != r["spfh"]).any(1)
    fbad = (fc.bits(out["fpfh"]) != fc.bits(r["fpfh"])).any(1)
    print(what, "points", len(t), "ambiguous pairs", int(r["pair_amb"].sum()), "tainted", int(t.sum()), "spfh rows that differ", int(differ.sum()),
          "of them untainted", int((differ & ~t).sum()), "fpfh rows that differ", int(fbad.sum()), "of them untainted", int((fbad & ~t).sum()))
    assert out["fpfh"].dtype == F and out["spfh"].dtype == np.uint8 and out["cnt"].dtype == np.int32
    assert float(t.mean()) <= fc.MAX_TAINTED, what
    np.testing.assert_array_equal(out["cnt"], r["cnt"], err_msg=what)
    bad = np.nonzero(differ & ~t)[0]
    assert len(bad) == 0, (what, "spfh", bad[:5], out["spfh"][bad[:2]], r["spfh"][bad[:2]])
    bad = np.nonzero(fbad & ~t)[0]
    assert len(bad) == 0, (what, "fpfh", bad[:5], out["fpfh"][bad[:2]], r["fpfh"][bad[:2]])
    for j in np.nonzero(t)[0]:
        assert fc.moved_by_ambiguous_pairs(out["spfh"][j], r["spfh"][j], r["pair_h1"][j][r["pair_amb"][j]].tolist()), (what, j)
    again, _ = _restated(ctx, cfg, spfh_rows=out["spfh"]) if differ.any() else (r, None)
    bad = np.nonzero((fc.bits(out["fpfh"]) != fc.bits(again["fpfh"])).any(1))[0]
    assert len(bad) == 0, (what, "fpfh from the device's rows", bad[:5])
    assert out["spfh"].any() and out["fpfh"].any(), what
    return out, r


def _same_bits(a, b, what):
    for key in ("fpfh", "spfh", "cnt"):
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (what, key)


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["scene-k10", "scene-k33"])
def test_rows_equal_the_restatement(scene_ctx, case):
    cfg = fc.CASES[case][1]
    out, r = _same_as_restatement(scene_ctx, cfg, case)
    # every non-empty group of a row sums to 100
    sums = out["fpfh"].astype(np.float64).reshape(-1, 3, fc.BINS).sum(2)
    live = r["group_sum"] != 0.0
    assert live.all() and np.all(np.abs(sums - 100.0) <= 33 * 2.0 ** -23 * 100.0)


# ---- 2. the walk over the tiles ---------------------------------------------------------------------------------------------------------
def test_lists_that_cross_300_m_take_the_walk_and_are_exact(built):
    pts = fc.two_clusters()
    ctx = _ctx(pts)
    try:
        for case in ("clusters-k64", "clusters-k64-gate"):
            out, r = _same_as_restatement(ctx, fc.CASES[case][1], case)
            assert not r["tainted"].any()
            assert np.all(out["cnt"] == (64 if case == "clusters-k64" else 40))
        idx, _, _ = ctx.knn_k(pts, 64)
        assert np.all((idx[:40] >= 40).sum(1) == 24) and np.all((idx[40:] < 40).sum(1) == 24)      # every list crosses over
    finally:
        ctx.close()


# ---- 3. nothing moves the bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 33])
def test_bits_do_not_depend_on_the_chunk_the_cell_size_the_range_or_the_call(scene_ctx, k):
    cfg = dict(k=k, normal_k=10)
    whole = scene_ctx.map_fpfh(**cfg)
    _same_bits(scene_ctx.map_fpfh(**cfg), whole, "twice")
    scene_ctx.set_fpfh_chunk(257)
    try:
        _same_bits(scene_ctx.map_fpfh(**cfg), whole, "chunk 257")
        first, n = 1000, 700                                          # neither a multiple of the chunk
        part = scene_ctx.map_fpfh(first, n, **cfg)
        _same_bits(part, {key: whole[key][first:first + n] for key in whole}, "range, chunk 257")
    finally:
        scene_ctx.set_fpfh_chunk(0)
    _same_bits(scene_ctx.map_fpfh(1000, 700, **cfg), {key: whole[key][1000:1700] for key in whole}, "range")
    only = scene_ctx.map_fpfh(4000, None, want=(), **cfg)
    assert sorted(only) == ["fpfh"] and only["fpfh"].tobytes() == whole["fpfh"][4000:].tobytes()
    for cell in (0.5, 1.3):
        ctx = _ctx(fc.scene(), cell=cell)
        try:
            _same_bits(ctx.map_fpfh(**cfg), whole, "cell %g" % cell)
        finally:
            ctx.close()


# ---- 4. translation ---------------------------------------------------------------------------------------------------------------------
def test_a_translation_on_the_lattice_moves_no_bit(built):
    base = fc.scene(lattice=True)
    cfg = fc.CASES["lattice-k10"][1]
    a, b = _ctx(base), _ctx(fc.shifted(base))
    try:
        oa, ob = a.map_fpfh(**cfg), b.map_fpfh(**cfg)
        _same_bits(oa, ob, "shifted")
        _same_as_restatement(a, cfg, "lattice-k10")
    finally:
        a.close(); b.close()


# ---- 5. degenerate inputs ---------------------------------------------------------------------------------------------------------------
def test_a_list_of_exact_duplicates_gives_a_row_of_zeros(built):
    ctx = _ctx(fc.duplicate_scene(), downsample=False)
    try:
        cfg = fc.CASES["duplicates"][1]
        out, r = _same_as_restatement(ctx, cfg, "duplicates")
        assert np.all(out["cnt"][-4:] == 3) and not out["spfh"][-4:].any() and not out["fpfh"][-4:].any()
        assert fc.bits(out["fpfh"][-4:]).max() == 0                   # +0.0
    finally:
        ctx.close()


def test_a_point_without_a_plane_has_no_pairs_but_a_row_from_its_neighbours(built):
    pts = fc.sparse_scene()
    cfg = fc.CASES["sparse-normal"][1]
    ctx = _ctx(pts)
    try:
        out, r = _same_as_restatement(ctx, cfg, "sparse-normal")
        _, nrm = _restated(ctx, cfg)
        j = len(pts) - 1
        assert np.isnan(nrm[j, :3]).all() and not np.isnan(nrm[:j, :3]).any()
        assert not out["spfh"][j].any() and out["cnt"][j] == 10 and out["fpfh"][j].any()
        idx, _, _ = ctx.knn_k(pts, 10)
        lists_it = np.nonzero((idx == j).any(1))[0]
        lists_it = lists_it[lists_it != j]
        plain = ctx.map_fpfh(**fc.CASES["scene-k10"][1])             # (the normals' gate off: every point has a plane)
        print("points that list the point without a plane:", len(lists_it))
        for i in lists_it:                                            # they skip it: one pair fewer than without the gate
            assert out["spfh"][i, :11].sum() == plain["spfh"][i, :11].sum() - 1
    finally:
        ctx.close()


def test_a_gate_of_zero_gives_rows_of_zeros(scene_ctx):
    out = scene_ctx.map_fpfh(k=10, normal_k=10, max_dist=0.0)
    assert not out["cnt"].any() and not out["spfh"].any() and fc.bits(out["fpfh"]).max() == 0
    assert out["fpfh"].shape == (len(fc.scene()), 33)


def test_a_viewpoint_flips_normals_and_both_forms_equal_the_restatement(scene_ctx):
    cfg = fc.CASES["viewpoint"][1]
    on, _ = _same_as_restatement(scene_ctx, cfg, "viewpoint")
    off = scene_ctx.map_fpfh(**fc.CASES["scene-k10"][1])
    n = len(fc.scene())
    a = scene_ctx.normals_range(0, n, 10, viewpoint=fc.VIEWPOINT, want=())["normal"][:, :3]
    b = scene_ctx.normals_range(0, n, 10, want=())["normal"][:, :3]
    flipped = (a != b).any(1)
    moved = (on["spfh"][:, :11] != off["spfh"][:, :11]).any(1)
    print("normals flipped", int(flipped.sum()), "theta rows moved", int(moved.sum()))
    assert 100 < flipped.sum() < n and moved.sum() > 100
    np.testing.assert_array_equal(on["cnt"], off["cnt"])


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------------
def test_the_call_changes_neither_map_nor_scan_nor_a_later_pass(built):
    """Against a twin context that never makes the call: the pass before and the pass after have the twin's HTH / HTh bits.  (Two
    passes over one resident scan are not bit-equal to each other, call or no call: the second prunes with the first one's bound.)"""
    from fast_limo_amd import _lib
    mp = fc.scene()
    scan = np.ascontiguousarray(mp[::3] + F([0.01, -0.01, 0.005]))
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809

    def run(search):
        h = _ctx(mp)
        try:
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if search:
                assert h.map_fpfh(k=10, normal_k=10)["fpfh"].any()
                h.set_fpfh_chunk(777)
                assert h.map_fpfh(3000, 1000, k=33, normal_k=12, max_dist=1.0, viewpoint=(0, 0, 5))["fpfh"].shape == (1000, 33)
            out.append(h.match_reduce(x, mcfg))
            return out, h.map_size(), h.map_points().copy(), h.scan_get().copy(), h.grid_selfcheck()
        finally:
            h.close()

    (plain, pn, pm, ps, pl), (searched, sn, sm, ss, sl) = run(False), run(True)
    assert pn == sn == len(mp) and pm.tobytes() == sm.tobytes() == mp.tobytes() and ps.tobytes() == ss.tobytes() and pl == sl
    for a, b in zip(plain, searched):
        print("matches of the pass", a[2], b[2])
        assert a[2] == b[2] > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_outputs_are_untouched(scene_ctx):
    from fast_limo_amd import _lib
    L, h = scene_ctx._L, scene_ctx._h
    n = len(fc.scene())
    K = lambda **kw: _lib.fpfh_cfg(**dict(dict(k=10, normal_k=10), **kw))
    nanvp = K(viewpoint=(0.0, np.nan, 1.0))
    quiet = K()
    quiet.viewpoint[1] = np.nan                                       # (a NaN viewpoint that is switched off is not read)
    cases = [("null cfg", None, 0, n, ERR_INVALID), ("range beyond the map", K(), 0, n + 1, ERR_INVALID), ("first beyond the map", K(), n + 1, 0, ERR_INVALID),
             ("first + n wraps", K(), 2, 2 ** 64 - 1, ERR_INVALID), ("nan gate", K(max_dist=np.nan), 0, n, ERR_INVALID),
             ("negative gate", K(max_dist=-1.0), 0, n, ERR_INVALID), ("nan normal gate", K(normal_max_dist=np.nan), 0, n, ERR_INVALID),
             ("negative normal gate", K(normal_max_dist=-0.5), 0, n, ERR_INVALID), ("nan viewpoint", nanvp, 0, n, ERR_INVALID),
             ("normal_min_pts -1", K(normal_min_pts=-1), 0, n, ERR_INVALID), ("k 1", K(k=1), 0, n, ERR_UNSUPPORTED), ("k 65", K(k=65), 0, n, ERR_UNSUPPORTED),
             ("k -3", K(k=-3), 0, n, ERR_UNSUPPORTED), ("normal_k 0", K(normal_k=0), 0, n, ERR_UNSUPPORTED), ("normal_k 65", K(normal_k=65), 0, n, ERR_UNSUPPORTED),
             ("nan gate, n 0", K(max_dist=np.nan), 0, 0, ERR_INVALID), ("k 65, n 0", K(k=65), 5, 0, ERR_UNSUPPORTED)]
    for what, k, first, cnt_n, want in cases:
        kp = None if k is None else C.byref(k)
        fpfh, spfh, cnt = np.full((n + 1, 33), 7, F), np.full((n + 1, 33), 7, np.uint8), np.full(n + 1, 7, np.int32)
        assert L.flimo_map_fpfh(h, first, cnt_n, kp, fpfh.ctypes.data, spfh.ctypes.data, cnt.ctypes.data) == want, what
        assert np.all(fpfh == 7) and np.all(spfh == 7) and np.all(cnt == 7), what
    k = K()
    spfh = np.full((n, 33), 7, np.uint8)
    assert L.flimo_map_fpfh(h, 0, n, C.byref(k), None, spfh.ctypes.data, None) == ERR_INVALID and np.all(spfh == 7)      # fpfh is required
    assert L.flimo_map_fpfh(None, 0, n, C.byref(k), None, None, None) == ERR_INVALID
    # n == 0: nothing touched, fpfh may be NULL
    fpfh = np.full((4, 33), 7, F)
    assert L.flimo_map_fpfh(h, 17, 0, C.byref(k), fpfh.ctypes.data, None, None) == 0 and np.all(fpfh == 7)
    assert L.flimo_map_fpfh(h, n, 0, C.byref(k), None, None, None) == 0
    # spfh and cnt may be NULL; a NaN viewpoint that is off is not looked at
    fpfh = np.zeros((n, 33), F)
    assert L.flimo_map_fpfh(h, 0, n, C.byref(quiet), fpfh.ctypes.data, None, None) == 0
    assert fpfh.tobytes() == scene_ctx.map_fpfh(k=10, normal_k=10)["fpfh"].tobytes()
    with pytest.raises(ValueError):
        scene_ctx.map_fpfh(want=("spfh", "normals"), k=10)
    assert scene_ctx.map_size() == n
    np.testing.assert_array_equal(scene_ctx.map_points(), fc.scene())
    # an empty map
    ctx = _lib.HipCtx(0)
    try:
        fpfh = np.full((2, 33), 7, F)
        assert ctx._L.flimo_map_fpfh(ctx._h, 0, 0, C.byref(k), fpfh.ctypes.data, None, None) == 0 and np.all(fpfh == 7)
        assert ctx._L.flimo_map_fpfh(ctx._h, 0, 1, C.byref(k), fpfh.ctypes.data, None, None) == ERR_INVALID and np.all(fpfh == 7)
        assert ctx.map_fpfh(k=10)["fpfh"].shape == (0, 33)
    finally:
        ctx.close()


# ---- 8. tiny maps, the Localizer's form -------------------------------------------------------------------------------------------------
def test_maps_of_one_and_two_points(built):
    from fast_limo_amd import _lib
    for pts in (F([[1.0, 2.0, 3.0]]), F([[1.0, 2.0, 3.0], [1.0, 2.0, 7.0]])):
        ctx = _lib.HipCtx(0)
        try:
            ctx.map_add(pts, stamp=0.5)
            out = ctx.map_fpfh(k=8, normal_k=8)                       # no plane anywhere: no pair, rows of zeros
            assert out["cnt"].tolist() == [len(pts)] * len(pts) and not out["spfh"].any() and fc.bits(out["fpfh"]).max() == 0
        finally:
            ctx.close()


def test_the_localizer_form_equals_the_contexts(built):
    from fast_limo_amd import api
    cfg = dict(k=12, normal_k=10, max_dist=1.0, viewpoint=fc.VIEWPOINT)
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        out = loc.map_fpfh(**cfg)                                     # no map yet: an empty one's answer
        assert out["fpfh"].shape == (0, 33) and len(out["cnt"]) == 0
        with pytest.raises(api.FlimoError):
            loc.map_fpfh(0, 5, **cfg)
        with pytest.raises(api.FlimoError):
            loc.map_fpfh(k=1)
        loc.map_add(fc.scene())
        n = loc.map_size()
        _same_bits(loc.map_fpfh(**cfg), loc.hip.map_fpfh(**cfg), "whole")
        a, b = loc.map_fpfh(n - 300, 200, want=("cnt",), **cfg), loc.hip.map_fpfh(n - 300, 200, want=("cnt",), **cfg)
        assert sorted(a) == ["cnt", "fpfh"] and a["fpfh"].tobytes() == b["fpfh"].tobytes() and a["fpfh"].any()
        with pytest.raises(api.FlimoError):
            loc.map_fpfh(0, n + 1, **cfg)
    finally:
        loc.close()
