"""FPFH descriptors of the stored points (flimo_map_fpfh) as far as they can be checked without a GPU: both libraries export and
declare the new entry points, the calls reject a null context, and the numpy restatement of the definition (tests/fpfh_common.py)
has the properties the GPU tests lean on -- a pair worked by hand lands in the bins the hand computation gives, every non-empty
group of a row sums to 100, a point's counts stay below its list's length, a translation on a lattice moves no bit, and on every
cloud the GPU tests use the restatement taints at most 0.5 % of the points, so that their exclusion of tainted points cannot hide a
failure.  The kernels run on the GPU: tests/test_gpu_fpfh.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import fpfh_common as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2
F = np.float32

HIP_NAMES = ("flimo_map_fpfh", "flimo_set_fpfh_chunk")
HOST_NAMES = ("flimo_loc_map_fpfh",)


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
    assert "int flimo_map_fpfh(flimo_ctx* ctx, size_t first, size_t n, const flimo_fpfh_cfg* cfg, float* fpfh" in pub
    assert "} flimo_fpfh_cfg;" in pub and "tests/fpfh_common.py" in pub and "flimo_set_fpfh_chunk(" in dev
    for name in HOST_NAMES:
        assert hasattr(H, name) and name in api.HOST_SYMBOLS and name + "(" in decl, name
    for name in ("map_fpfh", "set_fpfh_chunk"):
        assert hasattr(_lib.HipCtx, name), name
    assert hasattr(api.Localizer, "map_fpfh")
    # the struct as the header lays it out
    assert C.sizeof(_lib.FpfhCfg) == 36
    assert [f[0] for f in _lib.FpfhCfg._fields_] == ["k", "max_dist", "normal_k", "normal_max_dist", "normal_min_pts", "has_viewpoint", "viewpoint"]
    k = _lib.fpfh_cfg(k=12, viewpoint=(1, 2, 3))
    assert (k.k, k.has_viewpoint, list(k.viewpoint), math.isinf(k.max_dist)) == (12, 1, [1.0, 2.0, 3.0], True)
    assert _lib.fpfh_cfg().has_viewpoint == 0


def test_the_calls_reject_a_null_context_and_leave_their_outputs():
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    k = _lib.fpfh_cfg()
    fpfh, spfh, cnt = np.full((2, 33), 7, F), np.full((2, 33), 7, np.uint8), np.full(2, 7, np.int32)
    assert L.flimo_map_fpfh(None, 0, 2, C.byref(k), fpfh.ctypes.data, spfh.ctypes.data, cnt.ctypes.data) == ERR_INVALID
    assert H.flimo_loc_map_fpfh(None, 0, 2, C.byref(k), fpfh.ctypes.data, spfh.ctypes.data, cnt.ctypes.data) == ERR_INVALID
    assert L.flimo_set_fpfh_chunk(None, 5) == ERR_INVALID
    assert np.all(fpfh == 7) and np.all(spfh == 7) and np.all(cnt == 7)


def _pair_bins(p0, n0, p1, n1):
    f = fc.pair_features(F([p0]), F([p1]), F([n0]), F([n1]))
    assert f["ok"][0] and not f["ambiguous"][0]
    return int(f["h1"][0]), int(f["h2"][0]), int(f["h3"][0])


def test_a_pair_worked_by_hand():
    """Two points one unit apart on x.  s = sin 0.3 = 0.29552, c = cos 0.3; a bin of theta spans 2 pi / 11 = 0.5712 rad, bin 5 is
    [-0.2856, 0.2856); a bin of the two cosines spans 2 / 11, bin 5 is [-0.0909, 0.0909), bin 3 is [-0.4545, -0.2727).

    A. normals +z and (0, s, c) -- tilted about the line that joins the points.  0 -> 1: d = (1, 0, 0), a1 = a2 = 0, no swap:
       u = (0, 0, 1), m = (0, s, c), f3 = 0 -> bin 5.  v = d x u = (0, -1, 0), |v| = 1.  w = u x v = (1, 0, 0).  f2 = v.m = -s ->
       11 * (0.70448 / 2) = 3.87 -> bin 3.  f1 = atan2(w.m, u.m) = atan2(0, c) = 0 -> 5.5 -> bin 5.  So (5, 3, 5): the tilt
       shows in alpha, not in theta.  1 -> 0: d = (-1, 0, 0), a1 = a2 = 0: u = (0, s, c), m = (0, 0, 1), f3 = 0; v = d x u =
       (0, c, -s); w = u x v = (-(s*s + c*c), 0, 0) = (-1, 0, 0); f2 = v.m = -s; f1 = atan2(-0.0 + 0, c) = 0: (5, 3, 5) again.
    B. normals +z and (s, 0, c) -- tilted towards the line.  0 -> 1: d = (1, 0, 0), a1 = 0, a2 = s: |a1| < |a2| swaps: u = (s, 0, c),
       m = (0, 0, 1), d = (-1, 0, 0), f3 = -s -> bin 3.  v = d x u = (0, c, 0) -> (0, 1, 0).  w = u x v = (-c, 0, s).  f2 = v.m = 0
       -> bin 5.  f1 = atan2(w.m, u.m) = atan2(s, c) = 0.3 > 0.2856 -> 11 * (3.4416 / 6.2832) = 6.03 -> bin 6.  So (6, 5, 3).
       1 -> 0: d = (-1, 0, 0), a1 = -s, a2 = 0: no swap, the same u, m, d, f3 = a1 = -s: (6, 5, 3) again."""
    s, c = math.sin(0.3), math.cos(0.3)
    p0, p1, z = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    assert _pair_bins(p0, z, p1, (0.0, s, c)) == (5, 3, 5)
    assert _pair_bins(p1, (0.0, s, c), p0, z) == (5, 3, 5)
    assert _pair_bins(p0, z, p1, (s, 0.0, c)) == (6, 5, 3)
    assert _pair_bins(p1, (s, 0.0, c), p0, z) == (6, 5, 3)
    # no pair at all: a NaN normal on either side, a frame that degenerates (the normal along the line)
    f = fc.pair_features(F([p0, p0, p0]), F([p1, p1, p1]), F([z, (np.nan, 0, 1), (1, 0, 0)]), F([(0, np.nan, 1), z, (1, 0, 0)]))
    assert f["ok"].tolist() == [False, False, False]
    # the two ambiguous kinds: theta on a bin's edge; w.m == 0 with u.m < 0
    f = fc.pair_features(F([p0]), F([p1]), F([z]), F([(0.0, 0.0, -1.0)]))
    assert f["ok"][0] and f["ambiguous"][0] and int(f["h1"][0]) in (0, 10)


@pytest.fixture(scope="module")
def restated():
    """The restatement on every cloud the GPU tests use, fed by brute force on the CPU (computed once)."""
    out = {}
    for name, (cloud, cfg) in fc.CASES.items():
        pts = cloud()
        nrm = fc.cpu_normals(pts, cfg["normal_k"], cfg.get("normal_max_dist", fc.INF), 3, cfg.get("viewpoint"))
        idx, sqd, cnt = fc.cpu_lists(pts, cfg["k"], cfg.get("max_dist", fc.INF))
        out[name] = (pts, nrm, idx, sqd, cnt, fc.restate(pts, nrm, idx, sqd, cnt))
    return out


def test_rows_sum_to_100_and_counts_stay_below_the_lists_length(restated):
    for name, (pts, nrm, idx, sqd, cnt, r) in restated.items():
        rows = r["fpfh"].astype(np.float64).reshape(-1, 3, fc.BINS)
        sums, live = rows.sum(2), r["group_sum"] != 0.0
        print(name, "groups", int(live.sum()), "worst", float(np.abs(sums[live] - 100.0).max(initial=0.0)) / 100.0, "bound", 33 * 2.0 ** -23)
        assert np.all(np.abs(sums[live] - 100.0) <= 33 * 2.0 ** -23 * 100.0), name
        assert np.all(sums[~live] == 0.0) and np.all(rows >= 0.0), name
        assert live.any(), name
        if name == "duplicates":
            assert np.all(cnt[-4:] == 3) and not r["spfh"][-4:].any() and not r["fpfh"][-4:].any()
        per_group = r["spfh"].astype(np.int64).reshape(-1, 3, fc.BINS).sum(2)
        assert np.all(per_group <= np.maximum(cnt - 1, 0)[:, None]), name
        assert np.all(per_group[:, 0:1] == per_group), name              # a pair counts once in each of the three
    _, nrm, idx, _, cnt, r = restated["sparse-normal"]
    assert np.isnan(nrm[-1]).all() and not np.isnan(nrm[:-1]).any() and (idx[:-1] == len(cnt) - 1).any()
    assert not r["spfh"][-1].any() and cnt[-1] == 10 and r["fpfh"][-1].any()      # no plane of its own, a row from its neighbours


def test_a_translation_on_the_lattice_moves_no_bit(restated):
    a, b = restated["lattice-k10"], restated["lattice-shifted-k10"]
    assert np.all(np.abs(a[0]) <= 32.0) and np.array_equal(a[0] * 1024.0, np.round(a[0] * 1024.0))
    for i in (1, 2, 3, 4):
        assert a[i].tobytes() == b[i].tobytes(), i                        # normals, lists, distances, counts
    for key in ("fpfh", "spfh", "cnt", "tainted"):
        assert a[5][key].tobytes() == b[5][key].tobytes(), key


def test_the_restatement_taints_few_points_of_every_cloud(restated):
    for name, (pts, _, _, _, _, r) in restated.items():
        share = float(r["tainted"].mean())
        print(name, "points", len(pts), "ambiguous pairs", int(r["pair_amb"].sum()), "tainted", int(r["tainted"].sum()), "share", share)
        assert share <= fc.MAX_TAINTED, name


def test_moves_between_neighbouring_theta_bins():
    want = np.zeros(33, np.int64); want[[0, 4, 15, 30]] = [2, 1, 3, 3]
    got = want.copy(); got[0] -= 1; got[10] += 1
    assert fc.moved_by_ambiguous_pairs(got, want, [0]) and fc.moved_by_ambiguous_pairs(want, want, [0])
    assert not fc.moved_by_ambiguous_pairs(got, want, [4]) and not fc.moved_by_ambiguous_pairs(got, want, [])
    got = want.copy(); got[15] -= 1; got[16] += 1
    assert not fc.moved_by_ambiguous_pairs(got, want, [0, 4])
