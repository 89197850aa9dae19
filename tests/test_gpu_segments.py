"""GPU suite: map segments -- the table of insertion-index runs a context keeps, flimo_map_correct / flimo_map_transform (every
stored point moved by its segment's matrix, the index rebuilt once), flimo_map_corrected (the predicate alone) and
flimo_map_remove_range (forgetting by age).  The reference has no loop closure, so the meaning is this project's
(include/flimo_c.h, "Map segments"): tests/segments_common.py restates the segment of a point and the move in numpy, every
comparison of points is bit for bit, and a corrected map is compared with a twin context given clear + add(restated points).  The
one tolerance (the ring scene's last bullet) is derived where it is used.  Everything goes through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import segments_common as sg
from common import CAPS
from fast_limo_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_HIP, ERR_NOMAP, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -3, -4, -5, -6
F = np.float32
SEG_MAX = 1 << 20
SLAB = 2048                      # the move's default: a workgroup's step; each of its four waves takes a quarter
PLANS = [(0, 0), (256, 1)]       # (slab, blocks): the default, and the smallest slab on one workgroup


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b, what=""):
    assert a.shape == b.shape and _bits(a).tobytes() == _bits(b).tobytes(), what


def cloud(n, seed, spread=20.0, centre=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-spread, spread, (n, 3)) + np.asarray(centre)).astype(F)


def mats(S, kind, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "identity":
        return np.tile(sg.IDENTITY, (S, 1))
    if kind == "rigid":
        return np.array([sg.rigid(rng.uniform(-3, 3, 3), rng.uniform(-0.5, 0.5, 3)) for _ in range(S)])
    if kind == "nonrigid":
        return rng.normal(0, 1, (S, 12))
    raise KeyError(kind)


@pytest.fixture(scope="module")
def hip(built):
    """One context for the tests that only need stored points in a known order: nothing is dropped (down-sampling off)."""
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, False)
    yield ctx
    ctx.close()


def build(ctx, pts, bounds):
    """The map = pts in this order, with a mark at every entry of `bounds` (interior boundaries, ascending, repeats: empty segments)."""
    ctx.map_clear()
    ctx.set_segment_plan(0, 0)
    at = 0
    for b in bounds:
        if b > at:
            ctx.map_add(pts[at:b], stamp=1.0)
            at = b
        ctx.map_segment_mark()
    if len(pts) > at:
        ctx.map_add(pts[at:], stamp=2.0)
    begin, stale = ctx.map_segments()
    assert begin.tolist() == [0] + list(bounds) + [len(pts)] and not stale
    _same(ctx.map_points(), pts, "insertion order")
    return begin


def check_corrected(ctx, T, plans=PLANS):
    begin, _ = ctx.map_segments()
    pts = ctx.map_points().copy()
    want, chg = sg.corrected(begin, T, pts)
    for slab, blocks in plans:
        ctx.set_segment_plan(slab, blocks)
        got, c = ctx.map_corrected(T)
        _same(got, want, "plan %r" % ((slab, blocks),))
        assert c == chg
        assert ctx.map_corrected(T, want_xyz=False) == (None, chg)
    ctx.set_segment_plan(0, 0)
    _same(ctx.map_points(), pts, "the predicate changes nothing")
    return want, chg


def check_correct(ctx, T):
    begin, _ = ctx.map_segments()
    want, chg = sg.corrected(begin, T, ctx.map_points())
    t_before = ctx._L.flimo_map_last_time(ctx._h)
    assert ctx.map_correct(T) == chg
    _same(ctx.map_points(), want, "the corrected map")
    after, stale = ctx.map_segments()
    assert after.tolist() == begin.tolist() and not stale
    assert ctx._L.flimo_map_last_time(ctx._h) == t_before
    assert ctx.grid_selfcheck()[0] == 0
    return want, chg


def raw(ctx, name, *args):
    rc = getattr(ctx._L, name)(ctx._h, *args)
    return rc, ctx._L.flimo_last_error(ctx._h).decode()


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_the_table_follows_five_batches_through_the_down_sampling_rule(built):
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(0.2, 2, True)
        assert ctx.map_segments()[0].tolist() == [0, 0] and not ctx.map_segments()[1]
        base = synth.box_world_map(6000, 8.0, 3)
        sizes, given = [], 0
        for k in range(5):
            if k:
                assert ctx.map_segment_mark() == k
            b = base + F(0.003 * k) if k % 2 == 0 else np.concatenate([base[::2], synth.box_world_map(2000, 9.0, 10 + k)])
            ctx.map_add(b, stamp=10.0 + k)
            given += len(b)
            sizes.append(ctx.map_size())
        begin, stale = ctx.map_segments()
        assert begin.tolist() == [0] + sizes and not stale
        assert sizes[-1] < given and sizes == sorted(sizes) and len(set(sizes)) >= 3, (sizes, given)      # the rule dropped points
        # an add with nothing to store moves no boundary; the open segment's end is the size
        ctx.map_add(base, stamp=20.0)
        assert ctx.map_segments()[0].tolist() == [0] + sizes[:-1] + [ctx.map_size()]
    finally:
        ctx.close()


def test_empty_segments_the_zero_size_root_stale_reset_and_clear(hip):
    ctx = hip
    ctx.map_clear()
    assert [ctx.map_segment_mark() for _ in range(3)] == [1, 2, 3]
    assert ctx.map_segments()[0].tolist() == [0, 0, 0, 0, 0]
    # asked with too little room; asked for the count alone
    n_seg, stale, room = C.c_size_t(0), C.c_int(9), np.zeros(4, np.uint64)
    assert ctx._L.flimo_map_segments(ctx._h, room.ctypes.data, 4, C.byref(n_seg), C.byref(stale)) == ERR_INVALID
    assert ctx._L.flimo_map_segments(ctx._h, None, 0, C.byref(n_seg), C.byref(stale)) == 0 and (n_seg.value, stale.value) == (4, 0)
    # 300 duplicates, then one point elsewhere: the root has size zero and the batch leaves it -- everything is stored again, in order
    ctx.map_clear()
    dup = np.tile(F([[1.5, -2.25, 0.5]]), (300, 1))
    ctx.map_add(dup[:100], stamp=1.0)
    ctx.map_segment_mark()
    ctx.map_add(dup[100:], stamp=2.0)
    ctx.map_segment_mark()
    ctx.map_add(F([[7.0, 3.0, -1.0]]), stamp=3.0)
    begin, stale = ctx.map_segments()
    assert begin.tolist() == [0, 100, 300, 301] and not stale
    _same(ctx.map_points(), np.concatenate([dup, F([[7.0, 3.0, -1.0]])]))
    T = mats(3, "rigid", 1)
    check_corrected(ctx, T)
    check_correct(ctx, T)
    # a crop that removes nothing leaves the table valid; one that removes a point makes it stale
    pts = cloud(1000, 4)
    build(ctx, pts, [300, 700])
    assert ctx.map_crop_box(F([-100] * 3), F([100] * 3)) == 0
    begin, stale = ctx.map_segments()
    assert begin.tolist() == [0, 300, 700, 1000] and not stale
    lo, hi = pts.min(0), pts.max(0)
    worst = int(np.argmax(pts[:, 0]))
    hi_cut = hi.copy()
    hi_cut[0] = np.sort(pts[:, 0])[-2]                                  # the box ends at the second largest x: one point goes
    assert ctx.map_crop_box(lo, hi_cut) == 1
    kept = np.delete(pts, worst, axis=0)
    _same(ctx.map_points(), kept)
    assert ctx.map_segments()[1] is True
    T = mats(3, "rigid", 2)
    for name, args in (("flimo_map_segment_mark", (None,)), ("flimo_map_correct", (T.ctypes.data, 3, None)),
                       ("flimo_map_corrected", (T.ctypes.data, 3, 0, 10, None, None))):
        rc, msg = raw(ctx, name, *args)
        assert rc == ERR_NOMAP and "stale" in msg, (name, rc, msg)
    _same(ctx.map_points(), kept)
    # the rigid move of the whole map does not read the table: it works, and leaves table and flag alone
    one = mats(1, "rigid", 3)
    moved = sg.seg_move(np.tile(one, (len(kept), 1)), kept)
    assert ctx.map_transform(one) == int(np.any(_bits(moved) != _bits(kept), axis=1).sum()) > 0
    _same(ctx.map_points(), moved)
    assert ctx.map_segments()[1] is True
    ctx.map_segments_reset()
    begin, stale = ctx.map_segments()
    assert begin.tolist() == [0, 999] and not stale and ctx.map_segment_mark() == 1
    assert ctx.map_crop_box(lo - F(5), hi_cut - F(5)) > 0 and ctx.map_segments()[1] is True
    ctx.map_clear()
    begin, stale = ctx.map_segments()
    assert begin.tolist() == [0, 0] and not stale


def test_the_table_ends_at_seg_max(hip):
    ctx = hip
    ctx.map_clear()
    mark, h = ctx._L.flimo_map_segment_mark, ctx._h
    for _ in range(SEG_MAX - 2):
        mark(h, None)
    at = C.c_size_t(0)
    assert mark(h, C.byref(at)) == 0 and at.value == SEG_MAX - 1
    rc, msg = raw(ctx, "flimo_map_segment_mark", C.byref(at))
    assert rc == ERR_TOO_LARGE and at.value == SEG_MAX - 1
    begin, stale = ctx.map_segments()
    assert begin.shape == (SEG_MAX + 1,) and not begin.any() and not stale
    ctx.map_clear()
    assert ctx.map_segments()[0].tolist() == [0, 0]


# ---- the move ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097])
def test_the_move_is_the_restatement_at_every_size(hip, n):
    ctx = hip
    pts = cloud(n, n)
    pts[::7, 0] = -0.0                                                  # stored -0.0 coordinates
    pts[3::11] = np.where(pts[3::11] < 0, F(-0.0), pts[3::11])
    shapes = [[]] + ([[n // 3, n // 3, n - n // 4]] if n >= 255 else [])        # one segment; four with an empty one in the middle
    for bounds in shapes:
        begin = build(ctx, pts, bounds)
        S = len(begin) - 1
        # all-identity matrices: exactly the points with a -0.0 component change (it comes back as +0.0)
        want, chg = check_corrected(ctx, mats(S, "identity"))
        assert chg == int(np.any(_bits(pts) == 0x80000000, axis=1).sum()) > 0
        _same(np.abs(want), np.abs(pts))
        check_corrected(ctx, mats(S, "rigid", n))
        check_corrected(ctx, mats(S, "nonrigid", n))
        # ranges that cut segments
        T = mats(S, "rigid", n + 1)
        full, _ = sg.corrected(begin, T, pts)
        for first, m in {(0, n), (n // 2, n - n // 2), (n // 3 + (n > 1), max(n // 2 - 1, 0)), (n, 0), (n - 1, 1)}:
            got, c = ctx.map_corrected(T, first, m)
            _same(got, full[first:first + m], "range %d + %d" % (first, m))
            assert c == sg.corrected(begin, T, pts[first:first + m], first)[1]
        check_correct(ctx, T)
    # the identity on a map without -0.0: no bit changes, and nothing happens at all
    build(ctx, np.abs(pts), [])
    merges, builds = ctx.grid_selfcheck()[1:]
    assert ctx.map_correct(sg.IDENTITY) == 0 and ctx.map_transform(sg.IDENTITY) == 0
    assert ctx.grid_selfcheck()[1:] == (merges, builds)


def test_a_map_ten_kilometres_away(hip):
    ctx = hip
    pts = cloud(3000, 77, 30.0, (10000.0, -7000.0, 120.0))
    build(ctx, pts, [1000, 2100])
    T = np.array([sg.rigid((0.1 * s, -0.05, 0.3 * s), (0.2, -0.1 * s, 0.05)) for s in range(3)])
    # a correction about the far map's own centre: T = [R | c - R c + t]
    c0 = np.array([10000.0, -7000.0, 120.0])
    for s in range(3):
        R = T[s].reshape(3, 4)[:, :3]
        T[s].reshape(3, 4)[:, 3] += c0 - R @ c0
    check_corrected(ctx, T)
    want, chg = check_correct(ctx, T)
    assert chg > 2900 and np.abs(want - pts).max() < 5.0


def test_two_segments_with_the_boundary_around_every_edge(hip):
    """A wave takes a quarter of a slab: with the default slab of 2048 points its edges are the multiples of 512, with the slab
    forced to 256 the multiples of 64 (and a workgroup's edges the multiples of 256).  The boundary one before, at and one after."""
    ctx = hip
    for n, plan, step in ((4097, (0, 0), SLAB // 4), (1100, (256, 2), 64)):
        pts = cloud(n, 5 + n)
        T = mats(2, "rigid", n)
        for edge in range(step, n + 1, step):
            for b in (edge - 1, edge, edge + 1):
                if not 0 < b < n:
                    continue
                ctx.map_clear()
                ctx.map_add(pts[:b], stamp=1.0)
                ctx.map_segment_mark()
                ctx.map_add(pts[b:], stamp=2.0)
                ctx.set_segment_plan(*plan)
                got, c = ctx.map_corrected(T)
                want, chg = sg.corrected([0, b, n], T, pts)
                _same(got, want, "n %d boundary %d" % (n, b))
                assert c == chg
    ctx.set_segment_plan(0, 0)


def test_segment_shapes(hip):
    ctx = hip
    n = 4097
    pts = cloud(n, 31)
    shapes = {"an empty segment at the start, in the middle and at the end": [0, 0, 1500, 1500, 1500, 3000, n, n],
              "300 segments of one point": list(range(1, 301)),
              "300 segments of one point in the middle of a slab": [2500] + list(range(2501, 2801)),
              "a segment longer than several slabs between short ones": [3, 3600, 3601, 3700]}
    for what, bounds in shapes.items():
        begin = build(ctx, pts, bounds)
        S = len(begin) - 1
        check_corrected(ctx, mats(S, "rigid", S), plans=PLANS + [(512, 3), (16384, 0)])
        check_corrected(ctx, mats(S, "nonrigid", S))
        check_correct(ctx, mats(S, "rigid", S + 1))


# ---- the corrected map ---------------------------------------------------------------------------------------------------------
def _pass(ctx, x):
    """One registration pass as its bits: the sums, the count, which points found a plane and every record of those.  The resident
    scan is set again first, so that the pass is the first of its scan wherever it is asked for: the order in which a pass adds up
    its sums depends on its position in its scan (test_gpu_local_map.py), its records do not.  (This drops the scan's covariances.)"""
    ctx.scan_set(ctx.scan_get())
    ctx.set_debug_records(True)
    HTH, HTh, M = ctx.match_reduce(x, _lib.default_match_cfg(**CAPS))
    g = ctx.match_fetch()
    ctx.set_debug_records(False)
    ok = g["valid"] > 0
    assert M == int(ok.sum()) > 500
    return HTH.tobytes() + HTh.tobytes(), M, ok.tobytes(), g[ok].tobytes()


def _scene(ctx, seed=1):
    """A box world in four batches (down-sampling on: the rule drops points), a mark before each but the first, a scan."""
    ctx.map_config(0.2, 2, True)
    for k in range(4):
        if k:
            ctx.map_segment_mark()
        ctx.map_add(synth.box_world_map(6000, 12.0, seed + k) + F([0.5 * k, 0, 0]), stamp=3.0 + k)
    ctx.scan_set(np.ascontiguousarray(synth.box_world_scan_random(2048, 12.0, 9)[:, :3]))
    x = np.zeros(26)
    x[0:3], x[6], x[10], x[25] = synth.T_STAR_T, 1.0, 1.0, -9.809
    return x


def _assert_twins(ctx, twin, q, x, what):
    _same(ctx.map_points(), twin.map_points(), what)
    for a, b in zip(ctx.knn_k(q, 8), twin.knn_k(q, 8)):
        assert a.tobytes() == b.tobytes(), what
    # a pass as the context stands (a bound or a record that named old positions would show here), then one like for like
    cfg = _lib.default_match_cfg(**CAPS)
    a, b = ctx.match_reduce(x, cfg), twin.match_reduce(x, cfg)
    assert a[2] == b[2] > 500, what                                    # (sums of passes at different positions in their scans: another order)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-9, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-9, atol=1e-9, err_msg=what)
    assert _pass(ctx, x) == _pass(twin, x), what
    assert ctx.grid_selfcheck()[0] == 0


def test_after_a_correction_the_context_is_a_twin_given_clear_and_add(built):
    ctx, twin = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        x = _scene(ctx)
        twin.map_config(0.2, 2, True)
        twin.scan_set(ctx.scan_get())
        begin, _ = ctx.map_segments()
        assert len(begin) == 5 and ctx.map_size() < 24000
        before = ctx.map_points().copy()
        q = cloud(64, 3, 12.0)
        _pass(ctx, x)                                                   # a pass before: its bound and records name old positions
        T = np.array([sg.rigid((0.02 * s, -0.01, 0.2 * s), (0.03 * s, -0.02, 0.01)) for s in range(4)])
        want, chg = sg.corrected(begin, T, before)
        assert ctx.map_correct(T) == chg > 0.9 * len(before)
        twin.map_add(want, stamp=99.0)
        _assert_twins(ctx, twin, q, x, "map_correct")
        after, stale = ctx.map_segments()
        assert after.tolist() == begin.tolist() and not stale
        assert ctx._L.flimo_map_last_time(ctx._h) == 6.0                # a correction is no insert
        # adds go on: the open segment grows, on both
        more = synth.box_world_map(3000, 12.0, 50) + F([0.1, 0.2, 0])
        ctx.map_add(more, stamp=7.0)
        twin.map_add(more, stamp=7.0)
        _assert_twins(ctx, twin, q, x, "an add after map_correct")
        assert ctx.map_segments()[0].tolist() == begin.tolist()[:-1] + [ctx.map_size()]
        # map_transform = map_correct with the same matrix in every row; it works on a stale table
        one = sg.rigid((0.3, -0.2, 5.0), (1.0, -2.0, 0.25))
        now = ctx.map_points().copy()
        moved = sg.seg_move(np.tile(one, (len(now), 1)), now)
        twin.map_clear()
        twin.map_add(now, stamp=1.0)
        assert twin.map_correct(one) == ctx.map_transform(one) == int(np.any(_bits(moved) != _bits(now), axis=1).sum())
        _same(ctx.map_points(), moved)
        _assert_twins(ctx, twin, q, x, "map_transform")
    finally:
        ctx.close()
        twin.close()


def test_forgetting_by_age(built):
    ctx, twin = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        x = _scene(ctx, seed=20)
        twin.map_config(0.2, 2, True)
        twin.scan_set(ctx.scan_get())
        q = cloud(64, 4, 12.0)
        begin = ctx.map_segments()[0]
        b = [int(v) for v in begin]
        n = b[-1]
        t_last = ctx._L.flimo_map_last_time(ctx._h)
        cases = [("of nothing", 5, 0), ("beyond the size", n, 10), ("at the start", 0, b[1] // 2), ("in the middle", b[1] + 10, 500),
                 ("across three segments", None, None), ("at the end and past the size", None, 1 << 40)]
        for what, first, cnt in cases:
            begin = ctx.map_segments()[0]
            n = int(begin[-1])
            if what == "across three segments":
                first, cnt = int(begin[1]) - 7, int(begin[3]) + 9 - (int(begin[1]) - 7)
            if what == "at the end and past the size":
                first = n - 300
            pts = ctx.map_points().copy()
            gone = max(0, min(cnt, n - first))
            kept = np.concatenate([pts[:first], pts[first + gone:]])
            assert ctx.map_remove_range(first, cnt) == gone, what
            after, stale = ctx.map_segments()
            assert after.tolist() == sg.range_removed_table(begin, first, cnt).tolist() and not stale, what
            assert int(after[-1]) == ctx.map_size() == len(kept)
            _same(ctx.map_points(), kept, what)
            assert ctx._L.flimo_map_last_time(ctx._h) == t_last
            if gone:
                twin.map_clear()
                twin.map_add(kept, stamp=1.0)
                _assert_twins(ctx, twin, q, x, what)
        # the table still says where a stretch lies: a correction by it after the removals
        check_correct(ctx, mats(4, "rigid", 9))
        # everything goes: an empty map, the table all zero, not stale
        assert ctx.map_remove_range(0) == len(kept) and ctx.map_size() == 0
        after, stale = ctx.map_segments()
        assert after.tolist() == [0] * 5 and not stale
        assert ctx.map_correct(mats(4, "rigid", 9)) == 0
    finally:
        ctx.close()
        twin.close()


def test_failures_leave_everything_and_a_correction_leaves_what_it_should(built):
    ctx = _lib.HipCtx(0)
    try:
        x = _scene(ctx, seed=40)
        ctx.sc_db_add_scan(rings=10, sectors=30, max_range=40.0)
        ctx.gicp_build(10, float("inf"), 3)
        ctx.ndt_build(0, 1.0)
        assert ctx.gicp_info()["stale"] == 0 and ctx.ndt_info(0)["stale"] == 0
        pts, table = ctx.map_points().copy(), ctx.map_segments()[0]
        scan, sc = ctx.scan_get().copy(), ctx.sc_db_get().copy()
        first_pass = _pass(ctx, x)
        T = np.array([sg.rigid((0.02 * s, -0.01, 0.2 * s), (0.03 * s, -0.02, 0.01)) for s in range(4)])

        def untouched(what):
            _same(ctx.map_points(), pts, what)
            begin, stale = ctx.map_segments()
            assert begin.tolist() == table.tolist() and not stale, what
            assert _pass(ctx, x) == first_pass, what
            assert ctx.gicp_info()["stale"] == 0 and ctx.ndt_info(0)["stale"] == 0, what

        # the predicate moves no bit of a later pass
        ctx.map_corrected(T)
        untouched("map_corrected")
        # a matrix that overflows float32; a move whose box a fresh octree refuses (finite, but 2^48 * 0.4 m is about 1e14 m)
        big, far = T.copy(), T.copy()
        big[2, 3] = 1e39
        far[1, 0:3] *= 1e19
        keep = C.c_size_t(77)
        for name, bad in (("overflow", big), ("box", far)):
            rc, msg = raw(ctx, "flimo_map_correct", bad.ctypes.data, 4, C.byref(keep))
            assert rc == ERR_UNSUPPORTED and keep.value == 0, (name, rc, msg)
            untouched(name)
            rc, msg = raw(ctx, "flimo_map_transform", bad[1 if name == "box" else 2].ctypes.data, C.byref(keep))
            assert rc == ERR_UNSUPPORTED, (name, rc, msg)
            untouched(name + " (transform)")
        assert "not finite" in raw(ctx, "flimo_map_correct", big.ctypes.data, 4, None)[1]
        assert "octree too deep" in raw(ctx, "flimo_map_correct", far.ctypes.data, 4, None)[1]
        # every rejected argument
        nan, inf = T.copy(), T.copy()
        nan[3, 11], inf[0, 0] = np.nan, np.inf
        xyz = np.zeros((10, 3), F)
        for what, name, args in (("null T", "flimo_map_correct", (None, 4, None)), ("NaN", "flimo_map_correct", (nan.ctypes.data, 4, None)),
                                 ("inf", "flimo_map_correct", (inf.ctypes.data, 4, None)), ("S - 1", "flimo_map_correct", (T.ctypes.data, 3, None)),
                                 ("S + 1", "flimo_map_correct", (np.tile(T, (2, 1)).ctypes.data, 5, None)),
                                 ("no matrix", "flimo_map_correct", (T.ctypes.data, 0, None)),
                                 ("null T", "flimo_map_transform", (None, None)), ("NaN", "flimo_map_transform", (nan[3].ctypes.data, None)),
                                 ("null T", "flimo_map_corrected", (None, 4, 0, 10, xyz.ctypes.data, None)),
                                 ("NaN", "flimo_map_corrected", (nan.ctypes.data, 4, 0, 10, xyz.ctypes.data, None)),
                                 ("S - 1", "flimo_map_corrected", (T.ctypes.data, 3, 0, 10, xyz.ctypes.data, None)),
                                 ("beyond the map", "flimo_map_corrected", (T.ctypes.data, 4, len(pts) - 5, 10, xyz.ctypes.data, None)),
                                 ("beyond the map", "flimo_map_corrected", (T.ctypes.data, 4, len(pts) + 1, 0, xyz.ctypes.data, None))):
            rc, msg = raw(ctx, name, *args)
            assert rc == ERR_INVALID, (what, name, rc, msg)
        assert not xyz.any()
        assert ctx._L.flimo_map_correct(None, T.ctypes.data, 4, None) == ERR_INVALID
        assert ctx._L.flimo_map_remove_range(None, 0, 1, None) == ERR_INVALID
        assert ctx._L.flimo_set_segment_plan(ctx._h, 100, 0) == ERR_INVALID and ctx._L.flimo_set_segment_plan(ctx._h, 256, -1) == ERR_INVALID
        untouched("rejected arguments")
        # a correction: the models go stale, the scan, its covariances and the place database stay
        ctx.scan_cov_set(np.tile([1e-3, 0, 0, 1.0, 0, 1.0], (ctx.scan_size(), 1)))
        assert ctx.map_correct(T) > 0
        assert ctx.gicp_info()["stale"] == 1 and ctx.ndt_info(0)["stale"] == 1
        out = np.zeros(64)
        rc, msg = raw(ctx, "flimo_scan_gicp", x.ctypes.data, 1, 1.0, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, None)
        assert rc == ERR_NOMAP and "stale" in msg
        _same(ctx.scan_get(), scan)
        assert ctx.scan_cov_size() == len(scan) and ctx.sc_db_get().tobytes() == sc.tobytes() and ctx.sc_db_size() == 1
        # a stale table: the same refusal leaves the same map
        now = ctx.map_points().copy()
        assert ctx.map_crop_box(now.min(0) + F([0.5, 0, 0]), now.max(0)) > 0
        now = ctx.map_points().copy()
        rc, msg = raw(ctx, "flimo_map_correct", T.ctypes.data, 4, C.byref(keep))
        assert rc == ERR_NOMAP and "stale" in msg and keep.value == 0
        _same(ctx.map_points(), now)
        assert ctx.map_segments()[1] is True
    finally:
        ctx.close()


def test_the_localizer_twins(built):
    loc = api.Localizer(api.default_cfg(**CAPS))
    try:
        a, b = synth.box_world_map(5000, 12.0, 1), synth.box_world_map(4000, 12.0, 2) + F([0.4, 0, 0])
        loc.map_add(a, stamp=1.0)
        assert loc.map_segment_mark() == 1
        loc.map_add(b, stamp=2.0)
        begin, stale = loc.map_segments()
        assert begin.tolist() == [0, 5000, loc.map_size()] and not stale and 5000 < loc.map_size() <= 9000
        pts = loc.hip.map_points().copy()
        T = mats(2, "rigid", 5)
        want, chg = sg.corrected(begin, T, pts)
        got, c = loc.map_corrected(T)
        _same(got, want)
        assert c == chg and loc.map_corrected(T, 4990, 20, want_xyz=False) == (None, sg.corrected(begin, T, pts[4990:5010], 4990)[1])
        assert loc.map_correct(T) == chg
        _same(loc.hip.map_points(), want)
        one = mats(1, "rigid", 6)
        moved = sg.seg_move(np.tile(one, (len(want), 1)), want)
        assert loc.map_transform(one) > 0
        _same(loc.hip.map_points(), moved)
        assert loc.map_remove_range(4000, 2000) == 2000
        begin, stale = loc.map_segments()
        assert begin.tolist() == [0, 4000, len(pts) - 2000] and not stale
        _same(loc.hip.map_points(), np.concatenate([moved[:4000], moved[6000:]]))
        with pytest.raises(_lib.FlimoError):
            loc.map_correct(mats(3, "rigid", 1))
        loc.map_segments_reset()
        assert loc.map_segments()[0].tolist() == [0, len(pts) - 2000]
    finally:
        loc.close()


# ---- one scene -----------------------------------------------------------------------------------------------------------------
def test_a_loop_closure_moves_the_map_back(built):
    """24 keyframes on a circle of radius 10 m in the box world, each relative pose corrupted by the same body-frame error (0.02 m,
    0.1 degree); sweeps inserted at the drifted poses, one segment each; one exact loop edge, last -> first.

    The last bullet's bound, per stored point p of the last segment, taken by sweep point b (body frame):
      |stored - truth| <= |T_c b - T_true b| + 8 * 2^-24 * max|coordinate|
    T_c b is where the corrected last pose puts b in float64 -- its distance from the true place is that pose's own error.  What is
    stored differs from T_c b by float32 roundings only: b itself (half an ulp per component, carried through a rotation), the
    insert's rounding of T_drift b, the move's rounding, and the move's matrix T_c T_drift^-1 being float64 (negligible): under
    four ulps of the largest coordinate in all, eight with room."""
    truth, drift, edges = sg.ring_case(24, 10.0, 0.02, 0.1)
    x_drift = np.array([sg.x26_of(M) for M in drift])
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(0.2, 2, True)
        given = []
        for k in range(24):
            if k:
                assert ctx.map_segment_mark() == k
            body = sg.ring_sweep(k, truth[k]).astype(F)
            world = sg.place(drift[k], body.astype(np.float64)).astype(F)
            ctx.map_add(world, stamp=float(k))
            given.append((body, world))
        begin, stale = ctx.map_segments()
        assert len(begin) == 25 and not stale and np.all(np.diff(begin.astype(np.int64)) > 0)
        before = ctx.map_points().copy()
        out = api.loop_close(ctx, x_drift, edges)
        after = ctx.map_points()
        # every stored point of segment s lies where the restatement puts it
        want, chg = sg.corrected(begin, out["T"], before)
        _same(after, want)
        assert out["changed"] == chg and ctx.map_segments()[0].tolist() == begin.tolist()
        np.testing.assert_array_equal(out["T"], api.segment_corrections(x_drift, out["x26"]))
        # the last segment against the truth
        lo = int(begin[23])
        body, world = given[23]
        rows = {r.tobytes(): j for j, r in enumerate(world)}
        j = np.array([rows[r.tobytes()] for r in before[lo:]])          # which sweep point each stored point is
        b = body[j].astype(np.float64)
        true_at = sg.place(truth[23], b)
        pose_err = np.linalg.norm(sg.place(sg.mat_of_x26(out["x26"][23]), b) - true_at, axis=1)
        d_after = np.linalg.norm(after[lo:].astype(np.float64) - true_at, axis=1)
        d_before = np.linalg.norm(before[lo:].astype(np.float64) - true_at, axis=1)
        bound = pose_err + 8 * 2.0 ** -24 * max(np.abs(after).max(), np.abs(before).max(), np.abs(body).max())
        print("last segment, %d points: distance from the truth %.4f -> %.4f m (mean), %.4f -> %.4f m (max); largest excess over the pose's own error %.3e m"
              % (len(j), d_before.mean(), d_after.mean(), d_before.max(), d_after.max(), (d_after - pose_err).max()))
        assert np.all(d_after <= bound)
        assert d_after.mean() <= 0.1 * d_before.mean() and d_after.max() <= 0.1 * d_before.max()
    finally:
        ctx.close()
