"""GPU suite: Scan Context place recognition -- flimo_scan_context, the resident database flimo_sc_db_*, flimo_sc_match.  The
yardstick is the definition of include/flimo_c.h restated in numpy (tests/sc_common.py, which tests/test_sc_host.py holds to the
host entries): descriptors, idx, shift, cnt and every bit of dist and of profile are compared with no tolerance, at every edge of
the launch shapes; order, chunks, splits, the other queries and repetition move no bit.  The last test finds every query sweep of
the method's scene among the keyframes and refines its pose (api.place_relocalize)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import corr_common as cc
import front_end_common as fc
import fpfh_common as fpc
import sc_common as sc
from common import CAPS

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_LARGE = -2, -5
F = np.float32
INF = float("inf")


@pytest.fixture(autouse=True)
def feature(built):
    """Every test of this file is about the feature: without its entry points none of them has anything to say."""
    from fast_limo_amd import _lib, api
    L, H = _lib.load_hip(), api.load_host()
    for name in ("flimo_scan_context", "flimo_sc_db_add", "flimo_sc_db_add_scan", "flimo_sc_match", "flimo_sc_dist_host", "flimo_set_sc_chunk"):
        getattr(L, name)
    getattr(H, "flimo_loc_sc_match")


@pytest.fixture(scope="module")
def hip(built):
    from fast_limo_amd import _lib
    ctx = _lib.HipCtx(0)          # raises without a gfx950 device; an empty context will do
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def clean(hip):
    yield
    hip.set_sc_chunk(0, 0)
    hip.sc_db_clear()


def cfg_of(shape, **kw):
    return sc.cfg(rings=shape[0], sectors=shape[1], **kw)


@functools.lru_cache(maxsize=None)
def base(shape=(20, 60)):
    """5 queries, 257 entries and every pair's restated profile: the sub-shapes are its corners (a pair's profile depends on its two
    descriptors alone).  Entry 7 is all-zero, query 4 is all-zero, query 1 is entry 9 rolled by 7 (or 1) columns, entry 11 has a
    NaN, query 3's columns are mostly empty."""
    R, S = shape
    Q, E = sc.random_descs(31 + R, 5, R, S), sc.random_descs(47 + S, 257, R, S)
    E[7] = 0
    Q[4] = 0
    Q[1] = np.roll(E[9], 7 % S, axis=1)
    E[11, 0, 1] = np.nan
    Q[3, :, 3:] = 0
    Q.setflags(write=False)
    E.setflags(write=False)
    return Q, E, sc.profiles(Q, E, 1)


def same_bytes(a, b, tag):
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), f"{tag}: {name}"


# ---- 1. the descriptor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_the_descriptor_at_every_scan_size_with_and_without_a_frame(hip, shape):
    """Scans around the workgroup of 256 and across several of them; reversed and shuffled scans give the same bytes; used exact."""
    c = cfg_of(shape, min_range=1.0, max_range=40.0)
    frame = sc.yaw_frame12(0.7, (0.3, -0.2, 0.4))
    cloud = sc.random_cloud(5, 4097)
    cloud[17] = [np.nan, 1.0, 1.0]
    cloud[18] = [3.0, np.inf, 1.0]
    for n in (0, 1, 255, 256, 257, 4097):
        pts = cloud[:n]
        hip.scan_set(pts)
        for f in (None, frame):
            want, used = sc.descriptor(pts, c, f)
            got, got_used = hip.scan_context(frame12=f, **c)
            assert got.shape == shape and got.tobytes() == want.tobytes() and got_used == used, (n, f is None)
            assert n < 255 or used > n // 3
        if n > 1:
            want = hip.scan_context(**c)
            for order in (np.arange(n)[::-1], np.random.RandomState(n).permutation(n)):
                hip.scan_set(np.ascontiguousarray(pts[order]))
                again = hip.scan_context(**c)
                assert again[0].tobytes() == want[0].tobytes() and again[1] == want[1], n


def test_the_descriptor_with_one_bin_and_with_every_bin(hip):
    """4 097 points in ONE bin (every LDS atomic of a workgroup on one word) and a scan that hits every bin of 32 x 64 once."""
    c = sc.cfg()
    rs = np.random.RandomState(2)
    one = np.stack([np.full(4097, 10.3), np.full(4097, 0.2), rs.uniform(-1.9, 5.0, 4097)], axis=1).astype(F)
    hip.scan_set(one)
    got, used = hip.scan_context(**c)
    want, want_used = sc.descriptor(one, c)
    assert got.tobytes() == want.tobytes() and used == want_used == 4097 and np.count_nonzero(got) == 1
    assert got.max() == (one[:, 2] + F(2.0)).max()
    c = sc.cfg(rings=32, sectors=64, max_range=64.0)
    r, a = np.meshgrid(np.arange(32) * 2.0 + 1.0, (np.arange(64) + 0.5) * (2 * math.pi / 64))
    every = np.stack([r.ravel() * np.cos(a.ravel()), r.ravel() * np.sin(a.ravel()), rs.uniform(-1.0, 3.0, r.size)], axis=1).astype(F)
    hip.scan_set(every)
    got, used = hip.scan_context(**c)
    want, want_used = sc.descriptor(every, c)
    assert got.tobytes() == want.tobytes() and used == want_used == 32 * 64 and np.count_nonzero(got) == 32 * 64


def test_a_pending_deskew_runs_first():
    """After deskew_resident the deskew still rides on the next launch: the descriptor must be the deskewed scan's."""
    from fast_limo_amd import _lib
    case = fc.deskew_case(3)
    c = sc.cfg(max_range=60.0, z_offset=5.0)
    a, b = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        a.scan_set(sc.random_cloud(1, 100))      # (what a missing flush would describe instead)
        a.raw_scan_set(case["xyz"], case["t"])
        a.deskew_resident(case["frames"], case["L2B"], case["x26"])
        got = a.scan_context(**c)
        at = a.sc_db_add_scan(**c)
        body = a.scan_get()
        want = sc.descriptor(body, c)
        assert body.shape == (fc.N_DESKEW, 3) and want[1] > 0
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
        assert at == 0 and a.sc_db_get()[0].tobytes() == want[0].tobytes()
        b.scan_set(body)
        assert b.scan_context(**c)[0].tobytes() == got[0].tobytes()
    finally:
        a.close()
        b.close()


def test_rejected_descriptor_calls_leave_the_outputs_alone(hip):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    hip.scan_set(sc.random_cloud(3, 300))
    desc, used = np.full((20, 60), 7, F), C.c_int32(7)
    good = _lib.sc_cfg()
    frame = sc.yaw_frame12(0.1)

    def call(h=hip._h, k=good, f=None, d=desc.ctypes.data):
        return L.flimo_scan_context(h, None if k is None else C.byref(k), None if f is None else f.ctypes.data, d, C.byref(used))
    bad = [dict(rings=0), dict(rings=33), dict(sectors=1), dict(sectors=65), dict(min_range=-1.0), dict(min_range=float("nan")),
           dict(max_range=INF), dict(max_range=float("nan")), dict(min_range=5.0, max_range=5.0), dict(z_offset=INF), dict(z_offset=float("nan"))]
    for kw in bad:
        assert call(k=_lib.sc_cfg(**kw)) == ERR_INVALID, kw
        assert L.flimo_sc_db_add_scan(hip._h, C.byref(_lib.sc_cfg(**kw)), None, None) == ERR_INVALID, kw
    for j in (0, 5, 11):
        f = frame.copy()
        f[j] = np.nan if j else np.inf
        assert call(f=f) == ERR_INVALID, j
    assert call(h=None) == ERR_INVALID and call(k=None) == ERR_INVALID and call(d=None) == ERR_INVALID
    assert np.all(desc == 7) and used.value == 7 and hip.sc_db_size() == 0
    assert call() == 0 and call(f=frame) == 0
    assert desc.tobytes() == sc.descriptor(hip.scan_get(), sc.cfg(), frame)[0].tobytes()
    assert L.flimo_scan_context(hip._h, C.byref(good), None, desc.ctypes.data, None) == 0      # (used may be NULL)
    hip.scan_set(np.zeros((0, 3), F))
    got, n = hip.scan_context()
    assert n == 0 and not got.any() and got.shape == (20, 60)


# ---- 2. the database -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_adds_in_one_call_and_in_five_return_the_bytes_added(hip, n):
    """257 entries pass the first capacity (64) three times; the ids count up; a match sees the same database either way."""
    Q, E, P = base()
    assert hip.sc_db_size() == 0 and hip.sc_db_shape() == (0, 0)
    assert hip.sc_db_add(E[:n]) == 0
    assert hip.sc_db_size() == n and hip.sc_db_shape() == (20, 60)
    assert hip.sc_db_get().tobytes() == E[:n].tobytes()
    one = hip.sc_match(Q, k=8, want_profile=True)
    sc.same(one, sc.match(Q, E[:n], 8, P=P[:, :n]), f"one add of {n}")
    hip.sc_db_clear()
    cuts = sorted(set(min(n, c) for c in (0, n // 5, n // 3, n // 2, n - 1, n)))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        assert hip.sc_db_add(E[lo:hi]) == lo
    assert hip.sc_db_size() == n and hip.sc_db_get().tobytes() == E[:n].tobytes()
    if n > 2:
        assert hip.sc_db_get(1, n - 2).tobytes() == E[1:n - 1].tobytes()
    same_bytes(one, hip.sc_match(Q, k=8, want_profile=True), f"{n} in parts")


def test_add_scan_is_add_of_the_download_and_the_shape_rule(hip):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    Q, E, P = base()
    c = sc.cfg()
    hip.scan_set(sc.random_cloud(9, 3000))
    desc, _ = hip.scan_context(**c)
    assert hip.sc_db_add(E[:3]) == 0
    assert hip.sc_db_add_scan(**c) == 3 and hip.sc_db_add(desc) == 4
    got = hip.sc_db_get()
    assert got[3].tobytes() == got[4].tobytes() == desc.tobytes() == sc.descriptor(hip.scan_get(), c)[0].tobytes()
    m = hip.sc_match(desc, k=2, want_profile=True)
    assert m["idx"][0].tolist() == [3, 4] and m["shift"][0].tolist() == [0, 0] and m["dist"][0, 0].tobytes() == m["dist"][0, 1].tobytes()
    assert m["profile"][0, 0].tobytes() == m["profile"][0, 1].tobytes()
    # another shape, a NULL array, too many: refused, and the database is as it was
    other = sc.random_descs(1, 2, 32, 64)
    first = C.c_size_t(99)
    assert L.flimo_sc_db_add(hip._h, other.ctypes.data, 2, 32, 64, C.byref(first)) == ERR_INVALID
    assert L.flimo_sc_db_add(hip._h, None, 2, 20, 60, C.byref(first)) == ERR_INVALID
    assert L.flimo_sc_db_add(hip._h, E.ctypes.data, 2, 0, 60, C.byref(first)) == ERR_INVALID
    assert L.flimo_sc_db_add(hip._h, E.ctypes.data, 2, 20, 65, C.byref(first)) == ERR_INVALID
    assert L.flimo_sc_db_add(hip._h, E.ctypes.data, 2 ** 31 - 5, 20, 60, C.byref(first)) == ERR_TOO_LARGE
    assert L.flimo_sc_db_add_scan(hip._h, C.byref(_lib.sc_cfg(rings=32, sectors=64)), None, None) == ERR_INVALID
    assert L.flimo_sc_db_get(hip._h, 3, 3, got.ctypes.data) == ERR_INVALID and L.flimo_sc_db_get(hip._h, 0, 1, None) == ERR_INVALID
    assert first.value == 99 and hip.sc_db_size() == 5 and hip.sc_db_shape() == (20, 60) and hip.sc_db_get().tobytes() == got.tobytes()
    with pytest.raises(_lib.FlimoError):
        hip.sc_match(other[:1])
    # a clear, then the new shape
    hip.sc_db_clear()
    assert hip.sc_db_size() == 0 and hip.sc_db_shape() == (0, 0)
    assert hip.sc_db_add(other) == 0 and hip.sc_db_shape() == (32, 64) and hip.sc_db_get().tobytes() == other.tobytes()


# ---- 3. the match --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_the_match_at_every_database_size(hip, shape):
    """Database sizes around the wave's two entries, the workgroup's eight and the default split; one query and five (the tile is
    two); k 1 and 8, above the number of admissible entries at the small sizes: the slots beyond cnt are padded."""
    Q, E, P = base(shape)
    for n in (1, 2, 63, 64, 65, 257):
        hip.sc_db_clear()
        hip.sc_db_add(E[:n])
        for nq in (1, 5):
            for k in (1, 8):
                got = hip.sc_match(Q[:nq], k=k, want_profile=True)
                want = sc.match(Q[:nq], E[:n], k, P=P[:nq, :n])
                sc.same(got, want, f"{shape}: n {n}, nq {nq}, k {k}")
                pad = np.arange(k)[None, :] >= got["cnt"][:, None]
                assert np.all(got["idx"][pad] == -1) and np.all(got["shift"][pad] == -1) and np.all(sc.bits(got["dist"][pad]) == 0)
                assert np.all(np.isnan(got["profile"][pad]))
    if shape[1] > 2:
        assert got["cnt"].tolist()[:4] == [8, 8, 8, 8] and got["cnt"][4] == 0      # (the all-zero query)
        assert got["idx"][1, 0] == 9 and got["shift"][1, 0] == 7 % shape[1]        # (the rolled entry)
        assert 7 not in got["idx"] and 11 not in got["idx"]


def test_identical_entries_come_in_id_order_and_a_roll_is_found(hip):
    Q, E, _ = base()
    D = np.ascontiguousarray(E[:100]).copy()
    D[30:70] = D[30]
    hip.sc_db_add(D)
    for s in (0, 1, 29, 59):
        q = np.roll(D[30], s, axis=1)
        got = hip.sc_match(q, k=8)
        assert got["idx"][0].tolist() == list(range(30, 38)) and np.all(got["shift"][0] == s), s
        assert len(set(sc.bits(got["dist"][0]).tolist())) == 1
        sc.same(got, sc.match(q, D, 8), f"roll {s}", profile=False)
    hip.set_sc_chunk(0, 1)
    got = hip.sc_match(D[30], k=8, first=33)
    assert got["idx"][0].tolist() == list(range(33, 41))


def test_min_cols_max_dist_and_ranges(hip):
    Q, E, P = base()
    hip.sc_db_add(E)
    # min_cols: query 3 has three non-empty columns at most
    for mc in (1, 2, 3, 4, 30, 60):
        sc.same(hip.sc_match(Q, k=8, min_cols=mc, want_profile=True), sc.match(Q, E, 8, min_cols=mc), f"min_cols {mc}")
    assert hip.sc_match(Q[3], k=1, min_cols=4)["cnt"][0] == 0 and hip.sc_match(Q[3], k=1, min_cols=1)["cnt"][0] == 1
    # max_dist one float32 step either side of the distances of query 0's first, second and last entry: none, one, all
    all_ = sc.match(Q[:1], E, 8, P=P[:1])
    full = sc.match(Q[:1], E, 257, P=P[:1])
    d0, d1, dl = all_["dist"][0, 0], all_["dist"][0, 1], full["dist"][0, full["cnt"][0] - 1]
    assert d0 < d1
    for gate, cnt in ((d0, 0), (np.nextafter(d0, F(2)), 1), (d1, 1), (np.nextafter(d1, F(2)), 2), (dl, None), (np.nextafter(dl, F(2)), None)):
        got = hip.sc_match(Q, k=8, max_dist=float(gate), want_profile=True)
        sc.same(got, sc.match(Q, E, 8, max_dist=gate, P=P), f"max_dist {gate!r}")
        assert cnt is None or got["cnt"][0] == cnt
    # ranges that cut the database, are empty, or reach past the end
    for first, n in ((0, 100), (100, 57), (256, 1), (3, 1), (250, 100), (257, 5), (1000, 1), (5, 0), (0, None)):
        got = hip.sc_match(Q, k=8, first=first, n=n, want_profile=True)
        sc.same(got, sc.match(Q, E, 8, first=first, n=n, P=P), f"range {first} + {n}")
        if first >= 257 or n == 0:
            assert not got["cnt"].any()


def test_the_bits_do_not_move_with_chunks_splits_the_other_queries_or_repetition(hip):
    Q, E, P = base()
    hip.sc_db_add(E)
    want = hip.sc_match(Q, k=8, want_profile=True)
    sc.same(want, sc.match(Q, E, 8, P=P), "defaults")
    for chunk in (0, 1, 3):
        for split in (0, 1, 64, 100):
            hip.set_sc_chunk(chunk, split)
            same_bytes(want, hip.sc_match(Q, k=8, want_profile=True), f"chunk {chunk}, split {split}")
    hip.set_sc_chunk(0, 0)
    for i in range(5):      # (alone, and behind a larger call)
        got = hip.sc_match(Q[i], k=8, want_profile=True)
        for name in want:
            assert got[name][0].tobytes() == want[name][i].tobytes(), (i, name)
    same_bytes(want, hip.sc_match(Q, k=8, want_profile=True), "once more")
    assert hip.sc_match(Q, k=3)["idx"].tobytes() == want["idx"][:, :3].tobytes()


def test_trivial_and_rejected_match_calls_leave_the_outputs_alone(hip):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    Q, E, P = base()
    Q = np.ascontiguousarray(Q[:4])
    got = hip.sc_match(Q, k=3, want_profile=True)      # no database
    assert not got["cnt"].any() and np.all(got["idx"] == -1) and np.all(got["shift"] == -1) and np.all(np.isnan(got["profile"]))
    hip.sc_db_add(E[:50])
    idx, dist, shift, cnt = np.full((4, 2), 7, np.int32), np.full((4, 2), 7, F), np.full((4, 2), 7, np.int32), np.full(4, 7, np.int32)
    prof = np.full((4, 2, 60), 7, F)

    def call(q_p=Q.ctypes.data, nq=4, rings=20, sectors=60, first=0, n=50, k=2, min_cols=1, max_dist=INF, cfg=True, idx_p=idx.ctypes.data,
             dist_p=dist.ctypes.data, shift_p=shift.ctypes.data, cnt_p=cnt.ctypes.data):
        m = _lib.ScMatchCfg(k, min_cols, max_dist)
        return L.flimo_sc_match(hip._h, q_p, nq, rings, sectors, first, n, C.byref(m) if cfg else None, idx_p, dist_p, shift_p, cnt_p, prof.ctypes.data)
    for kw in (dict(q_p=None), dict(cfg=False), dict(idx_p=None), dict(dist_p=None), dict(shift_p=None), dict(cnt_p=None), dict(rings=19),
               dict(sectors=59), dict(rings=0), dict(sectors=65), dict(rings=32, sectors=64), dict(k=0), dict(k=9), dict(min_cols=0),
               dict(min_cols=61), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan"))):
        assert call(**kw) == ERR_INVALID, kw
    for kw in (dict(nq=2 ** 31), dict(nq=2 ** 30, k=2), dict(nq=2 ** 28, k=8)):
        assert call(**kw) == ERR_TOO_LARGE, kw
    assert call(nq=0) == 0 and call(nq=0, q_p=None) == 0
    assert np.all(idx == 7) and np.all(dist == 7) and np.all(shift == 7) and np.all(cnt == 7) and np.all(prof == 7)
    assert call() == 0
    sc.same(dict(idx=idx, dist=dist, shift=shift, cnt=cnt, profile=prof), sc.match(Q, E[:50], 2, P=P[:4, :50]), "through ctypes")
    assert L.flimo_set_sc_chunk(None, 1, 1) == ERR_INVALID and L.flimo_sc_db_clear(None) == ERR_INVALID
    hip.set_timing(1)
    hip.sc_match(Q)
    assert hip.sc_last_ms() > 0
    hip.set_timing(0)


# ---- 4. no side effects, the Localizer -----------------------------------------------------------------------------------------------
def test_the_calls_touch_neither_the_map_nor_the_scan_nor_a_later_pass():
    """Against a twin context that never makes the calls: the map, the scan, knn_k and the sums of three passes have the twin's
    bytes.  The database survives an insert, a crop and a clear of the map."""
    from fast_limo_amd import _lib
    mp = fpc.scene()
    scan = np.ascontiguousarray(mp[::3] + F([0.01, -0.01, 0.005]))
    mcfg = _lib.default_match_cfg(**CAPS)
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    Q, E, P = base()
    c = sc.cfg(max_range=10.0, z_offset=1.0)

    def run(calling):
        h = _lib.HipCtx(0)
        try:
            h.map_config(0.2, 2, True, 0.0)
            h.map_add(mp, stamp=0.5)
            h.scan_set(scan)
            out = [h.match_reduce(x, mcfg)]
            if calling:
                h.sc_db_add(E[:70])
                assert h.scan_context(**c)[1] > 0 and h.sc_db_add_scan(**c) == 70
                assert np.all(h.sc_match(Q[:4], k=8, want_profile=True)["cnt"] == 8)
            out.append(h.match_reduce(x, mcfg))
            if calling:
                h.set_sc_chunk(1, 7)
                h.sc_match(Q, k=2)
                h.sc_db_get()
            out.append(h.match_reduce(x, mcfg))
            knn = h.knn_k(scan[:64], 8)
            res = out, h.map_size(), h.map_points().copy(), h.scan_get().copy(), knn
            if calling:
                kept = h.sc_db_get().copy()
                h.map_add(mp[:100] + F(50.0), stamp=0.6)
                h.map_crop_box((-1.0, -1.0, -1.0), (2.0, 2.0, 2.0))
                h.map_clear()
                assert h.map_size() == 0 and h.sc_db_size() == 71 and h.sc_db_get().tobytes() == kept.tobytes()
                sc.same(h.sc_match(Q, k=8, n=70), sc.match(Q, E[:70], 8, P=P[:, :70]), "after the map went", profile=False)
            return res
        finally:
            h.close()

    (plain, pn, pm, ps, pk), (called, cn, cm, cs, ck) = run(False), run(True)
    assert pn == cn == len(mp) and pm.tobytes() == cm.tobytes() == mp.tobytes() and ps.tobytes() == cs.tobytes() == scan.tobytes()
    for a, b in zip(pk, ck):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(plain, called):
        assert a[2] == b[2] > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_localizer_forwards(hip):
    from fast_limo_amd import api
    Q, E, _ = base()
    c = sc.cfg()
    cloud = sc.random_cloud(4, 2000)
    hip.sc_db_add(E)
    hip.scan_set(cloud)
    first, desc = hip.sc_match(Q, k=4, want_profile=True), hip.scan_context(**c)
    loc = api.Localizer(api.default_cfg())
    try:
        assert loc.hip.sc_db_size() == 0 and not loc.sc_match(Q, k=4)["cnt"].any()
        assert loc.sc_db_add(E) == 0 and loc.hip.sc_db_size() == len(E) and loc.hip.sc_db_shape() == (20, 60)
        same_bytes(first, loc.sc_match(Q, k=4, want_profile=True), "Localizer with no map")
        assert loc.sc_db_get(5, 3).tobytes() == E[5:8].tobytes()
        loc.map_add(cloud)
        same_bytes(first, loc.sc_match(Q, k=4, want_profile=True), "Localizer with a map")
        loc.hip.scan_set(cloud)
        got = loc.scan_context(**c)
        assert got[0].tobytes() == desc[0].tobytes() and got[1] == desc[1]
        assert loc.sc_db_add_scan(**c) == len(E) and loc.sc_db_get(len(E), 1)[0].tobytes() == desc[0].tobytes()
        with pytest.raises(api.FlimoError):
            loc.sc_match(Q, k=9)
        loc.sc_db_clear()
        assert loc.hip.sc_db_size() == 0
    finally:
        loc.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
# scan_align from the restatement's guess (the keyframe's position, up to 1 m off, yaw within a sector): measured on an MI355X
# and recorded in profiles/scan_context/README.md -- the worst of the 20 queries ends 1.86 mm and 0.0083 degrees from the truth;
# the bars are twice that (tighter than scan_align's documented 1 cm / 0.1 degrees: the map is made of the very points swept).
END_POS_BAR, END_ROT_BAR_DEG = 2 * 0.00186, 2 * 0.0083


def test_place_relocalize_finds_every_query_of_the_scene():
    """The map is the union of the keyframes' sweeps in the world frame, the database their descriptors by sc_db_add_scan;
    api.place_relocalize of every query sweep picks the restatement's keyframe and shift and ends within the bars above."""
    from fast_limo_amd import _lib, api
    s = sc.scene()
    K, Qd = sc.scene_descs()
    want = sc.match(Qd, K, 4)
    world = []
    for x, body in zip(s["kf_x26"], s["kf_sweep"]):
        yaw, cs = sc.yaw_of(x), body.astype(np.float64)
        c_, s_ = math.cos(yaw), math.sin(yaw)
        world.append(np.stack([c_ * cs[:, 0] - s_ * cs[:, 1] + x[0], s_ * cs[:, 0] + c_ * cs[:, 1] + x[1], cs[:, 2] + x[2]], axis=1).astype(F))
    h = _lib.HipCtx(0)
    try:
        h.map_config(0.2, 2, True, 0.0)
        for w in world:
            h.map_add(w, stamp=0.5)
        for i, body in enumerate(s["kf_sweep"]):
            h.scan_set(body)
            assert h.sc_db_add_scan(**sc.SCENE_CFG) == i
        assert h.sc_db_get().tobytes() == K.tobytes()
        worst = [0.0, 0.0]
        for i, body in enumerate(s["q_sweep"]):
            h.scan_set(body)
            out = api.place_relocalize(h, s["kf_x26"], _lib.sc_cfg(**sc.SCENE_CFG), k=4, align=dict(iters=15))
            assert out["desc"].tobytes() == Qd[i].tobytes()
            for name in ("idx", "shift", "cnt"):
                assert np.array_equal(out["match"][name][0], want[name][i]), (i, name)
            assert out["match"]["idx"][0, 0] == s["truth"][i]
            dt, dr = cc.pose_error(out["x26"], s["q_x26"][i])
            worst = [max(worst[0], dt), max(worst[1], dr)]
            print(f"query {i}: keyframe {out['match']['idx'][0, 0]}, shift {out['match']['shift'][0, 0]}, ranked first "
                  f"{out['fitness']['order'][0]}, aligned {dt * 1e3:.2f} mm {dr:.4f} deg")
        print(f"worst: {worst[0] * 1e3:.2f} mm {worst[1]:.4f} deg")
        assert worst[0] <= END_POS_BAR and worst[1] <= END_ROT_BAR_DEG
    finally:
        h.close()
