"""The map index where its escape pool runs out.

A segment (8 fine x columns of a row) with a column of more than 15 points is an ESCAPE: its entry points at a slot of eight
cumulative counts in the index's escape pool.  An escape in the FIRST segment of an x-tile (other than tile 0) takes two slots:
its own entry and the closing entry of the tile to its left.  So 16 points can cost two slots -- n / 8 in the worst case --
while the pool starts at (capacity of the point buffer) / 16 + 64 slots.  The inputs below are that worst case: 16-point
clusters, each inside one fine column right behind a tile boundary, enough of them that the slots they need exceed that first
size of the pool by a quarter.  A full layout that ran out of slots used to leave the entry zero, and the points behind it vanished
from every search without an error; it now grows the pool and writes its entries again.

The clusters are placed by the layout the library actually made (flimo_map_index_layout), read from a probe context that holds
the sparse "frame" alone: clusters strictly inside the frame's box leave the bounding box, and with it the layout, as it is
(asserted).  Every comparison is bit for bit against numpy brute force over ctx.map_points() (knn_k_common / radius_common:
float32 squared distances, order (distance bits, insertion index)); every cluster is queried and every query is compared.
test_builder_places_clusters_as_intended checks the placement arithmetic without a device."""
import numpy as np
import pytest

from knn_k_common import brute_knn
from radius_common import bits, brute_force_multi, sorted_order, sqdist_f32
import normals_common as nc

INF = float("inf")
PER = 16                                   # points of a cluster: one more than a nibble counts
FRAME_LO, FRAME_HI = (0.0, 0.0, 0.0), (330.0, 21.0, 2.5)
ROWS_ISSUE, ROWS_SMALL = 160, 80           # x 5 tile boundaries: 800 clusters (12 800 points) and 400 (6 400)
X_LOW, X_SPAN = 0.005, 0.002               # a cluster's x: [column edge + 5 mm, + 7 mm]
Q_OUT = 0.010                              # the outer queries: 1 cm outside the cluster on either side in x
GATE, R_IN, R_ROWS = 0.012, 0.005, 0.6     # the k = 16 gate; a radius inside a cluster; one that reaches the rows next to it
F = np.float32


# ---- the arithmetic of the index in numpy (float32, the expression of column_key in flimo_map.hip) ----
def columns(p, lay):
    """(column, row y, row z) of points p [n, 3] float32 under a layout (dict of map_index_layout)."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    inv = F(1.0) / F(lay["cell"])
    xs = lay["xs"]
    tx = (p[:, 0] - F(lay["ox"])) * inv
    assert tx.dtype == np.float32
    cx = np.floor(np.clip(tx * F(xs), F(-1.0e9), F(1.0e9))).astype(np.int64) - lay["six"] * xs
    cy = np.floor((p[:, 1] - F(lay["oy"])) * inv).astype(np.int64) - lay["siy"]
    cz = np.floor((p[:, 2] - F(lay["oz"])) * inv).astype(np.int64) - lay["siz"]
    return (np.clip(cx, 0, lay["nx"] * xs - 1), np.clip(cy, 0, lay["ny"] - 1), np.clip(cz, 0, lay["nz"] - 1))


def on_an_edge(p, lay, margin=1e-3):
    """Points closer than `margin` (in columns / cells, float64) to a column or cell edge: none may be."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    t = np.stack([(p[:, 0] - float(lay["ox"])) / float(lay["cell"]) * lay["xs"], (p[:, 1] - float(lay["oy"])) / float(lay["cell"]),
                  (p[:, 2] - float(lay["oz"])) / float(lay["cell"])], 1)
    return int((np.abs(t - np.round(t)) < margin).sum())


def slots_needed(p, lay):
    """Escape slots a full layout of points p takes: one per (row, segment) with a column of more than 15 points, one more when
    that segment is the first of an x-tile other than tile 0 (the closing entry of the tile to its left)."""
    cx, cy, cz = columns(p, lay)
    nxs = lay["nx"] * lay["xs"] + 1
    key = (cz * lay["ny"] + cy) * nxs + cx
    u, cnt = np.unique(key, return_counts=True)
    big = u[cnt > 15]
    seg = np.unique((big // nxs) * nxs + ((big % nxs) >> 3))        # (row, segment) pairs
    sg = seg % nxs
    return int(seg.size + ((sg != 0) & ((sg & ((1 << lay["ts"]) - 1)) == 0)).sum())


def first_pool(n):
    """Slots of the pool a first batch of n points used to get for good: the point buffer's capacity / 16 + 64."""
    return (n + n // 4 + 1024) // 16 + 64


def geometry(lay):
    return {k: v for k, v in lay.items() if k not in ("escape_slots", "escape_slots_taken", "points")}


# ---- the input ----
def frame(lo=FRAME_LO, hi=FRAME_HI, inside=56, seed=3):
    """The sparse batch that fixes the bounding box: the box's corners and a few points inside."""
    lo, hi = np.float64(lo), np.float64(hi)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    rs = np.random.RandomState(seed)
    return np.concatenate([corners, lo + (hi - lo) * rs.uniform(0.05, 0.95, (inside, 3))]).astype(F)


def build(lay, n_rows, lo=FRAME_LO, hi=FRAME_HI, seed=11):
    """16-point clusters in column (t << ts) * 8 of `n_rows` rows, for every x-tile t >= 1 whose first column lies inside the box
    [lo, hi]: dict of pts [16 S, 3] (cluster after cluster), centres [S, 3], col / cy / cz [S] (where each is meant to land)."""
    cell, xs, ts = float(lay["cell"]), lay["xs"], lay["ts"]
    o = np.float64([lay["ox"], lay["oy"], lay["oz"]])
    si = np.array([lay["six"], lay["siy"], lay["siz"]])
    tile_cols = 8 << ts
    cols = [t * tile_cols for t in range(1, lay["ntx"])]
    edge = lambda c: o[0] + (c + si[0] * xs) * (cell / xs)            # world x of the low edge of column c
    cols = [c for c in cols if c < lay["nx"] * xs and lo[0] + 0.1 < edge(c) and edge(c) + cell / xs < hi[0] - 0.1]
    rows = [(y, z) for z in range(lay["nz"]) for y in range(lay["ny"])
            if lo[1] < o[1] + (y + si[1]) * cell and o[1] + (y + si[1] + 1) * cell < hi[1]
            and lo[2] < o[2] + (z + si[2]) * cell and o[2] + (z + si[2] + 1) * cell < hi[2]]
    assert len(rows) >= n_rows and cols, (len(rows), n_rows, cols)
    rows = rows[:n_rows]
    rs = np.random.RandomState(seed)
    g = (np.arange(4) - 1.5) * 0.003                                  # 4 x 4 points 3 mm apart in y and z around the row's axis
    dy, dz = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    pts, centres, where = [], [], []
    for (y, z) in rows:
        for c in cols:
            x0 = edge(c)
            yc, zc = o[1] + (y + si[1] + 0.5) * cell, o[2] + (z + si[2] + 0.5) * cell
            pts.append(np.stack([x0 + X_LOW + rs.uniform(0.0, X_SPAN, PER), yc + dy, zc + dz], 1))
            centres.append([x0 + X_LOW + 0.5 * X_SPAN, yc, zc])
            where.append((c, y, z))
    where = np.array(where)
    return dict(pts=np.concatenate(pts).astype(F), centres=np.array(centres).astype(F), col=where[:, 0], cy=where[:, 1], cz=where[:, 2])


def queries(centres):
    """Per cluster its centre and a point 1 cm outside it on either side in x: the lower one lies beyond the tile boundary."""
    d = np.zeros((1, 3), F)
    d[0, 0] = 0.5 * X_SPAN + Q_OUT
    return np.concatenate([centres, centres - d, centres + d]).astype(F)


def check_placement(sc, lay, extra, pool_n=None, bound=True):
    """The conditions on the input, in numpy: every cluster in its column and row, no point on an edge, the slots the whole map
    needs (returned) 25 % above the pool a first batch of its size gets (`bound`).  extra: the other points the index holds."""
    cx, cy, cz = columns(sc["pts"], lay)
    S = sc["centres"].shape[0]
    assert np.array_equal(cx, np.repeat(sc["col"], PER)) and np.array_equal(cy, np.repeat(sc["cy"], PER)) and np.array_equal(cz, np.repeat(sc["cz"], PER))
    ts = lay["ts"]
    assert np.all((sc["col"] & ((8 << ts) - 1)) == 0) and np.all(sc["col"] > 0)
    assert on_an_edge(sc["pts"], lay) == 0
    q = queries(sc["centres"])
    qx = columns(q, lay)[0]
    assert np.array_equal(qx[:S], sc["col"]) and np.array_equal(qx[S:2 * S], sc["col"] - 1) and np.array_equal(qx[2 * S:], sc["col"])
    allp = np.concatenate([extra, sc["pts"]])
    need, n = slots_needed(allp, lay), allp.shape[0] if pool_n is None else pool_n
    assert need == slots_needed(sc["pts"], lay) == 2 * S, (need, S)
    assert n <= 40000 and (not bound or need >= 1.25 * first_pool(n)), (need, n, first_pool(n))
    return need


def test_builder_places_clusters_as_intended():
    """No device: the placement arithmetic under a layout of the kind the library makes for the frame (cell 0.5 m, two columns per
    cell, tiles of 32 segments), and what the yardsticks make of the input."""
    lay = dict(valid=True, ox=F(-6.25), oy=F(-4.25), oz=F(-2.25), cell=F(0.5), xs=2, six=0, siy=0, siz=0, nx=690, ny=60, nz=15,
               ts=5, ty=5, tz=3, ntx=6, nty=2, ntz=3, points=64, escape_slots=0, escape_slots_taken=0)
    fr = frame()
    assert fr.min(0).tolist() == list(FRAME_LO) and fr.max(0).tolist() == list(FRAME_HI)
    for n_rows, S in ((ROWS_ISSUE, 800), (ROWS_SMALL, 400)):
        sc = build(lay, n_rows)
        assert sc["centres"].shape[0] == S and sc["pts"].shape[0] == PER * S
        assert np.all(sc["pts"] > fr.min(0)) and np.all(sc["pts"] < fr.max(0))            # strictly inside the frame's box
        need = check_placement(sc, lay, fr)
        print(f"{S} clusters, {fr.shape[0] + PER * S} points: {need} slots against a first pool of {first_pool(fr.shape[0] + PER * S)}")
    # 76 rows are the fewest that meet the 25 % condition (exactly); 75 no longer do
    small = build(lay, 75)
    assert 2 * small["centres"].shape[0] < 1.25 * first_pool(fr.shape[0] + small["pts"].shape[0])
    # the counter itself: a column of 15 points is no escape, one of 16 in another segment takes one slot
    lone = np.tile(sc["pts"][:1], (31, 1))
    lone[15:, 0] += F(8.0)
    assert slots_needed(lone[:15], lay) == 0 and slots_needed(lone, lay) == 1
    # the yardstick of the normals keeps every centre (a cluster is a thin plate across x)
    mp = np.concatenate([fr, sc["pts"]])
    ref = nc.reference(sc["centres"][::7], mp, PER)
    assert np.all(ref["cnt"] == PER) and nc.left_out_fraction(ref) == 0.0
    assert np.all(np.abs(np.abs(ref["normal"][:, 0]) - 1.0) < 0.05)


# ---- GPU ----
def _ctx(env=None, monkeypatch=None):
    from fast_limo_amd import _lib
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                 # (read when the context is made)
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, False, 0.0)           # nothing is down-sampled; the default cell of 0.5 m
    return ctx


def _probe(fr, level=0, env=None, monkeypatch=None):
    """The layout the library makes for the frame alone."""
    ctx = _ctx(env, monkeypatch)
    try:
        ctx.map_add(fr)
        assert ctx.map_size() == fr.shape[0]
        return ctx.map_index_layout(level)
    finally:
        ctx.close()


_BRUTE = {}


def _brute(mp, q, tag):
    """The yardsticks over one map and one set of queries, computed once: the first 64 in the unique order (the first 5 and the
    gated 16 are read off it: a gate admits a prefix of that order), and the two radii."""
    key = (mp.tobytes(), q.tobytes())
    if key not in _BRUTE:
        idx, sqd, cnt = brute_knn(q, mp, 64)
        with np.errstate(over="ignore"):
            g2 = F(F(GATE) * F(GATE))
        adm = np.minimum(((sqd < g2) & (idx >= 0)).sum(1), 16)
        assert np.all(adm < 64)                                  # (the 64 reach beyond the gate: nothing admitted lies behind them)
        keep = np.arange(16)[None, :] < adm[:, None]
        _BRUTE[key] = dict(idx=idx, sqd=sqd, cnt=cnt, gidx=np.where(keep, idx[:, :16], -1), gsqd=np.where(keep, sqd[:, :16], F(0)),
                           gcnt=adm.astype(np.int32), radius=brute_force_multi(q, mp, [R_IN, R_ROWS]))
    return _BRUTE[key]


def _wrong_queries(ctx, mp, q, tag, radii=True):
    """Number of queries (of 3 per cluster) for which some search differs from brute force, per kind of search."""
    b = _brute(mp, q, tag)
    bad = {}
    i5, s5, c5 = ctx.knn(q, 5)
    # flimo_knn: distances and count exactly; among exactly tied distances it keeps the candidate the reference meets first, so a
    # neighbour is checked by being a stored point at exactly that distance, each one once
    ok5 = (c5 == np.minimum(b["cnt"], 5)) & np.all(bits(s5) == bits(b["sqd"][:, :5]), 1) & np.all(i5 >= 0, 1)
    d5 = np.stack([sqdist_f32(q[j:j + 1], mp[np.maximum(i5[j], 0)])[0] for j in range(q.shape[0])])
    ok5 &= np.all(bits(d5) == bits(s5), 1) & np.array([len(set(r)) == 5 for r in i5.tolist()])
    bad["knn 5"] = ~ok5
    i64, s64, c64 = ctx.knn_k(q, 64)
    bad["knn_k 64"] = ~((c64 == b["cnt"]) & np.all(i64 == b["idx"], 1) & np.all(bits(s64) == bits(b["sqd"]), 1))
    ig, sg, cg = ctx.knn_k(q, 16, GATE)
    bad["knn_k 16 gated"] = ~((cg == b["gcnt"]) & np.all(ig == b["gidx"], 1) & np.all(bits(sg) == bits(b["gsqd"]), 1))
    if radii:
        for r, (off, idx, sqd) in zip((R_IN, R_ROWS), b["radius"]):
            bi, bs = sorted_order(off, idx, sqd)
            goff, gi, gs = ctx.radius_search(q, r, sorted=True)
            w = np.diff(goff.astype(np.int64)) != np.diff(off.astype(np.int64))
            if not w.any():
                qid = np.repeat(np.arange(q.shape[0]), np.diff(off.astype(np.int64)))
                w[qid[(gi != bi) | (bits(gs) != bits(bs))]] = True
            bad[f"radius {r}"] = w
    print(f"{tag}: {q.shape[0]} queries over {mp.shape[0]} points; wrong: " + ", ".join(f"{k} {int(v.sum())}" for k, v in bad.items()))
    return bad


def _check_pass(ctx, oracle, mp, q, tag, brute=True):
    """A registration pass over the queries at the identity pose: its fast path reads a range's two ends from two NEIGHBOURING
    entries of one tile -- for a range that crosses into the next tile the second is the tile's closing entry, the second of the
    two slots a cluster takes.  Match records against the oracle's (test_match_records_bit_exact), the 5 distances against brute
    force as well; a pass with the previous pass's bound and the one-launch layout must find the same matches."""
    from common import CAPS
    from fast_limo_amd import _lib
    oc = oracle.Octree(0.2, False)
    oc.update(mp)
    x0 = oracle.identity_x26()
    recs, H, h, _ = oracle.match_H(oc, oracle.default_cfg(num_threads=4, **CAPS), x0, q)
    cfg = _lib.default_match_cfg(**CAPS)
    ctx.scan_set(q)
    p1 = ctx.match_reduce(x0, cfg)
    p2 = ctx.match_reduce(x0, cfg)
    ctx.set_debug_records(True)
    HTH, HTh, M = ctx.match_reduce(x0, cfg)
    g = ctx.match_fetch()
    ctx.set_debug_records(False)
    vg, vo = g["valid"] > 0, recs["is_plane"] > 0
    b5 = brute_knn(q, mp, 5)[1] if brute else oc.knn(q, 5, num_threads=8)[1]
    wrong = ~np.all(bits(g["sqd"]) == bits(b5), 1)
    print(f"{tag}, pass: {q.shape[0]} queries, {int(vo.sum())} planes in the oracle, {int(vg.sum())} here; 5 distances differ from {'brute force' if brute else 'the oracle'} at {int(wrong.sum())}")
    assert not wrong.any(), f"{tag}: the pass's 5 distances differ at {int(wrong.sum())} of {wrong.size} queries"
    np.testing.assert_array_equal(g["p_global"], q)
    np.testing.assert_array_equal(vg, vo)
    assert p1[2] == p2[2] == M == H.shape[0] == int(vg.sum()) and M >= q.shape[0] // 3, (p1[2], p2[2], M, H.shape, int(vg.sum()))
    np.testing.assert_array_equal(g["sqd"][vg], recs["sqd"][vg])
    np.testing.assert_array_equal(g["n"][vg], recs["n"][vg])
    np.testing.assert_array_equal(g["H"][vg].astype(np.float64), H)
    for p in (p1, p2, (HTH, HTh, M)):
        np.testing.assert_allclose(p[0], H.T @ H, rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(p[1], H.T @ h, rtol=1e-12, atol=1e-9)


def _check_searches(ctx, expect, sc, tag, normals=True, radii=True, oracle=None):
    mp = ctx.map_points()
    assert np.array_equal(bits(mp), bits(expect)), tag + ": the stored points are not the input in its order"
    q = queries(sc["centres"])
    if oracle is not None:
        _check_pass(ctx, oracle, mp, q, tag)
    bad = _wrong_queries(ctx, mp, q, tag, radii)
    for kind, w in bad.items():
        assert not w.any(), f"{tag}: {kind}: {int(w.sum())} of {w.size} queries differ from brute force"
    if normals:
        nc.check(ctx.normals(sc["centres"], PER), nc.reference(sc["centres"], mp, PER), tag + ", normals")
    mm = ctx.grid_selfcheck()[0]
    assert mm == 0, f"{tag}: the index differs from a fresh sort at {mm} places"


def _layout_after(ctx, lay0, need, tag, exact=True):
    lay = ctx.map_index_layout(0)
    assert geometry(lay) == geometry(lay0), (tag, lay, lay0)
    print(f"{tag}: {need} escape slots needed, {lay['escape_slots_taken']} taken, pool of {lay['escape_slots']}")
    if exact:
        assert lay["escape_slots_taken"] == need, (tag, lay, need)
    assert lay["escape_slots"] >= need, (tag, lay, need)
    return lay


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [ROWS_ISSUE, ROWS_SMALL])
def test_first_layout(built, oracle, n_rows):
    """Frame + clusters as ONE batch: the first layout itself needs 2 slots per 16 points.
    Measured once before the layout grew its pool (the 800-cluster input, 12 864 points): 1 600 slots asked for, 1 133 in the
    pool.  The workgroups of the rows run side by side and write a segment's own entry before the closing entry of the tile
    to its left, so the 467 entries left unwritten were closing entries: all 2 400 queries of every search here agreed with
    brute force, the self-check counted 3 892 mismatches, and the registration pass -- whose fast path reads a range's end
    from the closing entry -- read a range that ended before it began and stopped with an illegal memory access.  On another
    machine the unwritten entries may as well be the segments' own, and then the searches miss the cluster."""
    fr = frame()
    lay0 = _probe(fr)
    sc = build(lay0, n_rows)
    need = check_placement(sc, lay0, fr)
    allp = np.concatenate([fr, sc["pts"]])
    oc = oracle.Octree(0.2, False)
    oc.update(allp)
    ctx = _ctx()
    try:
        ctx.map_add(allp)
        assert ctx.map_size() == oc.size() == allp.shape[0]
        _layout_after(ctx, lay0, need, f"first layout, {n_rows} rows")
        _check_searches(ctx, allp, sc, f"first layout, {n_rows} rows", oracle=oracle)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_merges_run_out_then_the_relayout(built, oracle):
    """The frame first, the clusters in 8 batches (the clusters of a row spread over the batches: its row moves again and again):
    an insert finds the pool exhausted, and the full layout that answers it must be complete."""
    fr = frame()
    lay0 = _probe(fr)
    sc = build(lay0, ROWS_SMALL)
    need = check_placement(sc, lay0, fr)
    S = sc["centres"].shape[0]
    oc = oracle.Octree(0.2, False)
    ctx = _ctx()
    try:
        ctx.map_add(fr); oc.update(fr)
        cap0, relay0 = ctx.map_index_layout(0)["escape_slots"], ctx.map_index_bytes()["tile_pool_relayouts"]
        order = np.concatenate([np.arange(b, S, 8) for b in range(8)])
        bounds = np.cumsum([0] + [np.arange(b, S, 8).size for b in range(8)])
        stored = fr
        caps = []
        for b in range(8):
            mine = order[bounds[b]:bounds[b + 1]]
            batch = sc["pts"].reshape(S, PER, 3)[mine].reshape(-1, 3)
            ctx.map_add(batch); oc.update(batch)
            stored = np.concatenate([stored, batch])
            assert ctx.map_size() == oc.size() == stored.shape[0]
            sofar = dict(centres=sc["centres"][order[:bounds[b + 1]]])
            _check_searches(ctx, stored, sofar, f"batch {b + 1} of 8", normals=False, radii=False)
            lay = ctx.map_index_layout(0)
            assert geometry(lay) == geometry(lay0)
            caps.append(lay["escape_slots"])
        relay = ctx.map_index_bytes()["tile_pool_relayouts"] - relay0
        print(f"8 batches: pool {cap0} -> {caps} slots, {relay} relayouts after an insert ran out, {need} slots needed")
        assert relay >= 1 or caps[-1] > cap0
        assert caps[-1] >= need
        _check_searches(ctx, stored, dict(centres=sc["centres"][order]), "after the 8 batches", oracle=oracle)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"FLIMO_FULL_REBUILD": "1"}, {"FLIMO_ROW_SLACK": "0"}], ids=["full_rebuild", "packed_rows"])
def test_forced_full_layouts(built, oracle, monkeypatch, env):
    """The first layout's checks when every insert lays the whole map out afresh (fed in two batches: the second layout is one
    over a map), and with the packed layout (no room behind the rows)."""
    fr = frame()
    lay0 = _probe(fr, env=env, monkeypatch=monkeypatch)
    sc = build(lay0, ROWS_SMALL)
    need = check_placement(sc, lay0, fr)
    allp = np.concatenate([fr, sc["pts"]])
    half = fr.shape[0] + PER * (sc["centres"].shape[0] // 2)
    oc = oracle.Octree(0.2, False)
    ctx = _ctx(env, monkeypatch)
    try:
        for part in (allp[:half], allp[half:]):
            ctx.map_add(part); oc.update(part)
            assert ctx.map_size() == oc.size()
        assert ctx.map_size() == allp.shape[0]
        # (with FLIMO_FULL_REBUILD the second insert is a full layout: the slots are counted from zero; otherwise it is a merge
        #  or the layout that follows it, and the count is the layout's or more)
        _layout_after(ctx, lay0, need, str(env), exact="FLIMO_FULL_REBUILD" in env)
        _check_searches(ctx, allp, sc, str(env), oracle=oracle)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_after_a_crop(built, oracle):
    """A crop ends in a full layout with a fresh origin.  The other way round: the crop box is chosen first (the frame's box), the
    layout of the KEPT frame is probed, the clusters are placed for it, and sparse points far out in y join the batch; the crop
    removes exactly those."""
    fr = frame()
    lay_kept = _probe(fr)
    sc = build(lay_kept, ROWS_SMALL)
    rs = np.random.RandomState(4)
    far = (np.float64(FRAME_LO) + (np.float64(FRAME_HI) - np.float64(FRAME_LO)) * rs.uniform(0.1, 0.9, (32, 3)) + [0.0, 80.0, 0.0]).astype(F)
    need = check_placement(sc, lay_kept, fr, pool_n=fr.shape[0] + sc["pts"].shape[0] + far.shape[0])
    kept = np.concatenate([fr, sc["pts"]])
    allp = np.concatenate([fr, far, sc["pts"]])
    ctx = _ctx()
    try:
        ctx.map_add(allp)
        assert ctx.map_size() == allp.shape[0]
        assert geometry(ctx.map_index_layout(0)) != geometry(lay_kept)          # the far points stretched this one
        assert ctx.grid_selfcheck()[0] == 0
        removed = ctx.map_crop_box(FRAME_LO, FRAME_HI)
        oc = oracle.Octree(0.2, False)                                          # clear() + initialize(kept)
        oc.update(kept)
        assert removed == far.shape[0] and ctx.map_size() == oc.size() == kept.shape[0]
        _layout_after(ctx, lay_kept, need, "after the crop")
        _check_searches(ctx, kept, sc, "after the crop", oracle=oracle)
    finally:
        ctx.close()


# ---- the second level over a crowded region: its own grid (a quarter of the cell, one column per cell), its own pool ----
FINE_ENV = {"FLIMO_FINE": "1", "FLIMO_FINE_THRESHOLD": "32", "FLIMO_FINE_MIN_POINTS": "0"}
FINE_ROWS = 400                            # x 3 tile boundaries of the fine grid: 1 200 clusters, 19 200 points


ANCHOR_LO, ANCHOR_HI = (40, 12, 5), (260, 24, 8)      # main cells


def anchors(lay, c_lo=ANCHOR_LO, c_hi=ANCHOR_HI, per=40, seed=6):
    """Two main cells with `per` points each (more than the threshold: crowded), at opposite corners of the region the second
    level is to cover; the box of the crowded cells -- and with it the fine grid -- is theirs.  Returns the points and the world
    box strictly between the two clouds' extremes (what lies in it adds no cell outside that box)."""
    cell = float(lay["cell"])
    o = np.float64([lay["ox"], lay["oy"], lay["oz"]])
    si = np.array([lay["six"], lay["siy"], lay["siz"]])
    rs = np.random.RandomState(seed)
    a = [(o + (np.array(c) + si + 0.5) * cell) + rs.uniform(-0.1, 0.1, (per, 3)) for c in (c_lo, c_hi)]
    a = np.concatenate(a).astype(F)
    cx, cy, cz = columns(a, lay)
    got = np.stack([cx // lay["xs"], cy, cz], 1)
    assert np.all(got[:per] == c_lo) and np.all(got[per:] == c_hi)
    return a, a[:per].max(0).astype(np.float64), a[per:].min(0).astype(np.float64)


def inside(p, lay):
    """Points that lie inside a grid's extent (columns() clamps the others to its border)."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    inv = F(1.0) / F(lay["cell"])
    t = np.stack([np.floor(((p[:, 0] - F(lay["ox"])) * inv) * F(lay["xs"])) - lay["six"] * lay["xs"], np.floor((p[:, 1] - F(lay["oy"])) * inv) - lay["siy"],
                  np.floor((p[:, 2] - F(lay["oz"])) * inv) - lay["siz"]], 1)
    return np.all((t >= 0) & (t < np.array([lay["nx"] * lay["xs"], lay["ny"], lay["nz"]])), 1)


@pytest.mark.gpu
def test_second_level(built, oracle, monkeypatch):
    """The second level's index is a full layout of its own, with a pool of (m + m / 2 + 4096) / 16 + 64 slots for the m points
    of the region.  The region is stretched along x (two crowded anchor cells 110 m apart) so that the fine grid has four x-tiles;
    the clusters sit behind its three tile boundaries, inside the part where the second level settles the queries.  With n <=
    40 000 the slots needed can exceed that pool by a fifth at most (2 S against 1.5 S + 320: a quarter takes 3 300 clusters,
    52 800 points); this input is 13 % above it.  5-NN and a registration pass's match records against the oracle."""
    fr = frame()
    lay0 = _probe(fr, env=FINE_ENV, monkeypatch=monkeypatch)
    anc, in_lo, in_hi = anchors(lay0)
    base = np.concatenate([fr, anc])
    ctx = _ctx(FINE_ENV, monkeypatch)
    try:
        ctx.map_add(base)
        assert geometry(ctx.map_index_layout(0)) == geometry(lay0)
        f0 = ctx.map_index_layout(1)
    finally:
        ctx.close()
    assert f0["valid"] and f0["xs"] == 1 and f0["ntx"] >= 2 and f0["cell"] == lay0["cell"] / F(4), f0
    cf = float(f0["cell"])
    o = np.float64([f0["ox"], f0["oy"], f0["oz"]])
    lo = np.maximum(in_lo, o + np.float64(f0["qlo"]) * cf)
    hi = np.minimum(in_hi, o + (np.float64(f0["qhi"]) + 1.0) * cf)
    sc = build(f0, FINE_ROWS, lo, hi)
    q = queries(sc["centres"])
    qc = np.stack(columns(q, f0), 1)
    assert np.all(qc >= np.array(f0["qlo"])) and np.all(qc <= np.array(f0["qhi"]))          # every query is the second level's to settle
    # what the second level holds beside the clusters: the points of the main cells of the crowded box and one cell around it
    bx, by, bz = columns(base, lay0)
    bc = np.stack([bx // lay0["xs"], by, bz], 1)
    near = np.all((bc >= np.array(ANCHOR_LO) - 1) & (bc <= np.array(ANCHOR_HI) + 1), 1)
    assert np.all(inside(base[near], f0))
    held = base[near]
    need = check_placement(sc, f0, held, bound=False)
    m = held.shape[0] + sc["pts"].shape[0]
    assert need > (m + m // 2 + 4096) // 16 + 64, (need, m)
    allp = np.concatenate([base, sc["pts"]])
    assert allp.shape[0] <= 40000
    oc = oracle.Octree(0.2, False)
    oc.update(allp)
    ctx = _ctx(FINE_ENV, monkeypatch)
    try:
        ctx.map_add(allp)
        assert ctx.map_size() == oc.size() == allp.shape[0]
        assert geometry(ctx.map_index_layout(0)) == geometry(lay0)
        f1 = ctx.map_index_layout(1)
        assert geometry(f1) == geometry(f0), (f1, f0)
        print(f"second level: {f1['points']} points, {f1['ntx']} x-tiles, {need} escape slots needed, {f1['escape_slots_taken']} taken, pool of "
              f"{f1['escape_slots']} (first size {(m + m // 2 + 4096) // 16 + 64})")
        assert f1["points"] == m and f1["escape_slots_taken"] == need and f1["escape_slots"] >= need, (f1, m, need)
        mp = ctx.map_points()
        assert np.array_equal(bits(mp), bits(allp))
        i5, s5, c5 = ctx.knn(q, 5)
        osqd, ocnt = oc.knn(q, 5, num_threads=8)[1:3]
        assert np.all(c5 == 5) and np.all(ocnt == 5)
        np.testing.assert_array_equal(bits(s5), bits(osqd))
        d5 = np.stack([sqdist_f32(q[j:j + 1], mp[i5[j]])[0] for j in range(q.shape[0])])      # the neighbours are stored points at those distances
        np.testing.assert_array_equal(bits(d5), bits(s5))
        passes0 = ctx.fine_stats()["passes"]
        _check_pass(ctx, oracle, mp, q, "second level", brute=False)
        fs = ctx.fine_stats()
        assert fs["active"] and fs["points"] == m and fs["passes"] >= passes0 + 3, fs
        assert ctx.grid_selfcheck()[0] == 0
    finally:
        ctx.close()
