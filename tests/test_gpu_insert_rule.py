"""GPU suite: the device's insert rule (fast_limo_amd/csrc/hip/flimo_gbook.hip: route, sort, decide, compact, gather, build) at
its thresholds, on the fixtures of insert_rule_common.py, against the oracle's octree.  After every batch the map's size, its points
row for row in insertion order, and the index's self-check; after the last one the distances of a few hundred 5-NN queries placed
at the case's own edges, bit for bit.  Everything goes through the C ABI (_lib.HipCtx).

The one place where the reference has no answer is the zero-size root ("The zero-size root"): irc.OracleMap states this
project's rule from oracle octrees alone."""
import numpy as np
import pytest

import insert_rule_common as irc

pytestmark = pytest.mark.gpu

GROUPS = irc.groups()
X_IDENTITY = np.zeros(26)
X_IDENTITY[6] = 1.0
X_IDENTITY[10] = 1.0
X_IDENTITY[25] = -9.809


def _check_batch(ctx, om, what):
    assert ctx.map_size() == om.oc.size() == len(om.expect), what
    np.testing.assert_array_equal(ctx.map_points(), om.expect, err_msg=what)
    assert ctx.grid_selfcheck()[0] == 0, what


def _check_knn(ctx, om, case):
    if om.oc.size() == 0:
        return
    q = irc.queries_of(case)
    assert 100 <= len(q) <= 1000
    idx, sqd, cnt = ctx.knn(q, 5)
    _, osqd, ocnt, _ = om.oc.knn(q, 5)
    np.testing.assert_array_equal(cnt, ocnt, err_msg=case["name"])
    valid = np.arange(5)[None, :] < ocnt[:, None]
    np.testing.assert_array_equal(sqd[valid], osqd[valid], err_msg=case["name"])


def _run_case(_lib, oracle, case, downsample, add=None):
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(case["min_extent"], 2, downsample, irc.cell_size_of(case))
        om = irc.OracleMap(oracle, case["min_extent"], downsample)
        for k, b in enumerate(case["batches"]):
            (add or (lambda c, pts: c.map_add(pts)))(ctx, b)
            om.update(b)
            _check_batch(ctx, om, "%s downsample=%s batch %d" % (case["name"], downsample, k))
        if case["stored"] is not None:
            assert ctx.map_size() == case["stored"][downsample], (case["name"], "the count worked out by hand")
        _check_knn(ctx, om, case)
        return om
    finally:
        ctx.close()


@pytest.mark.parametrize("downsample", [True, False])
@pytest.mark.parametrize("group", list(GROUPS))
def test_device_insert_rule_at_its_edges(built, oracle, group, downsample):
    from fast_limo_amd import _lib
    for case in GROUPS[group]:
        _run_case(_lib, oracle, case, downsample)


def test_big_item_through_the_resident_scan(built, oracle):
    """The device-batch entry: every batch of a whole-block case goes in as the resident scan at the identity pose."""
    from fast_limo_amd import _lib
    case = next(c for c in GROUPS["big_items"] if c["name"] == "big_child_of_2049")

    def add(ctx, pts):
        ctx.scan_set(pts)
        ctx.map_add_scan(X_IDENTITY)

    _run_case(_lib, oracle, case, True, add)


@pytest.mark.parametrize("downsample", [True, False])
def test_a_crop_to_one_point_then_a_batch_elsewhere(built, oracle, downsample):
    """The zero-size root reached by removal: a crop that leaves one stored point leaves a root of half edge 0."""
    from fast_limo_amd import _lib
    s = 0.25
    rng = np.random.default_rng(71)
    first = np.concatenate([irc.corners(8 * s), irc.dense_over(rng, -8 * s, 8 * s, 300)])
    P = first[7].copy()
    P1 = first[7:8].copy()                                                # the same as a batch of one
    assert np.sum(np.all(first == P, axis=1)) == 1
    near = np.abs(first - P).max(1)
    eps = np.float32(0.5 * np.sort(near)[1])                              # half the way to the next stored point
    case = dict(name="crop_to_one_point", min_extent=s, focus=np.array([P, [3.0, 3.0, 3.0], [0.0] * 3], np.float32), stored=None,
                batches=[first, irc.cube_pts(rng, 2.0, 4.0, 50), irc.dense_over(rng, -4, 4, 3000)])
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(s, 2, downsample)
        ctx.map_add(first)
        assert ctx.map_crop_box(P - eps, P + eps) == len(first) - 1
        om = irc.OracleMap(oracle, s, downsample)
        om.update(P1)                                                # clear() + initialize(kept)
        _check_batch(ctx, om, "after the crop")
        ctx.map_add(P1)                                              # the same location again: appended as ever
        om.update(P1)
        _check_batch(ctx, om, "second copy")
        for k, b in enumerate(case["batches"][1:]):
            ctx.map_add(b)
            om.update(b)
            _check_batch(ctx, om, "batch %d after the crop" % k)
        assert om.reinits == 1
        _check_knn(ctx, om, case)
    finally:
        ctx.close()


def test_a_deep_tree_beside_an_ordinary_map(built, oracle):
    """Two contexts fed in turn, one with the deepest chain, one with an ordinary case: the per-context scratch stays apart."""
    from fast_limo_amd import _lib
    deep = next(c for c in GROUPS["deep_d24_s0.01"] if c["name"].startswith("deep_create_") and c["name"].endswith("oct7"))
    plain = next(c for c in GROUPS["root_growth"] if c["name"] == "root_both_sides_in_one_batch")
    a, b = _lib.HipCtx(0), _lib.HipCtx(0)
    try:
        oms = []
        for ctx, case in ((a, deep), (b, plain)):
            ctx.map_config(case["min_extent"], 2, True, irc.cell_size_of(case))
            oms.append(irc.OracleMap(oracle, case["min_extent"], True))
        for k in range(max(len(deep["batches"]), len(plain["batches"]))):
            for ctx, case, om in ((a, deep, oms[0]), (b, plain, oms[1])):
                if k < len(case["batches"]):
                    ctx.map_add(case["batches"][k])
                    om.update(case["batches"][k])
            for ctx, case, om in ((a, deep, oms[0]), (b, plain, oms[1])):
                _check_batch(ctx, om, "%s batch %d" % (case["name"], k))
        _check_knn(a, oms[0], deep)
        _check_knn(b, oms[1], plain)
    finally:
        a.close()
        b.close()


def test_a_tree_deeper_than_the_build_supports_is_refused_untouched(built, oracle):
    """GB_MAX_DEPTH = 48 (flimo_gbook.h): a batch whose root cube would be more halvings than that above 2 min_extent is refused by
    name before anything changes -- map, index and book answer as before, and the next ordinary batch is decided as if the refused
    one had never been sent."""
    from fast_limo_amd import _lib
    t = irc.too_deep_case()
    rng = np.random.default_rng(3)
    nxt = irc.dense_over(rng, -9, 9, 1500)
    q = rng.uniform(-10, 10, (300, 3)).astype(np.float32)
    ctx = _lib.HipCtx(0)
    try:
        ctx.map_config(t["min_extent"], 2, True)
        with pytest.raises(_lib.FlimoError, match="too deep"):
            ctx.map_add(t["first_too_deep"])                              # as a first batch
        assert ctx.map_size() == 0
        om = irc.OracleMap(oracle, t["min_extent"], True)
        ctx.map_add(t["ok"])
        om.update(t["ok"])
        _check_batch(ctx, om, "first batch")
        pts0, knn0, check0, bytes0 = ctx.map_points().copy(), ctx.knn(q, 5), ctx.grid_selfcheck(), ctx.map_index_bytes()
        with pytest.raises(_lib.FlimoError, match="too deep"):
            ctx.map_add(t["too_deep"])                                    # as a later batch: the root would have to grow
        assert ctx.map_size() == len(pts0)
        np.testing.assert_array_equal(ctx.map_points(), pts0)
        for x, y in zip(ctx.knn(q, 5), knn0):
            np.testing.assert_array_equal(x, y)
        assert ctx.grid_selfcheck() == check0 and check0[0] == 0
        assert ctx.map_index_bytes() == bytes0
        ctx.map_add(nxt)                                                  # outside the root by one metre: it still grows
        om.update(nxt)
        _check_batch(ctx, om, "the batch after the refusal")
    finally:
        ctx.close()
