"""GPU: the hand-offs at the two ends of a measurement pass, through the C ABI.

  tail   fit_reduce_publish (flimo_kernels.hip): partial sums -> group ticket -> gather -> 16-byte {sum, pass number} granules, and the
         launch's two counters, loaded by a lane of their own right behind the gather and published beside the sums;
  head   chain_enter: a pass queued ahead of its pose (pipelined host loop) gets "go" and its constants in one look -- PH_GRANULES
         eight-byte granules {word, epoch} (PipeHead, flimo_chain.h) -- and starts only when it has seen every one of them.

Neither changes a sum or an order of summation: everything here is compared byte for byte, except the pass's sums against the record
path's rows added on the host, which add in another order (bound below)."""
import threading

import numpy as np
import pytest

from common import CAPS, cfg1_scene
from fast_limo_amd import synth

pytestmark = pytest.mark.gpu


def _ident():
    x = np.zeros(26); x[6] = 1.0; x[10] = 1.0; x[25] = -9.809
    return x


def _tstar():
    x = _ident()
    x[0:3] = synth.T_STAR_T
    r, p_, y = [np.deg2rad(v) for v in synth.T_STAR_RPY_DEG]
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p_ / 2), np.sin(p_ / 2), np.cos(y / 2), np.sin(y / 2)
    x[3:7] = [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]
    return x


def _poses(x, n=4):
    """n poses around x that differ in position AND attitude (every matrix of the pass's constants changes from pass to pass)."""
    out = []
    for k in range(n):
        xk = x.copy()
        xk[0] += 0.004 * k; xk[1] -= 0.003 * k
        q = xk[3:7] + np.array([0.0, 0.0, 0.0008 * k, 0.0])
        xk[3:7] = q / np.linalg.norm(q)
        out.append(xk)
    return out


def _queues_ahead():
    """Whether a context of this device queues passes ahead of their poses is the HARDWARE's answer (large BAR), asked before any work:
    where it says yes, a context that published nothing is a failure (its head's allocation or its host-store probe broke), not a skip."""
    from fast_limo_amd import _lib
    if not _lib.device_large_bar(0):
        pytest.skip("this device does not map its memory for the host: the plain loop runs")


def _same(a, b, msg=""):
    assert a[2] == b[2], msg
    assert a[0].tobytes() == b[0].tobytes(), msg
    assert a[1].tobytes() == b[1].tobytes(), msg


def _against_the_rows(ctx, got, tag):
    """The pass's sums against the record path's rows (flimo_match_fetch_H) added on the host in float64, at relative 1e-12.  Both
    add the same exact products (float32 rows, float64 products) in different orders, so entry (i, j) of either sum is off by a
    multiple of 2^-53 * sum_k |H_ki H_kj| <= 2^-53 * sqrt(D_i D_j) with D = diag(H^T H) (Cauchy-Schwarz): that is the scale the
    1e-12 is relative to (an off-diagonal entry may cancel to nothing).  The multiple is ~sqrt(n) in practice (5e-14 at 200 000
    rows); a lost or doubled partial, which is what this check is for, shows at 1e-3 and above."""
    HTH, HTh, M = got
    H, h = ctx.match_fetch_H()
    assert H.shape[0] == M, tag
    if M == 0:
        return
    ref, refh = H.T @ H, H.T @ h
    d = np.sqrt(np.diag(ref))
    hn = np.sqrt(float(h @ h))
    err, errh = np.abs(HTH - ref) / np.outer(d, d), np.abs(HTh - refh) / (d * hn)
    print("%s: M %d, sums vs rows: H^T H %.2e, H^T h %.2e (relative to sqrt(D_i D_j))" % (tag, M, err.max(), errh.max()))
    assert err.max() <= 1e-12, (tag, err.max())
    assert errh.max() <= 1e-12, (tag, errh.max())


def test_the_same_pass_200_times_is_the_same_bytes(built):
    """One context, one scan, one pose (the converged one: few stragglers, so every pass after the scan's first keeps its layout): 200
    one-launch passes, then 200 with the fit as its own dispatch (fuse = 0) -- H^T H, H^T h and M identical bytes every time; the sums
    of either layout equal the record path's rows added on the host."""
    from fast_limo_amd import _lib
    mp, scan5, _ = cfg1_scene()
    cfg = _lib.default_match_cfg(**CAPS)
    x = _tstar()
    for fuse in (1, 0):
        h = _lib.HipCtx()
        h.set_update_mode(1)
        h.set_path_switches(fuse=fuse)
        h.map_add(np.ascontiguousarray(mp[:, :3]))
        h.scan_set(np.ascontiguousarray(scan5[:, :3]))
        for _ in range(5):                               # (the scan's first pass has no bound; pass positions 1 .. 3 settle their layout)
            h.match_reduce(x, cfg)
        assert max(h.stragglers_by_pass()) <= 1024, h.stragglers_by_pass()
        n0 = h.fused_pass_count()
        ref = h.match_reduce(x, cfg)
        for it in range(200):
            _same(ref, h.match_reduce(x, cfg), "pass %d, fuse=%d" % (it, fuse))
        assert h.fused_pass_count() - n0 == (201 if fuse == 1 else 0)
        _against_the_rows(h, ref, "cfg1 fuse=%d" % fuse)
        h.close()


def _crowded_context():
    """A map crowded under the sensor as in test_crowded_cells_second_level_is_exact (raw sweeps inserted at the pose; second level
    off: the one-launch pass carries the crowded cells itself, which is where its workgroups' loads are most uneven)."""
    import os
    from fast_limo_amd import _lib
    L = 40.0
    mp = synth.box_world_map(150000, L, 5)
    x = _tstar()
    os.environ["FLIMO_FINE"] = "0"
    try:
        ctx = _lib.HipCtx(0)
    finally:
        os.environ.pop("FLIMO_FINE")
    ctx.set_update_mode(1)
    ctx.map_config()
    ctx.map_add(mp)
    for j in range(6):
        ctx.scan_set(np.ascontiguousarray(synth.velodyne_scan(64, 1024, L, 40 + j)[:, :3]))
        ctx.map_add_scan(x, 0.1 * (j + 1))
    return ctx, np.ascontiguousarray(synth.velodyne_scan(64, 512, L, 77)[:, :3]), x


def test_uneven_load_three_contexts_at_once(built):
    """Uneven load is where hand-offs break.  Three contexts over a crowded map register at the same time from three threads, 100
    registrations each (scan set, then four pipelined passes at four poses); every pass of every registration equals, byte for byte,
    the same context's registration running alone."""
    from fast_limo_amd import _lib
    _queues_ahead()
    cfg = _lib.default_match_cfg(**CAPS)
    ctxs = [_crowded_context() for _ in range(3)]
    xs = _poses(ctxs[0][2])

    def registration(ctx, query):
        ctx.scan_set(query)
        ctx.set_pass_pipeline(True)
        out = []
        for k, xk in enumerate(xs):
            if k == len(xs) - 1:
                ctx.pass_pipeline_last()
            out.append(ctx.match_reduce(xk, cfg))
        ctx.pass_pipeline_end()
        return out

    # (which layout a pass runs in follows the straggler counts of the passes before it: the first registrations of a context settle that)
    for c, q, _ in ctxs:
        for _ in range(3):
            registration(c, q)
    alone = [registration(c, q) for c, q, _ in ctxs]
    for a in alone[1:]:
        for ra, rb in zip(alone[0], a):
            _same(ra, rb, "three contexts over the same map")
    assert alone[0][0][2] > 1000
    errors = []

    def worker(i):
        try:
            c, q, _ = ctxs[i]
            for r in range(100):
                for k, (ra, rb) in enumerate(zip(alone[i], registration(c, q))):
                    _same(ra, rb, "context %d registration %d pass %d" % (i, r, k))
        except BaseException as e:          # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    stats = [c.pass_pipeline_stats() for c, _, _ in ctxs]
    for c, _, _ in ctxs:
        c.close()
    if errors:
        raise errors[0]
    print("pipeline counters of the three contexts:", stats)
    for st in stats:
        # 104 registrations of three queued passes each; a host thread that came back late may have aged a few, none may have left
        assert st["published"] >= 104 * 3 // 2 and st["left"] == 0, st


def test_a_queued_pass_starts_on_a_complete_head_only(built, monkeypatch):
    """A pass queued ahead of its pose: (1) published a few milliseconds late (FLIMO_TEST_PUBLISH_DELAY_MS), (2) published in two
    halves a few milliseconds apart (FLIMO_TEST_PUBLISH_SPLIT_MS: the launch sees half of its granules carry its epoch for that long
    and must not start -- the other half still holds the previous pass's constants, and every pass here has a pose of its own;
    the second half's only words that change with the pose are R_inv's, granules 36 .. 44: _poses must keep changing the attitude),
    (3) cancelled (the scan is set again while the launch waits).  All well below the 50 ms after which a waiting launch leaves.
    The sums are the unqueued loop's byte for byte, and the pipeline's counters say what happened."""
    from fast_limo_amd import _lib
    _queues_ahead()
    mp, scan5, _ = cfg1_scene()
    scan = np.ascontiguousarray(scan5[:, :3])
    cfg = _lib.default_match_cfg(**CAPS)
    xs = _poses(_ident())

    def run(pipeline, env=None, cancel_after=None):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, str(v))
        h = _lib.HipCtx()
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)
        h.set_update_mode(1)
        h.map_add(np.ascontiguousarray(mp[:, :3]))
        h.scan_set(scan)
        h.set_pass_pipeline(pipeline)
        out = []
        for k, xk in enumerate(xs):
            out.append(h.match_reduce(xk, cfg))
            if cancel_after == k:
                h.scan_set(scan)                  # (nothing may line up behind a pass that waits: it is told to leave)
        h.pass_pipeline_end()
        st = h.pass_pipeline_stats()
        h.close()
        return out, st

    plain, st0 = run(False)
    assert st0["published"] == 0
    piped, st1 = run(True)
    assert st1["published"] == len(xs) - 1 and st1["aged"] == 0 and st1["left"] == 0, st1      # (nothing delays this run)
    late, st2 = run(True, {"FLIMO_TEST_PUBLISH_DELAY_MS": 4})
    halves, st3 = run(True, {"FLIMO_TEST_PUBLISH_SPLIT_MS": 4})
    print("pipeline counters: plain", st1, "late", st2, "in two halves", st3)
    for tag, got, st in (("pipelined", piped, st1), ("published late", late, st2), ("published in two halves", halves, st3)):
        for k, (ra, rb) in enumerate(zip(plain, got)):
            _same(ra, rb, "%s, pass %d" % (tag, k))
        # three passes were queued ahead; each was published to (or, on a host that came back after the 12.5 ms age bound, told to
        # leave and launched the usual way); none of the launches left on its own
        assert st["published"] + st["aged"] == len(xs) - 1 and st["published"] >= 1 and st["left"] == 0, (tag, st)
    # (3) the scan set again after the second pass: the launch queued behind it leaves, the next pass is a first pass
    ref_out, _ = run(False, cancel_after=1)
    got_out, st4 = run(True, cancel_after=1)
    assert st4["cancelled"] >= 1 and st4["left"] == 0, st4
    for k, (ra, rb) in enumerate(zip(ref_out, got_out)):
        _same(ra, rb, "cancelled after pass 1, pass %d" % k)


@pytest.mark.parametrize("case", ["spread_1900", "dense_256k"])
def test_other_grid_sizes(built, case):
    """A small scan (1 900 points: the one-launch pass spreads its queries over more workgroups) and a 256k-point scan (256 workgroups
    per group: more than one batch of the gather per slice), one launch and three dispatches.  Repeated passes are the same bytes,
    pipelined passes equal the unqueued loop's, and the sums equal the record path's rows."""
    from fast_limo_amd import _lib
    if case == "spread_1900":
        L = 25.0
        mp = synth.box_world_map(50000, L, 1)
        scan = np.ascontiguousarray(synth.box_world_scan_random(1900, L, 2)[:, :3])
    else:
        L = 150.0
        mp = synth.box_world_map(3000000, L, 1)
        scan = np.ascontiguousarray(synth.velodyne_scan(128, 2048, L, 2)[:, :3])
    cfg = _lib.default_match_cfg(**CAPS)
    xs = _poses(_tstar())
    res = {}
    for label, fuse, pipeline in (("fused", 1, False), ("piped", 1, True), ("split", 0, False)):
        h = _lib.HipCtx()
        h.set_update_mode(1)
        h.set_path_switches(fuse=fuse)
        h.map_add(np.ascontiguousarray(mp[:, :3]))
        h.scan_set(scan)
        h.set_pass_pipeline(pipeline)
        out = [h.match_reduce(xk, cfg) for xk in xs]
        h.pass_pipeline_end()
        st = h.pass_pipeline_stats()
        print("%s %s: pipeline counters" % (case, label), st)
        if pipeline and _lib.device_large_bar(0):
            assert st["published"] >= 1 and st["left"] == 0, (case, st)
        else:
            assert st["published"] == 0, (case, st)
        h.set_pass_pipeline(False)
        again = h.match_reduce(xs[-1], cfg)
        for it in range(20):
            _same(again, h.match_reduce(xs[-1], cfg), "%s %s repeat %d" % (case, label, it))
        assert out[-1][2] == again[2]
        assert (h.fused_pass_count() > 0) == (fuse == 1)
        if not pipeline:
            _against_the_rows(h, again, "%s %s" % (case, label))
        res[label] = out
        h.close()
    assert res["fused"][-1][2] > (200 if case == "spread_1900" else 10000)
    for k, (ra, rb) in enumerate(zip(res["fused"], res["piped"])):
        _same(ra, rb, "%s: unqueued against pipelined, pass %d" % (case, k))
    for ra, rb in zip(res["fused"], res["split"]):
        assert ra[2] == rb[2]                                  # (another partition of the scan: the same matches, another order)
