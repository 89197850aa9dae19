"""Developer probe (GPU box): what flimo_map_correct costs and what it replaces (profiles/map_correct/README.md).

Per step -- a map of N stored points in S segments (N = 1M and 20M, S = 1, 100 and 10 000; the box world of bench.py, every segment a
batch of its own, down-sampling off so that the sizes are exact), medians of --reps repeats, wall clock (every call ends after a
stream wait):
  move        flimo_map_corrected without the points coming back: the table's upload and the move's launch alone
  correct     flimo_map_correct: the move, then clear() + initialize(moved points)           (rebuild = correct - move)
  crop        flimo_map_crop_box that removes ONE point of the same map: what a removal's rebuild costs at that size
  by_hand     what a caller without the entry does on the same device: flimo_map_points -> numpy, the same move per segment ->
              flimo_map_clear -> flimo_map_add of the moved points in one batch (and the table is then the caller's to keep)
Every step runs as a child process of this script under its own time limit; after a child that fails or runs out of time nothing
more is started.

usage: python tools/gpu_map_correct_probe.py [--reps N] [--sizes 1000000,20000000] [--segs 1,100,10000] [--limit SECONDS] [--json FILE]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    import numpy as np
    return float(np.median(v)) if len(v) else None


def child(n, n_seg, reps):
    import math
    import numpy as np
    from fast_limo_amd import _lib, synth

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return 1e3 * (time.perf_counter() - t0), out

    def rigid(k):
        R = synth.rpy_to_R(math.radians(0.01 * (k % 7)), math.radians(-0.02), math.radians(0.05 * (k % 11 + 1)))
        return np.concatenate([R, np.array([[0.01 * (k % 5)], [-0.02], [0.005]])], axis=1).reshape(12)

    def move(begin, T, pts):      # the contract's move in numpy (tests/segments_common.py)
        out = np.empty_like(pts)
        for s in range(len(T)):      # one slice per segment: no [N, 12] gather of matrices
            a, b, M = int(begin[s]), int(begin[s + 1]), T[s]
            X, Y, Z = (pts[a:b, c].astype(np.float64) for c in range(3))
            for k in range(3):
                out[a:b, k] = M[4 * k] * X + (M[4 * k + 1] * Y + (M[4 * k + 2] * Z + M[4 * k + 3]))
        return out

    mp = synth.box_world_map(n, 447.0 if n > 2000000 else 100.0, 1)
    T = np.array([rigid(k) for k in range(n_seg)])
    edges = [(n * k) // n_seg for k in range(n_seg + 1)]
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, False)
    t_build, _ = timed(lambda: [(ctx.map_segment_mark() if k else None, ctx.map_add(mp[edges[k]:edges[k + 1]], stamp=float(k))) for k in range(n_seg)])
    begin, stale = ctx.map_segments()
    assert ctx.map_size() == n and len(begin) == n_seg + 1 and not stale, (ctx.map_size(), len(begin), stale)
    t_move, t_correct, t_crop, t_hand, changed = [], [], [], [], 0
    for _ in range(reps):
        t_move.append(timed(lambda: ctx.map_corrected(T, want_xyz=False))[0])
        ms, changed = timed(lambda: ctx.map_correct(T))
        t_correct.append(ms)
    assert ctx.map_size() == n and ctx.map_segments()[0].tolist() == begin.tolist()
    for _ in range(reps):
        ms, pts = timed(ctx.map_points)
        ms2, moved = timed(lambda: np.ascontiguousarray(move(begin, T, pts)))
        ms3, _ = timed(lambda: (ctx.map_clear(), ctx.map_add(moved, stamp=1.0)))
        t_hand.append((ms + ms2 + ms3, ms, ms2, ms3))
        assert ctx.map_size() == n
    for _ in range(reps):      # each repeat removes the point of largest x
        pts = ctx.map_points()
        hi = pts.max(0)
        hi[0] = np.partition(pts[:, 0], -2)[-2]
        ms, removed = timed(lambda: ctx.map_crop_box(pts.min(0), hi))
        if removed >= 1:
            t_crop.append(ms)
    ctx.close()
    hand = np.array(t_hand)
    out = dict(map_points=n, segments=n_seg, reps=reps, build_ms=t_build, changed=int(changed), move_ms=med(t_move), correct_ms=med(t_correct),
               rebuild_ms=med(t_correct) - med(t_move), crop_one_point_ms=med(t_crop), by_hand_ms=med(hand[:, 0]),
               by_hand_points_ms=med(hand[:, 1]), by_hand_numpy_ms=med(hand[:, 2]), by_hand_clear_add_ms=med(hand[:, 3]))
    print("RESULT " + json.dumps(out), flush=True)


def main(args):
    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    if "--child" in args:
        at = args.index("--child")
        return child(int(args[at + 1]), int(args[at + 2]), int(opt("--reps", 3)))
    sizes = [int(v) for v in opt("--sizes", "1000000,20000000").split(",")]
    segs = [int(v) for v in opt("--segs", "1,100,10000").split(",")]
    limit = float(opt("--limit", 240))
    res = []
    for n in sizes:
        for s in segs:
            reps = opt("--reps", 5 if n <= 2000000 else 3)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(s), "--reps", str(reps)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print("step %d x %d ran out of its %g s: stopping" % (n, s, limit), flush=True)
                res.append(dict(map_points=n, segments=s, error="time limit"))
                break
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print("step %d x %d failed (%d): stopping\n%s" % (n, s, p.returncode, p.stderr[-2000:]), flush=True)
                res.append(dict(map_points=n, segments=s, error="exit %d" % p.returncode))
                break
            res.append(json.loads(line[0][7:]))
            print(res[-1], flush=True)
        else:
            continue
        break
    if "--json" in args:
        with open(opt("--json", None), "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if all("error" not in r for r in res) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]) or 0)
