"""Developer probe (GPU box): what flimo_map_outliers / flimo_map_remove_outliers cost and what they replace
(profiles/outliers/README.md).  A 1M-point box world plus 2 % specks in the air; for k = 8, 16, 32, ungated, std_mul 1 (wall clock, each
call ends after a stream wait; medians and the spread of each series):

  predicate   flimo_map_outliers over the whole map, stats only (no per-point output comes back)
  normals     in the same process and interleaved with it: flimo_map_normals_range(0, n, k + 1, INFINITY) without optional outputs --
              the same search with the heavier ending
  removal     flimo_map_remove_outliers on a freshly built map, beside flimo_map_crop_box on the same map with a box that removes
              about as many points (the same ordered compaction and relayout, no search)
  composed    the route without the calls: flimo_map_points, flimo_knn_k over them in chunks, numpy for the rest

usage: python tools/gpu_outliers_probe.py [--reps N] [--points N] [--json FILE]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fast_limo_amd import _lib, synth

INF = float("inf")


def series(v):
    v = np.asarray(v, float)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), reps=int(len(v))) if len(v) else None


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def composed(ctx, k, std_mul, chunk=1 << 19):
    """numpy on top of flimo_knn_k: PCL's StatisticalOutlierRemoval as a caller would write it today."""
    pts = ctx.map_points()
    mean = np.empty(len(pts))
    for a in range(0, len(pts), chunk):
        idx, sqd, cnt = ctx.knn_k(pts[a:a + chunk], k + 1)
        own = idx == (a + np.arange(idx.shape[0]))[:, None]
        d = np.where(own, 0.0, np.sqrt(sqd).astype(np.float64))
        mean[a:a + chunk] = d.sum(1) / np.maximum(cnt - 1, 1)
    return mean > mean.mean() + std_mul * mean.std(ddof=1)


def main(reps, n_pts):
    rs = np.random.RandomState(5)
    n_specks = n_pts // 50
    specks = np.stack([rs.uniform(-90, 90, n_specks), rs.uniform(-90, 90, n_specks), rs.uniform(0, 18, n_specks)], 1).astype(np.float32)
    mp = np.concatenate([synth.box_world_map(n_pts, 100.0, 1), specks])
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    out = {}
    try:
        ctx.map_add(mp)
        n = ctx.map_size()
        x = ctx.map_points()[:, 0].copy()
        for k in (8, 16, 32):
            cfg = dict(k=k, max_dist=INF, min_pts=0, std_mul=1.0)
            ctx.map_outliers(want=(), **cfg); ctx.normals_range(0, n, k + 1, INF, want=())      # warm-up
            t_pred, t_norm = [], []
            for r in range(reps):
                t_norm.append(timed(lambda: ctx.normals_range(0, n, k + 1, INF, want=()))[0])
                ms, res = timed(lambda: ctx.map_outliers(want=(), **cfg))
                t_pred.append(ms)
            stats = res["stats"]
            t_comp = [timed(lambda: composed(ctx, k, 1.0))[0] for _ in range(2)]
            mask = composed(ctx, k, 1.0)
            # the removal and a crop of as many points, each on a freshly built map
            hi = np.float32([np.quantile(x, 1.0 - stats["outliers"] / n), 1e4, 1e4])
            lo = np.float32([-1e4, -1e4, -1e4])
            t_rem, t_crop, removed, cropped = [], [], 0, 0
            for r in range(max(3, reps // 2)):
                ctx.map_clear(); ctx.map_add(mp)
                ms, (removed, _) = timed(lambda: ctx.map_remove_outliers(**cfg))
                t_rem.append(ms)
                ctx.map_clear(); ctx.map_add(mp)
                ms, cropped = timed(lambda: ctx.map_crop_box(lo, hi))
                t_crop.append(ms)
            ctx.map_clear(); ctx.map_add(mp)
            out["k%d" % k] = dict(map_points=int(n), outliers=stats["outliers"], composed_outliers=int(mask.sum()), mu=stats["mu"], sigma=stats["sigma"],
                                  predicate=series(t_pred), normals=series(t_norm), composed=series(t_comp), removal=series(t_rem),
                                  removed=int(removed), crop=series(t_crop), cropped=int(cropped))
            print("k%d" % k, json.dumps(out["k%d" % k]), flush=True)
    finally:
        ctx.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
    n_pts = int(args[args.index("--points") + 1]) if "--points" in args else 1000000
    res = main(reps, n_pts)
    if "--json" in args:
        with open(args[args.index("--json") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
