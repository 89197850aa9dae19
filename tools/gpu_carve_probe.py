"""Developer probe (GPU box): what seeing through the map costs ("Map carving"; profiles/carve/README.md).

Per case -- a 64k-point sweep (64 rings x 1024 azimuths) at res 256 / win 1 against a box world of 1M and of 20M stored points,
a tenth of them a cloud of "ghost" points in the free space the sweep looks through --:

  seen_through   flimo_map_seen_through with and without the mask download
  carve          a removing flimo_map_carve (the map is put back before every repetition, outside the timed window)
  carve_nothing  flimo_map_carve that removes nothing (a margin beyond the scene): the two launches, no relayout
  crop           flimo_map_crop_box removing about as many points, for the relayout both share
  manual         the route the call replaces: flimo_map_points -> the numpy yardstick (tests/carve_common.py) -> flimo_map_clear ->
                 flimo_map_add(kept)

Every call ends synchronised, so the host clock around it is the call's time; beside it the time between two device events
recorded around the call on the null stream (torch.cuda.Event).  Medians over --reps (default 10; the 20M case runs a fifth of them,
the manual route at most 3).  (--kernels-only: just the GPU calls, for a rocprofv3 --kernel-trace --stats run of its own.)

usage: python tools/gpu_carve_probe.py [1M] [20M] [--reps N] [--kernels-only] [--json FILE]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from fast_limo_amd import _lib, synth
import carve_common as cc

CFG = dict(res=256, win=1, margin=0.2, rel_margin=0.02)
CASES = {"1M": dict(n=1000000, box=100.0), "20M": dict(n=20000000, box=447.0)}


def med(v):
    return float(np.median(v)) if len(v) else None


def timed(fn):
    """(result, wall ms, device-event ms) of a call that ends synchronised."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    r = fn()
    wall = 1e3 * (time.perf_counter() - t0)
    e1.record()
    e1.synchronize()
    return r, wall, float(e0.elapsed_time(e1))


def scene(n, box):
    static = synth.box_world_map(n - n // 10, box, 1)
    rs = np.random.RandomState(5)
    m = n // 10
    ghost = np.stack([rs.uniform(0.05 * box, 0.6 * box, m), rs.uniform(-0.3 * box, 0.3 * box, m), rs.uniform(-1.5, 6.0, m)], 1).astype(np.float32)
    scan = np.ascontiguousarray(synth.velodyne_scan(64, 1024, box, 2)[:, :3])
    x = np.zeros(26); x[6] = 1; x[10] = 1
    x[0:3] = synth.T_STAR_T
    return np.concatenate([static, ghost]), scan, x, np.float32(synth.T_STAR_T)


def run(name, reps, kernels_only):
    c = CASES[name]
    mp, scan, x, sensor = scene(c["n"], c["box"])
    reps = reps if c["n"] <= 2000000 else max(2, reps // 5)
    ctx = _lib.HipCtx(0)
    ctx.map_config(0.2, 2, False)                                       # (every point stored: the sizes are the cases' names)
    ctx.scan_set(scan)
    out = dict(scan_points=int(len(scan)), cfg=CFG)
    t = {k: [] for k in ("seen_wall", "seen_dev", "seen_count_wall", "carve_wall", "carve_dev", "nothing_wall", "nothing_dev", "crop_wall",
                         "crop_dev", "manual_wall")}
    removed = kept_crop = 0
    for r in range(reps + 1):                                           # (repetition 0 warms every launch up and is dropped)
        ctx.map_clear(); ctx.map_add(mp)
        n0 = ctx.map_size()
        (mask, cnt), w, d = timed(lambda: ctx.map_seen_through(x, sensor, **CFG))
        (_, cnt2), w2, _ = timed(lambda: ctx.map_seen_through(x, sensor, want_mask=False, **CFG))
        _, wn, dn = timed(lambda: ctx.map_carve(x, sensor, **dict(CFG, margin=1e4)))
        removed, wc, dc = timed(lambda: ctx.map_carve(x, sensor, **CFG))
        assert cnt == cnt2 == removed and ctx.map_size() == n0 - removed
        ctx.map_clear(); ctx.map_add(mp)
        # a crop that removes about as many: everything above the matching quantile of x
        hi = np.float32([np.quantile(mp[:, 0], 1.0 - removed / float(n0)), 1e30, 1e30])
        kept_crop, wk, dk = timed(lambda: ctx.map_crop_box(np.float32([-1e30] * 3), hi))
        if r:
            for k, v in (("seen_wall", w), ("seen_dev", d), ("seen_count_wall", w2), ("carve_wall", wc), ("carve_dev", dc), ("nothing_wall", wn),
                         ("nothing_dev", dn), ("crop_wall", wk), ("crop_dev", dk)):
                t[k].append(v)
    for r in range(0 if kernels_only else min(reps, 3)):
        ctx.map_clear(); ctx.map_add(mp)
        t0 = time.perf_counter()
        pts = ctx.map_points()
        m = cc.yardstick(ctx.scan_to_world(x), pts, sensor, **CFG)
        kept = np.ascontiguousarray(pts[~m])
        ctx.map_clear()
        ctx.map_add(kept)
        t["manual_wall"].append(1e3 * (time.perf_counter() - t0))
        assert ctx.map_size() == n0 - removed, (ctx.map_size(), n0, removed)
    ctx.close()
    out.update(map_points=int(n0), seen_through=int(removed), crop_removed=int(kept_crop), reps=reps)
    out.update({k + "_ms_median": med(v) for k, v in t.items()})
    print(name, json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        sys.exit("gpu_carve_probe: no GPU -- nothing is measured without one")
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
    res = {name: run(name, reps, "--kernels-only" in args) for name in ([a for a in args if a in CASES] or list(CASES))}
    if "--json" in args:
        with open(args[args.index("--json") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
