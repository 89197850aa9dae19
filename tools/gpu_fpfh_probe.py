"""Developer probe (GPU box): what flimo_map_fpfh costs and what it replaces (profiles/fpfh/README.md).

A 1M-point map as bench.py builds it, the descriptors of all its points at k = 10 and k = 32, normals from 10 neighbours, no gates.
In the same process:
  fused_k*      flimo_map_fpfh, 136 B per point come back (fpfh and cnt)
  range_k*      ... of the last 65 536 stored points only: the two stages over the whole map are still paid
  composed_k*   the route that exists without the call: flimo_map_normals_range (16 B per point back), flimo_knn_k with the points
                uploaded as queries (8 B x k per point back), the pair features, the histograms and the sums in numpy
                (tests/fpfh_common.py, the definition's restatement, on one core)
Milliseconds per call: host clock around the calls, each of which ends in a stream wait; the fused calls warm-up, then --reps repeats
taking turns: median, min, max; the composed route once per k (its parts timed apart).  The two routes are compared: cnt and spfh
equal, the bits of fpfh equal, on the points the restatement does not mark as tainted (atan2 on a bin's edge).
  --trace   a short run (a few fused calls per k, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_fpfh_probe.py --trace`

usage: python tools/gpu_fpfh_probe.py [--reps N] [--points N] [--trace] [--json FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from fast_limo_amd import _lib, synth
from gpu_scan_fitness_probe import taking_turns
import fpfh_common as fc

BOX, NORMAL_K, RANGE = 100.0, 10, 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(a.points, BOX, 1))
    pts = ctx.map_points()
    n = len(pts)
    fused = lambda k, first=0: ctx.map_fpfh(first, None, want=("cnt",), k=k, normal_k=NORMAL_K)

    if a.trace:
        for k in (10, 32):
            for _ in range(3):
                fused(k)
        ctx.close()
        return
    cases = {"fused_k10": lambda: fused(10), "fused_k32": lambda: fused(32), "range_k10": lambda: fused(10, n - RANGE),
             "range_k32": lambda: fused(32, n - RANGE)}
    res = dict(map_points=n, box=BOX, normal_k=NORMAL_K, range_points=RANGE, ms=taking_turns(cases, a.reps, 1), composed_ms={}, agreement={})
    for k in (10, 32):
        t0 = time.perf_counter()
        nrm = ctx.normals_range(0, n, NORMAL_K, want=())["normal"]
        t1 = time.perf_counter()
        idx, sqd, cnt = ctx.knn_k(pts, k)
        t2 = time.perf_counter()
        r = fc.restate(pts, nrm, idx, sqd, cnt)
        t3 = time.perf_counter()
        res["composed_ms"][f"k{k}"] = dict(normals=1e3 * (t1 - t0), knn_k=1e3 * (t2 - t1), numpy=1e3 * (t3 - t2), total=1e3 * (t3 - t0))
        out = ctx.map_fpfh(k=k, normal_k=NORMAL_K)
        clean = ~r["tainted"]
        res["agreement"][f"k{k}"] = dict(
            tainted=int(r["tainted"].sum()), cnt_equal=bool(np.array_equal(out["cnt"], r["cnt"])),
            spfh_rows_that_differ_untainted=int(((out["spfh"] != r["spfh"]).any(1) & clean).sum()),
            fpfh_rows_that_differ_untainted=int(((fc.bits(out["fpfh"]) != fc.bits(r["fpfh"])).any(1) & clean).sum()))
        res[f"speedup_k{k}"] = res["composed_ms"][f"k{k}"]["total"] / res["ms"][f"fused_k{k}"]["median"]
        res[f"points_per_second_fused_k{k}"] = n / (1e-3 * res["ms"][f"fused_k{k}"]["median"])
    print(json.dumps(res), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
