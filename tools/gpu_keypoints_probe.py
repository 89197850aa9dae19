"""Developer probe (GPU box): what flimo_map_keypoints costs and what it replaces (profiles/keypoints/README.md).

A 1M-point map as bench.py builds it, the ISS keypoints of all its points at k = nms_k = 32, PCL's thresholds, no gates.  In the same
process:
  fused       flimo_map_keypoints, 13 B per point come back (mask, saliency, cnt)
  mask_only   ... the mask and the count alone: 1 B per point
  range       ... of the last 65 536 stored points only: the saliency of the whole map is still paid
  composed    the route that exists without the call: flimo_map_normals_range with eig (68 B per point back), flimo_knn_k with the
              points uploaded as queries (8 B x nms_k per point back), the definition's restatement in numpy
              (tests/keypoints_common.py, on one core)
Milliseconds per call: host clock around the calls, each of which ends in a stream wait; the fused calls warm-up, then --reps repeats
taking turns: median, min, max; the composed route once (its parts timed apart).  The two routes are compared: saliency bits, cnt,
mask and count equal.
  --trace   a short run (a few fused calls, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_keypoints_probe.py --trace`

usage: python tools/gpu_keypoints_probe.py [--reps N] [--points N] [--trace] [--json FILE]"""
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
import keypoints_common as kc

BOX, K, RANGE = 100.0, 32, 65536
CFG = dict(k=K, nms_k=K)


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
    fused = lambda first=0, want=("saliency", "cnt"): ctx.map_keypoints(first, None, want=want, **CFG)

    if a.trace:
        for _ in range(3):
            fused()
        ctx.close()
        return
    cases = {"fused": fused, "mask_only": lambda: fused(0, ()), "range": lambda: fused(n - RANGE)}
    res = dict(map_points=n, box=BOX, cfg=kc.full(CFG), range_points=RANGE, ms=taking_turns(cases, a.reps, 1))
    c = kc.full(CFG)
    t0 = time.perf_counter()
    nr = ctx.normals_range(0, n, c["k"], c["max_dist"], c["min_pts"], None, want=("eig",))
    t1 = time.perf_counter()
    idx, _, ncnt = ctx.knn_k(pts, c["nms_k"], c["nms_max_dist"])
    t2 = time.perf_counter()
    r = kc.restate(nr["eig"], nr["cnt"], idx, ncnt, CFG)
    t3 = time.perf_counter()
    res["composed_ms"] = dict(normals=1e3 * (t1 - t0), knn_k=1e3 * (t2 - t1), numpy=1e3 * (t3 - t2), total=1e3 * (t3 - t0))
    out = fused()
    nan = np.isnan(r["saliency"])
    res["agreement"] = dict(salient=int((~nan).sum()), keypoints=out["count"], count_equal=bool(out["count"] == r["count"]),
                            mask_equal=bool(np.array_equal(out["mask"], r["mask"])), cnt_equal=bool(np.array_equal(out["cnt"], r["cnt"])),
                            saliency_bits_equal=bool(np.array_equal(np.isnan(out["saliency"]), nan)
                                                     and out["saliency"][~nan].tobytes() == r["saliency"][~nan].tobytes()))
    res["composed_over_fused"] = res["composed_ms"]["total"] / res["ms"]["fused"]["median"]
    res["points_per_second_fused"] = n / (1e-3 * res["ms"]["fused"]["median"])
    print(json.dumps(res), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
