"""Developer probe (GPU box): what flimo_radius_search costs and what it replaces (profiles/radius_search/README.md).

Per map (1M and 20M points as bench.py builds them), 65 536 queries near the surfaces, radius 0.3 / 1 / 3 m:
  calls     milliseconds per call of the C entry (host clock around the call, which ends in a stream wait; arrays sized
            beforehand, warm-up, then --reps repeats: median, min, max) for count-only / unsorted / sorted; results and candidates
            examined per query; bytes of results copied back
  replaces  same queries: (a) the reference's traversal restated in tests/radius_ref on ONE CPU thread, a 1 024-query sample
            (octree of the same points); (b) flimo_map_points alone -- the floor of "download the map and search on the host";
            (c) flimo_knn k = 5 for scale
  --trace   a short run (a few calls per case, nothing else) for `rocprofv3 --kernel-trace --stats -- python tools/gpu_radius_probe.py --trace`

usage: python tools/gpu_radius_probe.py [--maps 1M,20M] [--reps N] [--no-ref] [--trace] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from fast_limo_amd import _lib, synth

MAPS = {"1M": (1000000, 100.0), "20M": (20000000, 447.0)}      # bench.py: the headline's map, roofline.hbm_regime's map
RADII = (0.3, 1.0, 3.0)
NQ = 65536


def stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def call(ctx, q, radius, flags, off, idx, sqd, cap):
    total = C.c_uint64(0)
    t0 = time.perf_counter()
    rc = ctx._L.flimo_radius_search(ctx._h, q.ctypes.data, q.size // 3, float(radius), flags, off.ctypes.data, None if idx is None else idx.ctypes.data,
                                    None if sqd is None else sqd.ctypes.data, None, cap, C.byref(total))
    ms = 1e3 * (time.perf_counter() - t0)
    assert rc == 0, (rc, ctx._L.flimo_last_error(ctx._h))
    return ms, int(total.value)


def probe_map(name, reps, with_ref, trace):
    n, box = MAPS[name]
    mp = synth.box_world_map(n, box, 1)
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(mp)
    rs = np.random.RandomState(7)
    q = np.ascontiguousarray((mp[rs.choice(n, NQ)] + rs.normal(0, 0.3, (NQ, 3))).astype(np.float32)).reshape(-1)
    out = dict(map_points=ctx.map_size(), box=box, queries=NQ, radii={})
    off = np.zeros(NQ + 1, np.uint64)
    for radius in RADII:
        _, total = call(ctx, q, radius, 0, off, None, None, 0)
        idx, sqd = np.empty(total, np.int32), np.empty(total, np.float32)
        r = dict(results_per_query=total / NQ, result_bytes_copied_back=8 * total + 8 * (NQ + 1))
        if not trace:
            r["candidates_per_query"] = float(ctx.radius_candidates(q, radius).mean())
        for tag, flags, a, b, cap in (("count_only", 0, None, None, 0), ("unsorted", 0, idx, sqd, total), ("sorted", 1, idx, sqd, total)):
            for _ in range(2):
                call(ctx, q, radius, flags, off, a, b, cap)
            r[tag + "_ms"] = stats([call(ctx, q, radius, flags, off, a, b, cap)[0] for _ in range(3 if trace else reps)])
        out["radii"][str(radius)] = r
        print(name, radius, json.dumps(r), flush=True)
    if trace:
        ctx.close()
        return out
    # (b) the map through PCIe, (c) k-NN for scale
    t = []
    for _ in range(max(3, reps // 4)):
        t0 = time.perf_counter(); ctx.map_points(); t.append(1e3 * (time.perf_counter() - t0))
    out["map_points_download_ms"] = stats(t)
    qq = q.reshape(-1, 3)
    ctx.knn(qq, 5)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.knn(qq, 5); t.append(1e3 * (time.perf_counter() - t0))
    out["knn5_ms"] = stats(t)
    stored = ctx.map_points()
    ctx.close()
    # (a) the reference's traversal, one CPU thread, 1 024 of the queries; its octree holds the points the map stores
    if with_ref:
        from radius_common import RadiusRef
        ref = RadiusRef()
        t0 = time.perf_counter()
        ref.update(stored)
        out["ref_octree_build_s"] = time.perf_counter() - t0
        sample = qq[np.sort(np.random.RandomState(1024).choice(NQ, 1024, replace=False))]
        out["ref_cpu_one_thread"] = {}
        for radius in RADII:
            t0 = time.perf_counter()
            roff, _, _, sc = ref.radius_search(sample, radius)
            ms = 1e3 * (time.perf_counter() - t0)
            out["ref_cpu_one_thread"][str(radius)] = dict(ms_for_1024_queries=ms, ms_scaled_to_65536=ms * 64.0, results=int(roff[-1]), through_shortcut=sc)
    print(name, json.dumps({k: v for k, v in out.items() if k != "radii"}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="1M,20M")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {m: probe_map(m, a.reps, not a.no_ref, a.trace) for m in a.maps.split(",")}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
