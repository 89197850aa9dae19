"""Developer probe (GPU box): what flimo_knn_k costs and what it replaces (profiles/knn_k/README.md).

Per map (1M and 20M points as bench.py builds them), 65 536 queries near the surfaces, k = 8 / 16 / 32 / 64, gate off and 1 m:
  calls     milliseconds per call of the C entry (host clock around the call, which ends in a stream wait; arrays sized beforehand,
            warm-up, then --reps repeats: median, min, max); stored points examined per query (flimo_knn_k_candidates)
  routes    same queries, same box, same run:
            (a) the oracle octree's knn at the same k on ONE CPU thread and at the best thread count up to 16 (1M map only:
                an octree of the stored points), a 4 096-query sample scaled to 65 536;
            (b) flimo_knn (k = 5), the parent's call;
            (c) the only route the parent offers for k > 5: sorted flimo_radius_search (count call + fill call) at the smallest
                radius that gives every query its k -- the largest k-th distance of the batch, taken from flimo_knn_k's own
                result, a hair widened -- then truncated
  --trace   a short run (a few calls per case, nothing else) for `rocprofv3 --kernel-trace --stats -- python tools/gpu_knn_k_probe.py --trace`

usage: python tools/gpu_knn_k_probe.py [--maps 1M,20M] [--reps N] [--no-ref] [--trace] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
from fast_limo_amd import _lib, synth

MAPS = {"1M": (1000000, 100.0), "20M": (20000000, 447.0)}      # bench.py: the headline's map, roofline.hbm_regime's map
KS = (8, 16, 32, 64)
GATES = (float("inf"), 1.0)
NQ = 65536


def stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
    return stats(t)


def probe_map(name, reps, with_ref, trace):
    n, box = MAPS[name]
    mp = synth.box_world_map(n, box, 1)
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(mp)
    rs = np.random.RandomState(7)
    q = np.ascontiguousarray((mp[rs.choice(n, NQ)] + rs.normal(0, 0.3, (NQ, 3))).astype(np.float32))
    out = dict(map_points=ctx.map_size(), box=box, queries=NQ, k={})
    if trace:
        reps = 3
    i5, s5, c5 = np.empty((NQ, 5), np.int32), np.empty((NQ, 5), np.float32), np.empty(NQ, np.int32)
    out["knn5_ms"] = timed(lambda: ctx._L.flimo_knn(ctx._h, q.reshape(-1), NQ, 5, i5.reshape(-1), s5.reshape(-1), c5), reps)
    print(name, "flimo_knn k = 5:", json.dumps(out["knn5_ms"]), flush=True)
    for k in KS:
        idx, sqd, cnt = np.empty((NQ, k), np.int32), np.empty((NQ, k), np.float32), np.empty(NQ, np.int32)
        r = {}
        for gate in GATES:
            def call():
                rc = ctx._L.flimo_knn_k(ctx._h, q.ctypes.data, NQ, k, gate, idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data)
                assert rc == 0, (rc, ctx._L.flimo_last_error(ctx._h))
            g = dict(ms=timed(call, reps), results_per_query=float(cnt.mean()))
            g["ratio_to_knn5"] = g["ms"]["median"] / out["knn5_ms"]["median"]
            if not trace:
                g["candidates_per_query"] = float(ctx.knn_k_candidates(q, k, gate).mean())
            r["gate_off" if np.isinf(gate) else "gate_%gm" % gate] = g
        # (c) the parent's only route: a sorted radius search wide enough for every query's k-th neighbour, truncated
        ctx._L.flimo_knn_k(ctx._h, q.ctypes.data, NQ, k, float("inf"), idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data)
        radius = float(np.nextafter(np.sqrt(np.float64(sqd[:, k - 1].max())).astype(np.float32) * np.float32(1.0 + 1e-6), np.float32(np.inf)))
        if not trace or k == 16:
            off = np.zeros(NQ + 1, np.uint64)
            total = C.c_uint64(0)
            rc = ctx._L.flimo_radius_search(ctx._h, q.ctypes.data, NQ, radius, 0, off.ctypes.data, None, None, None, 0, C.byref(total))
            assert rc == 0 and np.all(np.diff(off).astype(np.int64) >= k), "the radius gives every query its k"
            tot = int(total.value)
            r["route_c"] = dict(radius=radius, results_per_query=tot / NQ)
            if tot < 2**31:
                ridx, rsqd = np.empty(tot, np.int32), np.empty(tot, np.float32)

                def route_c():
                    t = C.c_uint64(0)
                    assert ctx._L.flimo_radius_search(ctx._h, q.ctypes.data, NQ, radius, 0, off.ctypes.data, None, None, None, 0, C.byref(t)) == 0
                    assert ctx._L.flimo_radius_search(ctx._h, q.ctypes.data, NQ, radius, 1, off.ctypes.data, ridx.ctypes.data, rsqd.ctypes.data, None,
                                                      tot, C.byref(t)) == 0
                r["route_c"]["ms"] = timed(route_c, max(3, reps // 4), warm=1)
                r["route_c"]["knn_k_over_route_c"] = r["gate_off"]["ms"]["median"] / r["route_c"]["ms"]["median"]
            else:
                r["route_c"]["ms"] = None      # more than 2^31 - 1 results: the route does not exist at this k
        out["k"][str(k)] = r
        print(name, "k =", k, json.dumps(r), flush=True)
    stored = ctx.map_points()
    ctx.close()
    # (a) the reference: the oracle octree's knn, one thread and the best thread count up to 16
    if with_ref and not trace and name == "1M":
        import oracle_py
        oc = oracle_py.Octree()
        t0 = time.perf_counter()
        oc.update(stored)
        out["ref_octree_build_s"] = time.perf_counter() - t0
        sample = q[np.sort(np.random.RandomState(4096).choice(NQ, 4096, replace=False))]
        out["ref_cpu"] = {}
        for k in KS:
            per = {}
            for th in (1, 4, 8, 16):
                t0 = time.perf_counter(); oc.knn(sample, k, num_threads=th); per[th] = 1e3 * (time.perf_counter() - t0) * (NQ / 4096.0)
            best = min(per, key=per.get)
            out["ref_cpu"][str(k)] = dict(ms_one_thread_scaled_to_65536=per[1], best_threads=best, ms_best_scaled_to_65536=per[best])
        print(name, "oracle octree:", json.dumps(out["ref_cpu"]), flush=True)
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
