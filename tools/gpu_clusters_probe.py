"""Developer probe (GPU box): what flimo_map_clusters costs and what it replaces (profiles/clusters/README.md).

A 1M-point map as bench.py builds it, the Euclidean clusters of all its points at tol = 0.3, 0.5 and 1.0 m.  In the same process:
  device      flimo_map_clusters, 9 B per point come back (label, size, mask)
  mask_only   ... the mask and the stats alone: 1 B per point
  composed    the route that exists without the call: flimo_radius_search with the stored points uploaded as queries, the CSR
              (offsets and indices) downloaded, then connected components on the host -- scipy's where it imports, the plain
              union-find of tests/clusters_common.py otherwise; its labels turned into smallest indices
Milliseconds per call between two HIP events recorded around it (every call ends in a wait for its stream, so the events bracket
all of it: allocations, launches, copies back); warm, median of --reps (10).  The composed route: --reps-composed (3) times, its
parts by the host clock.  The two routes are compared: labels equal.
  --trace   a short run (three device calls per tol, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_clusters_probe.py --trace`: the link kernel's share

usage: python tools/gpu_clusters_probe.py [--reps N] [--reps-composed N] [--points N] [--trace] [--json FILE]"""
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
import torch
from fast_limo_amd import _lib, synth
from gpu_scan_fitness_probe import stats
import clusters_common as cc

BOX, TOLS = 100.0, (0.3, 0.5, 1.0)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def csr_once(ctx, pts, tol, cap):
    """The composed route's device half at its best: ONE flimo_radius_search (count, sum, fill inside it), indices only, into arrays
    sized beforehand (``cap`` from an untimed counting call)."""
    import ctypes as C
    off = np.zeros(len(pts) + 1, np.uint64)
    idx = np.empty(max(cap, 1), np.int32)
    total = C.c_uint64(0)
    ctx._chk(ctx._L.flimo_radius_search(ctx._h, pts.ctypes.data, len(pts), float(tol), 0, off.ctypes.data, idx.ctypes.data, None, None, cap,
                                        C.byref(total)))
    return off, idx[:int(total.value)]


def host_components(n, off, idx):
    """(labels as smallest indices, which implementation)."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
        k, comp = connected_components(sp.csr_matrix((np.ones(len(idx), np.int8), idx, off.astype(np.int64)), shape=(n, n)), directed=False)
        first = np.full(k, n, np.int64)
        np.minimum.at(first, comp, np.arange(n))
        return first[comp], "scipy"
    except ImportError:
        keep = rows < idx
        return cc.components(n, rows[keep], idx[keep].astype(np.int64)), "python union-find"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-composed", type=int, default=3)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    torch.cuda.init()
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(a.points, BOX, 1))
    pts = ctx.map_points()
    n = len(pts)
    if a.trace:
        for tol in TOLS:
            for _ in range(3):
                ctx.map_clusters(tol=tol)
        ctx.close()
        return
    res = dict(map_points=n, box=BOX, layout={k: (float(v) if k == "cell" else v) for k, v in ctx.map_index_layout().items()
                                                if k in ("cell", "nx", "ny", "nz")}, tols={})
    for tol in TOLS:
        r = dict(plan=cc.plan(ctx.map_index_layout(), tol))
        for name, want in (("device", ("label", "size", "mask")), ("mask_only", ("mask",))):
            fn = lambda: ctx.map_clusters(want=want, tol=tol, min_size=1, max_size=9)
            for _ in range(2):
                fn()
            r[name + "_ms"] = stats([event_ms(fn)[0] for _ in range(a.reps)])
        out = ctx.map_clusters(tol=tol)
        r["stats"] = out["stats"]
        if a.reps_composed < 1:                                  # (the device route alone: an A/B of two builds)
            res["tols"]["%g" % tol] = r
            continue
        parts = []
        cap = int(ctx.radius_count(pts, tol).sum())
        for _ in range(a.reps_composed):
            t0 = time.perf_counter()
            (ms, (off, idx)) = event_ms(lambda: csr_once(ctx, pts, tol, cap))
            t1 = time.perf_counter()
            lab, how = host_components(n, off, idx)
            t2 = time.perf_counter()
            parts.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t2 - t0), ms))
        p = np.array(parts)
        r["composed_ms"] = dict(radius_search=float(np.median(p[:, 0])), radius_search_events=float(np.median(p[:, 3])),
                                host_components=float(np.median(p[:, 1])), total=float(np.median(p[:, 2])), host=how)
        r["csr"] = dict(results=int(off[-1]), bytes=int(off.nbytes + idx.nbytes), results_per_point=float(off[-1]) / n)
        r["labels_equal"] = bool(np.array_equal(out["label"], lab))
        r["composed_over_device"] = r["composed_ms"]["total"] / r["device_ms"]["median"]
        res["tols"]["%g" % tol] = r
        print("%g" % tol, json.dumps(r), flush=True)
    ctx.close()
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
