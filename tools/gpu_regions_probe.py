"""Developer probe (GPU box): what flimo_map_regions / flimo_map_region_list cost and what they replace (profiles/regions/README.md).

A 1M-point map as bench.py builds it; regions at tol 0.3 and 0.5 m, normal_k 16, min_cos = cos 20 deg, max_curv 0.05.  Steps, each a
fresh child process under its own time limit (the parent never opens the GPU; the first step that fails, faults or runs out of time
ends the run):
  device    per tol, milliseconds between two HIP events around the call (every call ends in a wait for its stream, so
            allocations, launches and copies back are inside), warm, median of --reps:
              regions        flimo_map_regions, border on, 9 B a point back (label, size, mask)
              no_border      ... border off
              no_link        ... at tol 0: the normals, init, flatten, count and finish without the link launch; regions - no_link is
                             the link launch with the border, no_border - no_link without it
              clusters       flimo_map_clusters at the same tol, 9 B a point back: what the normal test in the walk costs
              list           flimo_map_region_list, regions of at least 100 points: label, count, centroid, cov
              list_numpy     the route the listing replaces: flimo_map_points + the labels + np.add.at by label (count and
                             centroid sums, no covariance)
  composed  per tol, the route flimo_map_regions replaces, border off: flimo_map_normals_range downloaded, ONE flimo_radius_search with
            the stored points as queries and the CSR downloaded, the predicate in numpy over the CSR's pairs, connected components
            on the host (scipy's where it imports, the plain union-find of tests/clusters_common.py otherwise).  Labels compared
            with the device's.
  --trace   a short run (three device calls per tol, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_regions_probe.py --trace`: normals / link / the rest per kernel

usage: python tools/gpu_regions_probe.py [--reps N] [--points N] [--steps device composed] [--trace] [--json FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX, TOLS = 100.0, (0.3, 0.5)
CFG = dict(normal_k=16, min_cos=0.93969262, max_curv=0.05)


def _imports():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _map(a):
    import torch
    from fast_limo_amd import _lib, synth
    torch.cuda.init()
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(a.points, BOX, 1))
    return torch, ctx


def step_trace(a):
    _imports()
    torch, ctx = _map(a)
    for tol in TOLS:
        for _ in range(3):
            ctx.map_regions(tol=tol, border=1, **CFG)
    ctx.map_region_list(tol=TOLS[0], border=1, min_size=100, **CFG)
    ctx.close()
    return dict(step="trace")


def step_device(a):
    _imports()
    import numpy as np
    torch, ctx = _map(a)
    from gpu_scan_fitness_probe import stats
    import clusters_common as cc
    n = ctx.map_size()
    res = dict(step="device", map_points=n, box=BOX, cfg=CFG, tols={},
               layout={k: (float(v) if k == "cell" else v) for k, v in ctx.map_index_layout().items() if k in ("cell", "nx", "ny", "nz")})
    all3 = ("label", "size", "mask")
    for tol in TOLS:
        r = dict(plan=cc.plan(ctx.map_index_layout(), tol))
        cases = dict(regions=lambda: ctx.map_regions(want=all3, tol=tol, border=1, **CFG),
                     no_border=lambda: ctx.map_regions(want=all3, tol=tol, border=0, **CFG),
                     no_link=lambda: ctx.map_regions(want=all3, tol=0.0, border=1, **CFG),
                     clusters=lambda: ctx.map_clusters(want=all3, tol=tol),
                     list=lambda: ctx.map_region_list(want=("label", "count", "centroid", "cov"), tol=tol, border=1, min_size=100, **CFG))
        for name, fn in cases.items():
            fn(); fn()
            r[name + "_ms"] = stats([event_ms(torch, fn)[0] for _ in range(a.reps)])
        out = cases["regions"]()
        r["stats"] = out["stats"]
        r["stats_no_border"] = cases["no_border"]()["stats"]
        li = cases["list"]()
        r["listed"] = dict(nr=li["nr"], largest=int(li["count"].max()) if li["nr"] else 0)

        def by_numpy():
            pts = ctx.map_points().astype(np.float64)
            lab = ctx.map_regions(want=("label", "size"), tol=tol, border=1, **CFG)
            keep = lab["size"] >= 100
            labs, inv = np.unique(lab["label"][keep], return_inverse=True)
            cnt = np.bincount(inv, minlength=len(labs))
            s = np.zeros((len(labs), 3))
            np.add.at(s, inv, pts[keep])
            return labs, cnt, s / cnt[:, None]

        t = []
        for _ in range(max(a.reps // 3, 2)):
            t0 = time.perf_counter()
            labs, cnt, cen = by_numpy()
            t.append(1e3 * (time.perf_counter() - t0))
        r["list_numpy_ms"] = stats(t)
        r["list_equal"] = bool(np.array_equal(labs, li["label"]) and np.array_equal(cnt, li["count"]) and np.allclose(cen, li["centroid"], rtol=0, atol=1e-9))
        r["link_with_border_ms"] = r["regions_ms"]["median"] - r["no_link_ms"]["median"]
        r["link_without_border_ms"] = r["no_border_ms"]["median"] - r["no_link_ms"]["median"]
        r["regions_over_clusters"] = r["regions_ms"]["median"] / r["clusters_ms"]["median"]
        res["tols"]["%g" % tol] = r
        print("%g" % tol, json.dumps(r), flush=True)
    ctx.close()
    return res


def step_composed(a):
    _imports()
    import ctypes as C
    import numpy as np
    torch, ctx = _map(a)
    import clusters_common as cc
    pts = ctx.map_points()
    n = len(pts)
    res = dict(step="composed", map_points=n, tols={})
    for tol in TOLS:
        want = ctx.map_regions(want=("label",), tol=tol, border=0, **CFG)["label"]
        cap = int(ctx.radius_count(pts, tol).sum())
        parts = []
        for _ in range(a.reps_composed):
            t0 = time.perf_counter()
            nrm = ctx.normals_range(0, n, CFG["normal_k"], want=())["normal"]
            t1 = time.perf_counter()
            off = np.zeros(n + 1, np.uint64)
            idx = np.empty(max(cap, 1), np.int32)
            total = C.c_uint64(0)
            ctx._chk(ctx._L.flimo_radius_search(ctx._h, pts.ctypes.data, n, float(tol), 0, off.ctypes.data, idx.ctypes.data, None, None, cap,
                                                C.byref(total)))
            idx = idx[:int(total.value)]
            t2 = time.perf_counter()
            rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))
            sm = np.isfinite(nrm).all(1) & (nrm[:, 3] <= np.float32(CFG["max_curv"]))
            a3, b3 = nrm[rows, :3], nrm[idx, :3]
            dot = a3[:, 0] * b3[:, 0] + (a3[:, 1] * b3[:, 1] + a3[:, 2] * b3[:, 2])
            keep = (rows < idx) & sm[rows] & sm[idx] & (np.abs(dot) >= np.float32(CFG["min_cos"]))
            I, J = rows[keep], idx[keep].astype(np.int64)
            t3 = time.perf_counter()
            try:
                import scipy.sparse as sp
                from scipy.sparse.csgraph import connected_components
                k, comp = connected_components(sp.coo_matrix((np.ones(len(I), np.int8), (I, J)), shape=(n, n)).tocsr(), directed=False)
                first = np.full(k, n, np.int64)
                np.minimum.at(first, comp, np.arange(n))
                lab, how = first[comp], "scipy"
            except ImportError:
                lab, how = cc.components(n, I, J), "python union-find"
            lab = np.where(sm, lab, -1)
            t4 = time.perf_counter()
            parts.append([1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t4 - t3), 1e3 * (t4 - t0)])
        p = np.median(np.array(parts), axis=0)
        r = dict(normals_download=float(p[0]), radius_search=float(p[1]), numpy_predicate=float(p[2]), host_components=float(p[3]), total=float(p[4]),
                 host=how, csr_results=int(total.value), edges=int(len(I)), labels_equal=bool(np.array_equal(lab, want)))
        res["tols"]["%g" % tol] = r
        print("%g" % tol, json.dumps(r), flush=True)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-composed", type=int, default=2)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--steps", nargs="+", default=["device", "composed"])
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace:                                             # (under the profiler: this process is the one it follows)
        step_trace(a)
        return 0
    if a.child:
        res = dict(device=step_device, composed=step_composed)[a.child](a)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    # the parent: every step a child of its own under a time limit; nothing more is started after a step that did not end well
    results = []
    for name in a.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--reps-composed", str(a.reps_composed),
               "--points", str(a.points)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping" % (name, a.step_timeout), flush=True)
            break
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print("step %s ended with status %d: stopping" % (name, p.returncode), flush=True)
            break
        results += [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as fh:
                json.dump(dict(results=results), fh, indent=1)
    return 0 if len(results) == len(a.steps) else 1


if __name__ == "__main__":
    sys.exit(main())
