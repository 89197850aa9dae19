"""Developer probe (GPU box): what flimo_map_planes costs and what it replaces (profiles/planes/README.md).

A map as bench.py builds it (1M stored points; --points), nh = 1 024 and 4 096 samples of api.corr_triplets, dist 0.05 m, no
constraints (every sample of distinct points survives: the count runs for all of them).  In the same process:
  device    flimo_map_planes: 16 B a hypothesis come back, 48 with the plane
  numpy     route (a): flimo_map_points downloads the map, then the restatement's count per hypothesis in numpy (float32, anchored);
            --numpy-hyps (16) hypotheses are timed and the figure is scaled to nh -- the route is linear in nh
  torch     route (b): a chunked torch formulation on the same device, ((P - A_j) * n_j).sum(-1), float32, |t| < dist, counts and
            float64 sums of squares per hypothesis; the normals and anchors are given to it (the solve is not timed)
Milliseconds per call between two HIP events recorded around it (every call ends in a wait for its stream, so the events bracket
all of it: allocations, launches, copies back); warm, median of --reps (10).  Counts are compared: the numpy route's must equal
the call's; torch sums a dot product its own way, so its counts may differ by the points within an ulp of the gate (reported).
  --only-device   the call alone (an A/B of two builds of the library: FLIMO_HIP_LIB=...)

usage: python tools/gpu_planes_probe.py [--reps N] [--points N ...] [--nh N ...] [--only-device] [--json FILE]"""
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
from fast_limo_amd import _lib, api, synth
from gpu_scan_fitness_probe import stats
import planes_common as pc

BOX, DIST = 100.0, 0.05


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def torch_route(P, A, Nf, dist, chunk):
    """counts [nh] and float64 sums of squares [nh] on the device, chunk hypotheses at a time ([chunk, N, 3] float32 in flight)."""
    cnt, ssq = [], []
    for a in range(0, A.shape[0], chunk):
        t = ((P[None, :, :] - A[a:a + chunk, None, :]) * Nf[a:a + chunk, None, :]).sum(-1)
        inside = t.abs() < dist
        cnt.append(inside.sum(1))
        ssq.append(torch.where(inside, t.double() * t.double(), torch.zeros((), dtype=torch.float64, device=t.device)).sum(1))
    return torch.cat(cnt).cpu().numpy(), torch.cat(ssq).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, nargs="+", default=[1000000])
    ap.add_argument("--nh", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--numpy-hyps", type=int, default=16)
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    torch.cuda.init()
    dev = torch.device("cuda:0")
    res = dict(lib=os.environ.get("FLIMO_HIP_LIB", "libflimo_hip.so"), dist=DIST, runs=[])
    for points in a.points:
        ctx = _lib.HipCtx(0)
        ctx.map_config()
        ctx.map_add(synth.box_world_map(points, BOX, 1))
        n = ctx.map_size()
        for nh in a.nh:
            tri = api.corr_triplets(n, nh, 0)
            r = dict(map_points=n, nh=nh, slabs=(n + pc.SLAB - 1) // pc.SLAB)
            for name, want in (("device", ("plane",)), ("device_no_plane", ())):
                fn = lambda: ctx.map_planes(tri, want=want, dist=DIST)
                for _ in range(2):
                    fn()
                r[name + "_ms"] = stats([event_ms(fn)[0] for _ in range(a.reps)])
            out = ctx.map_planes(tri, dist=DIST)
            ok = out["status"] == pc.OK
            r["survivors"] = int(ok.sum())
            r["tests_per_second"] = float(ok.sum()) * n / (1e-3 * r["device_ms"]["median"])
            if not a.only_device:
                # (a) download + numpy per hypothesis
                t0 = time.perf_counter()
                pts = ctx.map_points()
                t1 = time.perf_counter()
                js = np.flatnonzero(ok)[:a.numpy_hyps]
                cnt = []
                for j in js:
                    t = pc.signed_t(pts, out["plane"][j, :3].astype(np.float32), pts[tri[j, 0]])
                    cnt.append(int((np.abs(t) < np.float32(DIST)).sum()))
                t2 = time.perf_counter()
                per = 1e3 * (t2 - t1) / max(len(js), 1)
                r["numpy_ms"] = dict(download=1e3 * (t1 - t0), per_hypothesis=per, total_scaled=1e3 * (t1 - t0) + per * nh, timed_hyps=len(js))
                r["numpy_counts_equal"] = bool(np.array_equal(cnt, out["inliers"][js]))
                # (b) torch on the same device
                P = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
                A = torch.from_numpy(np.ascontiguousarray(pts[tri[:, 0]])).to(dev)
                Nf = torch.from_numpy(np.nan_to_num(out["plane"][:, :3]).astype(np.float32)).to(dev)
                chunk = max(1, min(nh, (1 << 27) // n))                      # [chunk, N, 3] float32 of at most 1.5 GiB
                fn = lambda: torch_route(P, A, Nf, DIST, chunk)
                for _ in range(2):
                    fn()
                r["torch_ms"] = stats([event_ms(fn)[0] for _ in range(max(a.reps // 2, 3))])
                tc, ts = fn()
                r["torch_chunk"] = chunk
                r["torch_count_max_diff"] = int(np.abs(tc[ok].astype(np.int64) - out["inliers"][ok]).max())
                r["torch_sum_max_rel_diff"] = float(np.max(np.abs(ts[ok] - out["sum_sq"][ok]) / np.maximum(out["sum_sq"][ok], 1e-300)))
                r["numpy_over_device"] = r["numpy_ms"]["total_scaled"] / r["device_ms"]["median"]
                r["torch_over_device"] = r["torch_ms"]["median"] / r["device_ms"]["median"]
                del P, A, Nf
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
        ctx.close()
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
