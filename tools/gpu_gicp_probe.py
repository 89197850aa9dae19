"""Developer probe (GPU box): what the GICP entries cost beside the two passes they stand between (profiles/gicp/README.md).

The linearize and NDT probes' workload: a 1M-point map as bench.py builds it, a 65 536-point scan of the same box, 1 and 64 poses
within +-1 m / +-10 degrees (yaw) of the true one.  Every step is a child process of this script under its own time limit; the
first step that fails, faults or runs out of time ends the run.  Steps:
  build             flimo_gicp_build alone (k = 20, no gate, FLIMO_GICP_PLANE at eps 1e-3): ms and the points with a covariance;
                    beside it the scan's covariances by api.gicp_covs on a context whose map is the scan (once, host clock)
  gicp              flimo_scan_gicp(gate 1 m) at 1 and 64 poses: ms per call, pairs per second; with pair_idx / pair_m at 64
  linearize         flimo_scan_linearize(k = 5, gate 1 m) at 1 and 64 poses, the same shapes
  fitness           flimo_scan_fitness(gate 1 m) at 1 and 64 poses: the search a GICP pass shares with it
  trace             a few calls at 64 poses, nothing else: the two search launches against gicp_reduce_kernel are read from
                    `rocprofv3 --kernel-trace --stats -- python tools/gpu_gicp_probe.py --step trace`
Milliseconds: host clock around the calls, each of which ends in a stream wait; one warm-up, then --reps repeats: median, min, max.

usage: python tools/gpu_gicp_probe.py [--reps N] [--json FILE] [--step NAME]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_MAP, BOX, N_SCAN, GATE = 1000000, 100.0, 65536, 1.0
K_COV, EPS = 20, 1e-3
STEPS = (("build", 300), ("gicp", 300), ("linearize", 300), ("fitness", 300))      # (name, seconds)


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    t.sort()
    return dict(median=t[len(t) // 2], min=t[0], max=t[-1], n=len(t))


def scan_covs(scan):
    """(covariances [n, 6] of the scan's points, seconds it took) by a second context whose map is the scan."""
    from fast_limo_amd import _lib, api
    t0 = time.perf_counter()
    sctx = _lib.HipCtx(0)
    sctx.map_config(downsample=False)
    sctx.map_add(scan)
    cov = api.gicp_covs(sctx, k=K_COV, rule=_lib.GICP_PLANE, eps=EPS)
    sctx.close()
    return cov, time.perf_counter() - t0


def step(name, reps):
    import numpy as np
    from fast_limo_amd import _lib, synth
    from gpu_scan_fitness_probe import poses_around_the_true_one
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(N_MAP, BOX, 1))
    scan = np.ascontiguousarray(synth.box_world_scan_random(N_SCAN, BOX, 2)[:, :3])
    ctx.scan_set(scan)
    n = ctx.scan_size()
    x = poses_around_the_true_one(64, 11)
    res = dict(map_points=ctx.map_size(), scan_points=n)
    if name == "build":
        res["map"] = dict(ms=timed(lambda: ctx.gicp_build(K_COV, float("inf"), 3, _lib.GICP_PLANE, EPS), reps), n_cov=ctx.gicp_info()["n_cov"])
        cov, secs = scan_covs(scan)
        res["scan"] = dict(seconds=secs, n_cov=int(np.isfinite(cov).all(1).sum()))
    elif name in ("gicp", "trace"):
        ctx.gicp_build(K_COV, float("inf"), 3, _lib.GICP_PLANE, EPS)
        ctx.scan_cov_set(scan_covs(scan)[0])
        if name == "trace":
            for _ in range(3):
                ctx.scan_gicp(x, GATE)
        else:
            for m in (1, 64):
                ms = timed(lambda: ctx.scan_gicp(x[:m], GATE), reps)
                out = ctx.scan_gicp(x[:m], GATE)
                res[f"poses_{m}"] = dict(ms=ms, pairs_per_second=m * n / (1e-3 * ms["median"]), valid_min=int(out["valid"].min()))
            res["poses_64_with_pairs"] = dict(ms=timed(lambda: ctx.scan_gicp(x, GATE, want_pairs=True), reps))
    elif name == "linearize":
        for m in (1, 64):
            ms = timed(lambda: ctx.scan_linearize(x[:m], 5, GATE, 3, 0.05), reps)
            res[f"k5_poses_{m}"] = dict(ms=ms, pairs_per_second=m * n / (1e-3 * ms["median"]))
    elif name == "fitness":
        for m in (1, 64):
            ms = timed(lambda: ctx.scan_fitness(x[:m], GATE), reps)
            res[f"poses_{m}"] = dict(ms=ms, pairs_per_second=m * n / (1e-3 * ms["median"]))
    else:
        raise SystemExit(f"unknown step {name}")
    ctx.close()
    print("STEP " + json.dumps({name: res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        step(a.step, a.reps)
        return
    res = {}
    for name, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            res[name] = dict(error=f"ran past {limit} s")
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP ")]
        if p.returncode != 0 or not lines:
            res[name] = dict(error=f"exit code {p.returncode}", stderr=p.stderr[-2000:])
            break      # nothing more is started on the GPU after a step that failed
        res.update(json.loads(lines[-1][5:]))
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
