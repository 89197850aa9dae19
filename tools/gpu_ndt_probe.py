"""Developer probe (GPU box): what the NDT entries cost and what they replace (profiles/ndt/README.md).

The linearize probe's workload: a 1M-point map as bench.py builds it, a 65 536-point scan of the same box, 1 and 64 poses within
+-1 m / +-10 degrees (yaw) of the true one.  Every step is a child process of this script under its own time limit; the first
step that fails, faults or runs out of time ends the run.  Steps:
  build             flimo_ndt_build alone at leaf 0.5, 1.0 and 2.0 (min_pts 6, eig_ratio 0.01): cells and ms
  ndt               flimo_scan_ndt at every (leaf, hood 1 / 7, 1 / 64 poses): ms per call, pairs per second
  linearize         flimo_scan_linearize(k = 5, gate 1 m) at 1 and 64 poses, the same shapes
  composed          the route without the call, per pose: flimo_scan_to_world (a download), voxel keys and np.searchsorted over
                    the downloaded model's keys, the own cell's terms and their sums in numpy (hood 1, leaf 1.0)
  trace             a few calls at leaf 1.0, hood 7, 64 poses, nothing else: stage 1 (ndt_lookup_kernel) against stage 2
                    (ndt_reduce_kernel) are read from
                    `rocprofv3 --kernel-trace --stats -- python tools/gpu_ndt_probe.py --step trace`
Milliseconds: host clock around the calls, each of which ends in a stream wait; one warm-up, then --reps repeats: median, min, max.

usage: python tools/gpu_ndt_probe.py [--reps N] [--json FILE] [--step NAME]"""
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
LEAVES, MIN_PTS, EIG_RATIO, OUTLIER = (0.5, 1.0, 2.0), 6, 0.01, 0.55
STEPS = (("build", 240), ("ndt", 300), ("linearize", 300), ("composed", 300))      # (name, seconds)


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    t.sort()
    return dict(median=t[len(t) // 2], min=t[0], max=t[-1], n=len(t))


def step(name, reps):
    import numpy as np
    from fast_limo_amd import _lib, api, synth
    from gpu_scan_fitness_probe import poses_around_the_true_one
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(N_MAP, BOX, 1))
    ctx.scan_set(np.ascontiguousarray(synth.box_world_scan_random(N_SCAN, BOX, 2)[:, :3]))
    n = ctx.scan_size()
    x = poses_around_the_true_one(64, 11)
    res = dict(map_points=ctx.map_size(), scan_points=n)
    if name == "build":
        for slot, leaf in enumerate(LEAVES):
            res[f"leaf_{leaf}"] = dict(ms=timed(lambda: ctx.ndt_build(slot, leaf, MIN_PTS, EIG_RATIO), reps), cells=ctx.ndt_info(slot)["cells"])
    elif name in ("ndt", "trace"):
        for slot, leaf in enumerate(LEAVES):
            ctx.ndt_build(slot, leaf, MIN_PTS, EIG_RATIO)
        if name == "trace":
            for _ in range(3):
                ctx.scan_ndt(1, x, api.ndt_params(OUTLIER, 1.0)[1], hood=7)
        else:
            for slot, leaf in enumerate(LEAVES):
                d2 = api.ndt_params(OUTLIER, leaf)[1]
                for hood in (1, 7):
                    for m in (1, 64):
                        ms = timed(lambda: ctx.scan_ndt(slot, x[:m], d2, hood=hood), reps)
                        out = ctx.scan_ndt(slot, x[:m], d2, hood=hood)
                        res[f"leaf_{leaf}_hood_{hood}_poses_{m}"] = dict(ms=ms, pairs_per_second=m * n / (1e-3 * ms["median"]),
                                                                          valid_min=int(out["valid"].min()), cells_max=int(out["cells"].max()))
    elif name == "linearize":
        for m in (1, 64):
            ms = timed(lambda: ctx.scan_linearize(x[:m], 5, GATE, 3, 0.05), reps)
            res[f"k5_poses_{m}"] = dict(ms=ms, pairs_per_second=m * n / (1e-3 * ms["median"]))
    elif name == "composed":
        ctx.ndt_build(0, 1.0, MIN_PTS, EIG_RATIO)
        model = ctx.ndt_cells(0)
        d2 = api.ndt_params(OUTLIER, 1.0)[1]
        h = np.int64(1 << 20)
        keys = ((model["ijk"][:, 2] + h) << 42) | ((model["ijk"][:, 1] + h) << 21) | (model["ijk"][:, 0] + h)

        def composed(m):
            for j in range(m):
                w = ctx.scan_to_world(x[j])
                c = np.floor(w * np.float32(1.0)).astype(np.int64)
                k = ((c[:, 2] + h) << 42) | ((c[:, 1] + h) << 21) | (c[:, 0] + h)
                at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
                hit = keys[at] == k
                r = w[hit].astype(np.float64) - model["mean"][at[hit]]
                d = np.einsum("nka,na->nk", model["evec"][at[hit]], r)
                e = np.exp(-0.5 * d2 * np.sum(model["wgt"][at[hit]] * d * d, axis=1))
                float(e.sum())
        for m in (1, 64):
            res[f"hood_1_leaf_1.0_poses_{m}"] = dict(ms=timed(lambda: composed(m), max(1, reps // 2)), note="the score alone: H and g are not formed")
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
