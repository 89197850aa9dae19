"""Developer probe (GPU box): what flimo_scan_fitness costs and what it replaces (profiles/scan_fitness/README.md).

A 1M-point map as bench.py builds it, a 65 536-point scan of the same box, 64 poses within +-1 m / +-10 degrees (yaw) of the true one,
a gate of 1 m.  In the same process, the candidates taking turns within every repeat:
  fused            flimo_scan_fitness, two numbers per pose come back
  fused_nn         ... with nn_sqd and nn_idx (8 B per pair come back)
  composed         the route the call replaces: per pose flimo_scan_to_world (a download), flimo_knn_k(k = 1) on those points (an
                   upload, 12 B per point back), the count and the float64 sum in numpy
Milliseconds per batch of 64 poses: host clock around the calls, each of which ends in a stream wait; arrays sized beforehand;
warm-up, then --reps repeats: median, min, max.  The two routes are compared: inliers equal, sums within n * 2^-52 of each other.
  --trace   a short run (a few calls per case, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_scan_fitness_probe.py --trace`

usage: python tools/gpu_scan_fitness_probe.py [--reps N] [--trace] [--json FILE]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fast_limo_amd import _lib, synth

N_MAP, BOX, N_SCAN, N_POSES, GATE = 1000000, 100.0, 65536, 64, 1.0


def stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def taking_turns(cases, reps, warm=2):
    """Every case once per repeat, the order rotating; per case the statistics of its times [ms]."""
    names = list(cases)
    for _ in range(warm):
        for n in names:
            cases[n]()
    t = {n: [] for n in names}
    for r in range(reps):
        for j in range(len(names)):
            n = names[(j + r) % len(names)]
            t0 = time.perf_counter(); cases[n](); t[n].append(1e3 * (time.perf_counter() - t0))
    return {n: stats(v) for n, v in t.items()}


def poses_around_the_true_one(n, seed):
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 26))
    for j in range(n):
        dx, dy, dyaw = rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(-10, 10)
        R = synth.rpy_to_R(*[math.radians(a) for a in (synth.T_STAR_RPY_DEG[0], synth.T_STAR_RPY_DEG[1], synth.T_STAR_RPY_DEG[2] + dyaw)])
        w = 0.5 * math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
        out[j, 0:3] = (synth.T_STAR_T[0] + dx, synth.T_STAR_T[1] + dy, synth.T_STAR_T[2])
        out[j, 3:7] = ((R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w)
        out[j, 10] = 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    reps, warm = (2, 1) if a.trace else (a.reps, 2)

    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(N_MAP, BOX, 1))
    ctx.scan_set(np.ascontiguousarray(synth.box_world_scan_random(N_SCAN, BOX, 2)[:, :3]))
    n, n_map = ctx.scan_size(), ctx.map_size()
    x = poses_around_the_true_one(N_POSES, 11)
    L, h = ctx._L, ctx._h
    inl, s = np.empty(N_POSES, np.int32), np.empty(N_POSES)
    nn_sqd, nn_idx = np.empty((N_POSES, n), np.float32), np.empty((N_POSES, n), np.int32)
    world = np.empty((n, 3), np.float32)
    idx, sqd, cnt = np.empty((n, 1), np.int32), np.empty((n, 1), np.float32), np.empty(n, np.int32)
    c_inl, c_s = np.empty(N_POSES, np.int32), np.empty(N_POSES)

    def fused(nn):
        assert L.flimo_scan_fitness(h, x.ctypes.data, N_POSES, GATE, inl.ctypes.data, s.ctypes.data, nn_sqd.ctypes.data if nn else None,
                                    nn_idx.ctypes.data if nn else None) == 0

    def composed():
        for j in range(N_POSES):
            assert L.flimo_scan_to_world(h, x[j], world.ctypes.data, n) == 0
            assert L.flimo_knn_k(h, world.ctypes.data, n, 1, GATE, idx.ctypes.data, sqd.ctypes.data, None, cnt.ctypes.data) == 0
            c_inl[j] = cnt.sum()
            c_s[j] = sqd[:, 0].astype(np.float64).sum()      # (the padding of an empty query is 0)

    cases = {"fused": lambda: fused(False), "fused_nn": lambda: fused(True), "composed": composed}
    res = dict(map_points=n_map, box=BOX, scan_points=n, poses=N_POSES, gate=GATE, ms=taking_turns(cases, reps, warm))
    fused(False); composed()
    res["agreement"] = dict(inliers_equal=bool(np.array_equal(inl, c_inl)), inliers_min=int(inl.min()), inliers_max=int(inl.max()),
                            sum_max_rel_diff=float(np.max(np.abs(s - c_s) / np.maximum(c_s, 1e-300))), sum_bound=n * 2.0 ** -52)
    res["pairs_per_second_fused"] = N_POSES * n / (1e-3 * res["ms"]["fused"]["median"])
    print(json.dumps(res), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
