"""Developer probe (GPU box): what flimo_scan_linearize costs and what it replaces (profiles/scan_linearize/README.md).

The fitness probe's workload: a 1M-point map as bench.py builds it, a 65 536-point scan of the same box, 64 poses within +-1 m /
+-10 degrees (yaw) of the true one, a gate of 1 m, max_curv 0.05, at k = 5 and k = 20.  In the same process, the candidates taking
turns within every repeat:
  fused_k*         flimo_scan_linearize, 29 numbers per pose come back
  fused_rows_k5    ... with rows and pair_cnt (60 B per pair come back)
  composed_k*      the route that exists without the call: per pose flimo_scan_to_world (a download), flimo_map_normals on those
                   points with centroid and eig (an upload, 92 B per point back), the terms and their sums in numpy
  align            api.scan_align, 12 iterations over the 64 poses at k = 5 (once per repeat)
Milliseconds per batch of 64 poses: host clock around the calls, each of which ends in a stream wait; warm-up, then --reps
repeats: median, min, max.  The two routes are compared: valid equal, sums within n * 2^-52 * sum|term| of each other.
  --trace   a short run (a few fused calls per k, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_scan_linearize_probe.py --trace`

usage: python tools/gpu_scan_linearize_probe.py [--reps N] [--trace] [--json FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from fast_limo_amd import _lib, api, synth
from gpu_scan_fitness_probe import poses_around_the_true_one, taking_turns

N_MAP, BOX, N_SCAN, N_POSES, GATE, MIN_PTS, MAX_CURV = 1000000, 100.0, 65536, 64, 1.0, 3, 0.05
IU = np.triu_indices(6)


def pose_R(x26):
    """The rotation of pose_from_x26's float32 matrix, widened."""
    f = np.float32
    q = [f(v) for v in x26[3:7]]
    tx, ty, tz = f(2) * q[0], f(2) * q[1], f(2) * q[2]
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * q[3], ty * q[3], tz * q[3], tx * q[0], ty * q[0], tz * q[0], ty * q[1], tz * q[1], tz * q[2]
    return np.array([[f(1) - (tyy + tzz), txy - twz, txz + twy], [txy + twz, f(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, f(1) - (txx + tyy)]], np.float32).astype(np.float64)


def terms_and_sums(x26, scan64, w, cnt, centroid, eig):
    """The numpy end of the composed route: (valid, H [21], g [6], cost, sum|J_a J_b| [21])."""
    l, nr = eig[:, :3], eig[:, 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        tr = l[:, 0] + l[:, 1] + l[:, 2]
        ok = (cnt >= max(3, MIN_PTS)) & (np.where(tr == 0.0, 0.0, l[:, 0] / tr) <= np.float64(np.float32(MAX_CURV)))
    wd, c, nr, p = w[ok].astype(np.float64), centroid[ok], nr[ok], scan64[ok]
    R = pose_R(x26)
    d = nr[:, 0] * (wd[:, 0] - c[:, 0]) + (nr[:, 1] * (wd[:, 1] - c[:, 1]) + nr[:, 2] * (wd[:, 2] - c[:, 2]))
    a = nr @ R
    J = np.concatenate([a, np.cross(p, a)], axis=1)
    return int(ok.sum()), (J.T @ J)[IU], J.T @ d, float(d @ d), (np.abs(J).T @ np.abs(J))[IU]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(synth.box_world_map(N_MAP, BOX, 1))
    scan = np.ascontiguousarray(synth.box_world_scan_random(N_SCAN, BOX, 2)[:, :3])
    ctx.scan_set(scan)
    n, n_map = ctx.scan_size(), ctx.map_size()
    scan64 = ctx.scan_get().astype(np.float64)
    x = poses_around_the_true_one(N_POSES, 11)
    L, h = ctx._L, ctx._h
    valid, H, g, cost = np.empty(N_POSES, np.int32), np.empty((N_POSES, 21)), np.empty((N_POSES, 6)), np.empty(N_POSES)
    rows, pair_cnt = np.empty((N_POSES, n, 7)), np.empty((N_POSES, n), np.int32)
    world, normal, cnt = np.empty((n, 3), np.float32), np.empty((n, 4), np.float32), np.empty(n, np.int32)
    centroid, eig = np.empty((n, 3)), np.empty((n, 6))
    comp = dict(valid=np.empty(N_POSES, np.int32), H=np.empty((N_POSES, 21)), g=np.empty((N_POSES, 6)), cost=np.empty(N_POSES),
                absH=np.empty((N_POSES, 21)))

    def fused(k, with_rows=False):
        assert L.flimo_scan_linearize(h, x.ctypes.data, N_POSES, k, GATE, MIN_PTS, MAX_CURV, valid.ctypes.data, H.ctypes.data, g.ctypes.data,
                                      cost.ctypes.data, rows.ctypes.data if with_rows else None, pair_cnt.ctypes.data if with_rows else None) == 0

    def composed(k):
        for j in range(N_POSES):
            assert L.flimo_scan_to_world(h, x[j], world.ctypes.data, n) == 0
            assert L.flimo_map_normals(h, world.ctypes.data, n, k, GATE, MIN_PTS, None, normal.ctypes.data, cnt.ctypes.data, centroid.ctypes.data,
                                       None, eig.ctypes.data) == 0
            comp["valid"][j], comp["H"][j], comp["g"][j], comp["cost"][j], comp["absH"][j] = terms_and_sums(x[j], scan64, world, cnt, centroid, eig)

    if a.trace:
        for k in (5, 20):
            for _ in range(3):
                fused(k)
        ctx.close()
        return
    cases = {"fused_k5": lambda: fused(5), "fused_k20": lambda: fused(20), "fused_rows_k5": lambda: fused(5, True),
             "composed_k5": lambda: composed(5), "composed_k20": lambda: composed(20)}
    res = dict(map_points=n_map, box=BOX, scan_points=n, poses=N_POSES, gate=GATE, min_pts=MIN_PTS, max_curv=MAX_CURV,
               ms=taking_turns(cases, a.reps, 1), agreement={})
    for k in (5, 20):
        fused(k); composed(k)
        res["agreement"][f"k{k}"] = dict(valid_equal=bool(np.array_equal(valid, comp["valid"])), valid_min=int(valid.min()), valid_max=int(valid.max()),
                                         H_worst_of_bound=float(np.max(np.abs(H - comp["H"]) / (n * 2.0 ** -52 * comp["absH"]))))
        res[f"pairs_per_second_fused_k{k}"] = N_POSES * n / (1e-3 * res["ms"][f"fused_k{k}"]["median"])
    t = []
    for _ in range(max(2, a.reps // 2)):
        t0 = time.perf_counter()
        out = api.scan_align(ctx, x, k=5, max_dist=GATE, min_pts=MIN_PTS, max_curv=MAX_CURV, iters=12)
        t.append(1e3 * (time.perf_counter() - t0))
    err = np.linalg.norm(out["x26"][:, :3] - np.asarray(synth.T_STAR_T), axis=1)
    res["align_12_iterations_ms"] = dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), n=len(t))
    res["align_position_error_max_m"] = float(err.max())
    res["align_status_counts"] = [int(c) for c in np.bincount(out["status"], minlength=3)]
    print(json.dumps(res), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
