"""Developer probe (GPU box): what a crop of the map costs and what it buys ("The local map").

  crops     time of flimo_map_crop_box (wall clock, the call ends after a stream wait) on a 1M-point map losing about 10 % and on
            a 20M-point map cut to about 1M, medians; beside each what a caller WITHOUT the entry would have to do for the same
            meaning: flimo_map_points -> host filter -> flimo_map_clear -> flimo_map_add of the kept points in one batch.
            (--crops-only: just the crops, for a rocprofv3 --kernel-trace --stats run that times crop_compact_kernel alone)
  step      the 256k x 20M step of bench.py (roofline.hbm_regime: GPU deskew + iterated update of a resident scan) before and
            after a crop of the map to the scan's surroundings; flimo_map_index_bytes before / after
  corridor  a corridor drive with the policy on and off: map size, index bytes and ms per sweep at its end

usage: python tools/gpu_local_map_probe.py [crops] [step] [corridor] [--crops-only] [--reps N] [--json FILE]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fast_limo_amd import _lib, api, synth

CAPS = dict(MAX_NUM_PC2MATCH=10**7, MAX_NUM_MATCHES=10**7)
HBM = dict(rings=128, azimuths=2048, map_points=20000000, box=447.0)      # bench.py's HBM_REGIME (BASELINE.json configs[3])


def inside(p, lo, hi):
    return np.all((p >= lo) & (p <= hi), axis=1)


def med(v):
    return float(np.median(v)) if len(v) else None


def crops(reps, crops_only):
    out = {}
    cases = [("1M_minus_10pct", synth.box_world_map(1000000, 100.0, 1), np.float32([-1e3, -1e3, -1e3]), None),
             ("20M_to_1M", synth.box_world_map(HBM["map_points"], HBM["box"], 1), np.float32([-100, -100, -50]), np.float32([100, 100, 50]))]
    for name, mp, lo, hi in cases:
        if hi is None:                                                   # everything below the 90th percentile of x
            hi = np.float32([np.quantile(mp[:, 0], 0.9), 1e3, 1e3])
        n_rep = reps
        ctx = _lib.HipCtx(0)
        ctx.map_config()
        t_crop, t_manual, kept_n, n0 = [], [], 0, 0
        for r in range(n_rep):
            ctx.map_clear(); ctx.map_add(mp)
            n0 = ctx.map_size()
            t0 = time.perf_counter()
            removed = ctx.map_crop_box(lo, hi)
            t_crop.append(1e3 * (time.perf_counter() - t0))
            kept_n = n0 - removed
        n_manual = 0 if crops_only else (n_rep if mp.shape[0] <= 2000000 else 5)
        for r in range(n_manual):
            ctx.map_clear(); ctx.map_add(mp)
            t0 = time.perf_counter()
            pts = ctx.map_points()
            kept = np.ascontiguousarray(pts[inside(pts, lo, hi)])
            ctx.map_clear()
            ctx.map_add(kept)
            t_manual.append(1e3 * (time.perf_counter() - t0))
            assert ctx.map_size() == kept_n, (ctx.map_size(), kept_n)
        ctx.close()
        out[name] = dict(map_points=int(n0), kept=int(kept_n), crop_ms_median=med(t_crop), crop_ms_min=min(t_crop), crop_reps=len(t_crop),
                         manual_ms_median=med(t_manual), manual_reps=len(t_manual))
        print(name, out[name], flush=True)
    return out


def step(steps=20):
    mp = synth.box_world_map(HBM["map_points"], HBM["box"], 1)
    scan = synth.velodyne_scan(HBM["rings"], HBM["azimuths"], HBM["box"], 2)
    st, w, a = synth.stationary_imu(0.0, 0.35)
    loc = api.Localizer(api.default_cfg(gpu_device=0, num_threads=16, **CAPS))
    loc.set_flags(add_to_map=False, download_clouds=False, keep_log=False)
    loc.map_add(mp)
    i = 0
    while i < len(st) and st[i] <= 0.105:
        loc.update_imu(st[i], w[i], a[i]); i += 1
    rc1 = loc.update_pointcloud(scan, 0.0)
    while i < len(st) and st[i] <= 0.205:
        loc.update_imu(st[i], w[i], a[i]); i += 1
    x_prior, P_prior = loc.get_x(), loc.get_P()
    rc2 = loc.update_pointcloud(scan, 0.1)
    assert rc1 == 1 and rc2 == 0, (rc1, rc2)
    reg = loc.register_resident_call(x_prior, P_prior)

    def ms_per_step():
        for _ in range(3):
            assert reg() == 0
        t0 = time.perf_counter()
        for _ in range(steps):
            reg()
        return 1e3 * (time.perf_counter() - t0) / steps

    out = dict(before=dict(ms_per_step=ms_per_step(), map_points=loc.map_size(), index_bytes=loc.hip.map_index_bytes()))
    c = np.float32(loc.get_x()[0:3])
    half = np.float32([100.0, 100.0, 50.0])
    t0 = time.perf_counter()
    removed = loc.hip.map_crop_box(c - half, c + half)
    out["crop_ms"] = 1e3 * (time.perf_counter() - t0)
    out["removed"] = removed
    out["after"] = dict(ms_per_step=ms_per_step(), map_points=loc.map_size(), index_bytes=loc.hip.map_index_bytes())
    loc.close()
    print("step", out, flush=True)
    return out


def corridor(n_scans=300, n_pts=20000, speed=10.0):
    out = {}
    half, recentre = np.float32([37.0, 37.0, 37.0]), 5.0               # sensor range 30 m + MAX_DIST_PLANE 2 m + recentre_dist
    st, w, a = synth.stationary_imu(0.0, 0.1 * n_scans + 0.06)
    for name in ("policy_on", "policy_off"):
        loc = api.Localizer(api.default_cfg(**CAPS))
        loc.set_flags(add_to_map=True, download_clouds=False, keep_log=False)
        if name == "policy_on":
            loc.set_local_map(half, recentre)
        x0 = loc.get_x(); x0[14] = speed; loc.set_x(x0)
        i, ms = 0, []
        for k in range(n_scans):
            until = 0.1 * (k + 1) + 0.005
            j = i
            while j < len(st) and st[j] <= until:
                j += 1
            if j > i:
                loc.update_imu_n(st[i:j], w[i:j], a[i:j]); i = j
            scan = synth.corridor_scan(k, n_pts, 77, speed=speed)
            t0 = time.perf_counter()
            rc = loc.update_pointcloud(scan, 0.1 * k)
            loc.sync()                                                 # the insert (and the crop behind it) belong to the sweep's cost
            ms.append(1e3 * (time.perf_counter() - t0))
            assert rc == (1 if k == 0 else 0), (k, rc)
        out[name] = dict(sweeps=n_scans, points_per_sweep=n_pts, map_points=loc.map_size(), index_bytes=loc.hip.map_index_bytes(),
                         ms_per_sweep_last_50=med(ms[-50:]), ms_per_sweep_first_50=med(ms[5:55]), crops=loc.hip.map_crop_stats(),
                         final_x=float(loc.get_x()[0]))
        loc.close()
        print("corridor", name, out[name], flush=True)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
    what = [a for a in args if a in ("crops", "step", "corridor")] or ["crops", "step", "corridor"]
    res = {}
    if "crops" in what:
        res["crops"] = crops(reps, "--crops-only" in args)
    if "step" in what:
        res["step"] = step()
    if "corridor" in what:
        res["corridor"] = corridor()
    if "--json" in args:
        with open(args[args.index("--json") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
