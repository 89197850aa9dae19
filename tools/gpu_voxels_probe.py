"""Developer probe (GPU box): what flimo_map_voxels / flimo_map_thin cost and what they replace (profiles/voxels/README.md).

Steps, each a fresh child process under its own time limit (the parent never opens the GPU; the first step that fails, faults or
runs out of time ends the run):
  sizes     a map as bench.py builds it (--points: 1M and 20M stored points), leaf 0.1 / 0.25 / 1.0 m and the degenerate leaf that
            puts the whole map into one voxel (8 around the origin).  Per leaf, milliseconds between two HIP events around the call
            (every call ends in a wait for its stream), warm, median of --reps:
              sort      flimo_map_voxel_mask, KEEP_FIRST, no output: keys, sort, heads, scan, segments, classes, the per-point stage
              device    flimo_map_voxels, KEEP_NEAREST, no output: the same plus both passes of the moments, under the gather plan
                        (0) and the sorted-copy plan (8); moments = device - sort
              voxels    flimo_map_voxels with count, centroid and cov brought to the host (76 B a voxel), gather plan
              thin      flimo_map_thin(KEEP_FIRST, max_pts 1) once on a fresh copy of the map (it changes the map)
              numpy     route (a): flimo_map_points downloads the map, keys as the restatement forms them, np.unique, np.add.at for
                        count and centroid sums (no covariance)
              torch     route (b): the same on the device, torch.unique + index_add_ (float64 sums; its order is not fixed)
  crowded   bench.py's crowded_leg rebuilt here (50 raw sweeps inserted at the true pose into the 1M-point map): kernel time of the
            first and the later passes on the crowded map, then after map_thin(KEEP_FIRST, --max-pts) at --thin-leaf, and the
            difference of the two registrations' first Gauss-Newton steps (translation, rotation)

usage: python tools/gpu_voxels_probe.py [--reps N] [--points N ...] [--json FILE] [--steps sizes crowded]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES = (0.1, 0.25, 1.0, 4096.0)
BOX = 100.0


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def step_sizes(a):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from fast_limo_amd import _lib, synth
    from gpu_scan_fitness_probe import stats
    import voxels_common as vc
    torch.cuda.init()
    dev = torch.device("cuda:0")
    points = a.points[0]
    reps = a.reps if points <= 2000000 else max(a.reps // 3, 3)
    mp = synth.box_world_map(points, BOX, 1)
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(mp)
    n = ctx.map_size()
    runs = []
    for leaf in LEAVES:
        r = dict(map_points=n, leaf=leaf)
        timed = lambda fn, k=reps: stats([event_ms(torch, fn)[0] for _ in range(k)])
        sort_fn = lambda: ctx.map_voxel_mask(want=(), leaf=leaf)
        vox_fn = lambda: ctx.map_voxels(want=("count", "centroid", "cov"), leaf=leaf)
        sort_fn(); sort_fn()
        r["sort_ms"] = timed(sort_fn)
        dev_fn = lambda: ctx.map_voxels(want=(), leaf=leaf, keep=vc.KEEP_NEAREST)      # both passes of the moments, nothing downloaded
        for plan, name in ((0, "device_gather_ms"), (8, "device_sorted_copy_ms")):
            ctx.set_voxel_plan(plan)
            dev_fn(); dev_fn()
            r[name] = timed(dev_fn)
        ctx.set_voxel_plan(0)
        vox_fn(); vox_fn()
        r["voxels_gather_ms"] = timed(vox_fn)                # ... and with count, centroid and cov brought to the host (76 B a voxel)
        out = vox_fn()
        r.update(voxels=out["nv"], largest=out["stats"]["largest"], outside=out["stats"]["outside"])
        r["moments_gather_ms"] = r["device_gather_ms"]["median"] - r["sort_ms"]["median"]
        r["moments_sorted_copy_ms"] = r["device_sorted_copy_ms"]["median"] - r["sort_ms"]["median"]
        # thin once, on a second context holding the same map
        other = _lib.HipCtx(0)
        other.map_config()
        other.map_add(mp)
        ms, (removed, st) = event_ms(torch, lambda: other.map_thin(leaf=leaf, keep=vc.KEEP_FIRST, max_pts=1))
        r.update(thin_ms=ms, thin_removed=removed, thin_left=other.map_size())
        other.close()
        if not a.only_device:
            # (a) download + numpy
            t0 = time.perf_counter()
            pts = ctx.map_points()
            t1 = time.perf_counter()
            _, key, inside = vc.keys(pts, leaf)
            uniq, inv, cnt = np.unique(key[inside], return_inverse=True, return_counts=True)
            sums = np.zeros((len(uniq), 3))
            np.add.at(sums, inv, pts[inside].astype(np.float64))
            cen = sums / cnt[:, None]
            t2 = time.perf_counter()
            r["numpy_ms"] = dict(download=1e3 * (t1 - t0), unique_add_at=1e3 * (t2 - t1), total=1e3 * (t2 - t0))
            r["numpy_counts_equal"] = bool(len(uniq) == out["nv"] and np.array_equal(cnt, out["count"]))
            r["numpy_centroid_max_diff"] = float(np.abs(cen - out["centroid"]).max()) if len(uniq) == out["nv"] else None
            # (b) torch on the same device
            P = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
            inv32 = float(np.float32(1.0) / np.float32(leaf))

            def torch_route():
                c = torch.floor(P * inv32).to(torch.int64) + (1 << 20)
                k = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
                u, iv, ct = torch.unique(k, return_inverse=True, return_counts=True)
                s = torch.zeros((u.shape[0], 3), dtype=torch.float64, device=dev).index_add_(0, iv, P.double())
                return ct.cpu().numpy(), (s / ct[:, None]).cpu().numpy()

            torch_route(); torch_route()
            r["torch_ms"] = timed(torch_route, max(reps // 2, 3))
            tc, tcen = torch_route()
            r["torch_counts_equal"] = bool(len(tc) == out["nv"] and np.array_equal(tc, out["count"]))
            r["torch_centroid_max_diff"] = float(np.abs(tcen - out["centroid"]).max()) if len(tc) == out["nv"] else None
            r["numpy_over_device"] = r["numpy_ms"]["total"] / r["voxels_gather_ms"]["median"]
            r["torch_over_device"] = r["torch_ms"]["median"] / r["voxels_gather_ms"]["median"]
            del P
        runs.append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    return dict(step="sizes", points=points, runs=runs)


def step_crowded(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    from fast_limo_amd import _lib, synth
    rings, az, nmap, n_sweeps = 64, 1024, 1000000, 50      # bench.py's defaults and crowded_leg's sweeps
    mp = synth.box_world_map(nmap, BOX, 1)
    x = np.zeros(26); x[6] = 1; x[10] = 1; x[25] = -9.809
    x[0:3] = synth.T_STAR_T
    r, p_, y = [np.deg2rad(v) for v in synth.T_STAR_RPY_DEG]
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p_ / 2), np.sin(p_ / 2), np.cos(y / 2), np.sin(y / 2)
    x[3:7] = [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]
    query = np.ascontiguousarray(synth.velodyne_scan(rings, az, BOX, 999)[:, :3])
    cfg = _lib.default_match_cfg(MAX_NUM_PC2MATCH=10**7, MAX_NUM_MATCHES=10**7)
    ctx = _lib.HipCtx(0)
    ctx.map_config(); ctx.map_add(mp)

    def passes():
        ctx.set_timing(1)
        rows, step = [], None
        for rep in range(6):
            ctx.scan_set(query)
            row = []
            for k in range(3):
                HTH, HTh, M = ctx.match_reduce(x, cfg)
                if k == 0:
                    step = (-np.linalg.solve(HTH[:6, :6], HTh[:6]), M)      # the first Gauss-Newton step of the registration
                aa, w, f = ctx.last_kernel_ms()
                row.append((aa + w + f) * 1e3)
            rows.append(row)
        ctx.set_timing(0)
        m = np.median(np.array(rows[1:]), axis=0)
        return dict(first_pass=float(m[0]), later_passes=float(0.5 * (m[1] + m[2]))), step

    clean, _ = passes()
    for j in range(n_sweeps):
        ctx.scan_set(np.ascontiguousarray(synth.velodyne_scan(rings, az, BOX, 100 + j)[:, :3]))
        ctx.map_add_scan(x, 0.0)
    crowded, (s0, m0) = passes()
    n_crowded = ctx.map_size()
    before = ctx.map_voxels(want=(), leaf=a.thin_leaf)["stats"]
    t0 = time.perf_counter()
    removed, st = ctx.map_thin(leaf=a.thin_leaf, keep=0, max_pts=a.max_pts)
    thin_ms = 1e3 * (time.perf_counter() - t0)
    thinned, (s1, m1) = passes()
    return dict(step="crowded", thin_leaf=a.thin_leaf, max_pts=a.max_pts, map_points_crowded=n_crowded, map_points_thinned=ctx.map_size(),
                removed=removed, voxels=before["voxels"], largest_before=before["largest"], thin_wall_ms=thin_ms,
                clean_map_us=clean, crowded_map_us=crowded, thinned_map_us=thinned,
                crowded_over_clean=dict(first_pass=crowded["first_pass"] / clean["first_pass"], later_passes=crowded["later_passes"] / clean["later_passes"]),
                thinned_over_clean=dict(first_pass=thinned["first_pass"] / clean["first_pass"], later_passes=thinned["later_passes"] / clean["later_passes"]),
                matches=dict(crowded=int(m0), thinned=int(m1)),
                first_step_difference=dict(translation_m=float(np.linalg.norm(s1[0:3] - s0[0:3])), rotation_rad=float(np.linalg.norm(s1[3:6] - s0[3:6])),
                                           crowded_step=s0.tolist(), thinned_step=s1.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 20000000])
    ap.add_argument("--steps", nargs="+", default=["sizes", "crowded"])
    ap.add_argument("--thin-leaf", type=float, default=0.25)
    ap.add_argument("--max-pts", type=int, default=4)
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        res = step_sizes(a) if a.child == "sizes" else step_crowded(a)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    # the parent: every step a child of its own under a time limit; nothing more is started after a step that did not end well
    plan = [("sizes", ["--points", str(p)]) for p in a.points if "sizes" in a.steps] + ([("crowded", [])] if "crowded" in a.steps else [])
    results = []
    for name, extra in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--thin-leaf", str(a.thin_leaf),
               "--max-pts", str(a.max_pts)] + extra + (["--only-device"] if a.only_device else [])
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s %s ran out of its %d s: stopping" % (name, extra, a.step_timeout), flush=True)
            break
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print("step %s %s ended with status %d: stopping" % (name, extra, p.returncode), flush=True)
            break
        results += [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as fh:
                json.dump(dict(lib=os.environ.get("FLIMO_HIP_LIB", "libflimo_hip.so"), results=results), fh, indent=1)
    return 0 if len(results) == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
