"""Developer probe (GPU box): what flimo_sc_match and flimo_scan_context cost (profiles/scan_context/README.md).

Every step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the probe.
  match NQ NE   NQ queries against NE resident entries at 20 x 60, k 4: `launches` is the GPU time of the call's launches (HIP events
                inside the library, flimo_sc_last_ms), `call` the host clock around the whole call with its copies.  Beside it a
                batched torch formulation on the same device -- columns normalised, per roll an einsum of the queries with the
                entries and one of their valid masks, 1 - sum / count, the minimum over the rolls, topk -- timed by HIP events.
                The two routes' best entries are compared and the share that agrees recorded (torch's sums are in another order,
                so near-ties may differ); nothing is asserted.  Floor: 2 * 60 * 60 * 20 flop a pair at 157.3 TF (the f32 vector rate).
  desc N        the descriptor of an N-point scan against its download and tests/sc_common.py's numpy.
Milliseconds: warm-up, then --reps repeats: median, min, max.

usage: python tools/gpu_sc_probe.py [--reps N] [--json FILE]        (the parent)
       python tools/gpu_sc_probe.py --step match NQ NE | desc N     (one step, what the parent starts)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS, SECTORS, K, PEAK_TF = 20, 60, 4, 157.3
STEPS = (("match", 1, 10000, 240), ("match", 1, 100000, 300), ("match", 256, 10000, 300), ("desc", 65536, 0, 180))


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def torch_route(torch, E, q_host):
    """(best entry [nq], its distance, device ms): E [ne, rings, sectors] resident, the queries uploaded."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    q = torch.from_numpy(q_host).to(E.device)
    e0.record()

    def unit(D):
        n = torch.sqrt((D * D).sum(dim=1, keepdim=True))
        return torch.where(n > 0, D / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(D)), (n[:, 0, :] > 0).float()
    uq, vq = unit(q)
    ue, ve = unit(E)
    best = None
    for s in range(SECTORS):
        sums = torch.einsum("qrs,ers->qe", torch.roll(uq, -s, dims=2), ue)
        cnt = torch.einsum("qs,es->qe", torch.roll(vq, -s, dims=1), ve)
        d = torch.where(cnt > 0, 1.0 - sums / cnt.clamp(min=1.0), torch.full_like(sums, float("inf")))
        best = d if best is None else torch.minimum(best, d)
    dist, idx = torch.topk(best, 1, dim=1, largest=False)
    e1.record()
    idx, dist = idx.cpu().numpy()[:, 0], dist.cpu().numpy()[:, 0]
    return idx, dist, e0.elapsed_time(e1)


def step_match(nq, ne, reps):
    sys.path.insert(0, ROOT)
    import numpy as np
    try:
        import torch      # (before the library: one HIP runtime in the process, torch's)
    except ImportError:
        torch = None
    from fast_limo_amd import _lib
    rs = np.random.RandomState(0)
    ent = (rs.rand(ne, RINGS, SECTORS) * 10).astype(np.float32)
    ent[rs.rand(ne, RINGS, SECTORS) < 0.2] = 0
    q = np.roll(ent[rs.randint(0, ne, nq)], 7, axis=2) + (rs.rand(nq, RINGS, SECTORS) * 0.5).astype(np.float32)
    ctx = _lib.HipCtx(0)
    ctx.set_timing(1)
    t0 = time.perf_counter()
    ctx.sc_db_add(ent)
    add_ms = (time.perf_counter() - t0) * 1e3
    use_torch = torch is not None and torch.cuda.is_available()
    E = torch.from_numpy(ent).cuda() if use_torch else None
    got = ctx.sc_match(q, k=K)      # warm-up
    if use_torch:
        t_idx, _, _ = torch_route(torch, E, q)
    launches, call, t_dev = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = ctx.sc_match(q, k=K)
        call.append((time.perf_counter() - t0) * 1e3)
        launches.append(ctx.sc_last_ms())
        if use_torch:
            t_idx, _, ms = torch_route(torch, E, q)
            t_dev.append(ms)
    floor_ms = 2.0 * SECTORS * SECTORS * RINGS * nq * ne / (PEAK_TF * 1e12) * 1e3
    case = dict(step="match", nq=nq, ne=ne, db_add_ms=add_ms, floor_ms=floor_ms, launches_ms=stats(launches), call_ms=stats(call),
                launches_over_floor=stats(launches)["median"] / floor_ms)
    if use_torch:
        case.update(torch_device_ms=stats(t_dev), best_agree=float((t_idx == got["idx"][:, 0]).mean()))
    ctx.close()
    return case


def step_desc(n, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import sc_common as sc
    from fast_limo_amd import _lib
    pts = sc.random_cloud(0, n, reach=60.0)
    c = sc.cfg()
    ctx = _lib.HipCtx(0)
    ctx.scan_set(pts)
    got = ctx.scan_context(**c)
    call, numpy_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = ctx.scan_context(**c)
        call.append((time.perf_counter() - t0) * 1e3)
    for _ in range(2):
        t0 = time.perf_counter()
        want = sc.descriptor(ctx.scan_get(), c)
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    return dict(step="desc", n=n, used=got[1], call_ms=stats(call), download_numpy_ms=stats(numpy_ms),
                equal=bool(got[0].tobytes() == want[0].tobytes() and got[1] == want[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", nargs="+", default=None)
    a = ap.parse_args()
    if a.step:
        case = step_match(int(a.step[1]), int(a.step[2]), a.reps) if a.step[0] == "match" else step_desc(int(a.step[1]), a.reps)
        print("CASE " + json.dumps(case), flush=True)
        return 0
    cases = []
    for kind, x, y, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", kind, str(x)] + ([str(y)] if kind == "match" else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {kind} {x} {y}: ran past {limit} s; the probe ends here", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
        if r.returncode != 0 or not line:
            print(f"step {kind} {x} {y}: exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        print(line[-1][5:], flush=True)
        cases.append(json.loads(line[-1][5:]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(rings=RINGS, sectors=SECTORS, k=K, cases=cases), fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
