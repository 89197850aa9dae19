"""Developer probe (GPU box): what flimo_desc_match costs and what it replaces (profiles/desc_match/README.md).

dim 33, k 2, 1 000 000 reference rows, 4 096 and 65 536 query rows, all uniform in [0, 100) like FPFH bins.  In the same process,
the two routes taking turns within every repeat:
  call     flimo_desc_match against the resident set: `launches` is the GPU time of its launches (HIP events around them inside the
           library, flimo_desc_last_ms), `call` the host clock around the whole call with its copies
  torch    the route it replaces on the same device: torch.cdist of the queries against reference chunks that fit memory, squared,
           topk(2) per chunk, the chunks' winners merged per query by a second topk (references resident; queries uploaded, idx and
           dist downloaded); HIP events around the device work, host clock around the whole
Floor: 2 * 34 * nq * nr flop at 157.3 TF (the f32 MFMA rate).  Milliseconds: warm-up, then --reps repeats: median, min, max.  The two
routes' nearest indices are compared and the share that agrees is recorded (torch's distances carry another rounding, so near-ties
may order differently); nothing is asserted.

usage: python tools/gpu_desc_match_probe.py [--reps N] [--nr N] [--no-torch] [--json FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
try:
    import torch      # (before the library: one HIP runtime in the process, torch's)
except ImportError:
    torch = None
from fast_limo_amd import _lib

DIM, K, PEAK_TF = 33, 2, 157.3


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def torch_route(R, q_host, chunk):
    """(idx [nq, 2], squared dist [nq, 2], device ms) by cdist + topk over reference chunks."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    q = torch.from_numpy(q_host).to(R.device)
    e0.record()
    best_d, best_i = None, None
    for a in range(0, R.shape[0], chunk):
        d = torch.cdist(q, R[a:a + chunk]) ** 2
        dk, ik = torch.topk(d, K, dim=1, largest=False)
        ik = ik + a
        if best_d is None:
            best_d, best_i = dk, ik
        else:
            cd, ci = torch.cat([best_d, dk], 1), torch.cat([best_i, ik], 1)
            best_d, sel = torch.topk(cd, K, dim=1, largest=False)
            best_i = torch.gather(ci, 1, sel)
    e1.record()
    idx, dist = best_i.cpu().numpy(), best_d.cpu().numpy()
    return idx, dist, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nr", type=int, default=1000000)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    ref = (rs.rand(a.nr, DIM) * 100).astype(np.float32)
    ctx = _lib.HipCtx(0)
    ctx.set_timing(1)
    t0 = time.perf_counter()
    ctx.desc_ref_set(ref)
    out = dict(dim=DIM, k=K, nr=a.nr, ref_set_ms=(time.perf_counter() - t0) * 1e3, cases=[])
    use_torch = torch is not None and not a.no_torch and torch.cuda.is_available()
    R = torch.from_numpy(ref).cuda() if use_torch else None
    for nq in (4096, 65536):
        q = (rs.rand(nq, DIM) * 100).astype(np.float32)
        floor_ms = 2.0 * 34 * nq * a.nr / (PEAK_TF * 1e12) * 1e3
        chunk = max(min(a.nr, (1 << 31) // (4 * nq)), 1)      # a distance block of at most 2 GiB
        launches, call, t_dev, t_all = [], [], [], []
        got = ctx.desc_match(q, k=K)      # warm-up
        if use_torch:
            t_idx, _, _ = torch_route(R, q, chunk)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = ctx.desc_match(q, k=K)
            call.append((time.perf_counter() - t0) * 1e3)
            launches.append(ctx.desc_last_ms())
            if use_torch:
                t0 = time.perf_counter()
                t_idx, _, ms = torch_route(R, q, chunk)
                t_all.append((time.perf_counter() - t0) * 1e3)
                t_dev.append(ms)
        case = dict(nq=nq, floor_ms=floor_ms, launches_ms=stats(launches), call_ms=stats(call),
                    launches_over_floor=stats(launches)["median"] / floor_ms)
        if use_torch:
            case.update(torch_chunk=chunk, torch_device_ms=stats(t_dev), torch_whole_ms=stats(t_all),
                        nearest_agree=float((t_idx[:, 0] == got["idx"][:, 0]).mean()))
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
