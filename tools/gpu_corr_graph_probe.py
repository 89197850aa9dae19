"""Developer probe (GPU box): what flimo_corr_graph costs and what it replaces (profiles/corr_graph/README.md).

m putative correspondences of a 100 m box scene (6 % true, their mates displaced by N(0, 0.014) m; the rest random points of the
box), tol 0.06 m, min_edge 0.5 m, for m = 2 048, 8 192 and 32 768:
  call    flimo_corr_graph, degree + core + max_core come back (and once more with the bit matrix)
  numpy   the route without a GPU: the dense float64 predicate in row blocks and plain peeling -- up to --numpy-max pairs (default
          8 192; 32 768 pairs are 10^9 predicates and minutes of numpy)
Milliseconds per call: host clock around the call, which ends in a stream wait; warm-up, then --reps repeats: median, min, max.  The
two routes are compared (every output is an integer: equal or not) and the comparison is recorded, nothing is asserted.

usage: python tools/gpu_corr_graph_probe.py [--reps N] [--numpy-max M] [--json FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fast_limo_amd import _lib, synth

BOX, TOL, MIN_EDGE, KEEP, NOISE = 100.0, 0.06, 0.5, 0.06, 0.014


def scene(m, seed=0):
    rs = np.random.RandomState(seed)
    src = np.ascontiguousarray(synth.box_world_scan_random(m, BOX, 2)[:, :3], dtype=np.float32)
    R = synth.rpy_to_R(*np.radians(synth.T_STAR_RPY_DEG))
    true = rs.rand(m) < KEEP
    world = src.astype(np.float64) @ R.T + np.asarray(synth.T_STAR_T) + rs.randn(m, 3) * NOISE
    wrong = (rs.rand(m, 3) - 0.5) * BOX
    return src, np.ascontiguousarray(np.where(true[:, None], world, wrong), dtype=np.float32), true


def numpy_route(src, dst):
    """degree and core by the dense predicate and plain peeling."""
    s, d = src.astype(np.float64), dst.astype(np.float64)
    m = len(s)
    sq = lambda v: v[..., 0] * v[..., 0] + (v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    min2, tol = float(np.float32(MIN_EDGE)) ** 2, float(np.float32(TOL))
    A = np.zeros((m, m), bool)
    for a in range(0, m, 256):
        es, ed = sq(s[None] - s[a:a + 256, None]), sq(d[None] - d[a:a + 256, None])
        A[a:a + 256] = (es >= min2) & (ed >= min2) & (np.abs(np.sqrt(es) - np.sqrt(ed)) <= tol)
    A[np.arange(m), np.arange(m)] = False
    degree = A.sum(1).astype(np.int64)
    deg, live, core, k = degree.copy(), np.ones(m, bool), np.zeros(m, np.int32), 0
    while live.any():
        while True:
            go = live & (deg <= k)
            if not go.any():
                break
            core[go], live[go] = k, False
            deg -= A[:, go].sum(1)
        k += 1
    return degree.astype(np.int32), core


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy-max", type=int, default=8192)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _lib.HipCtx(0)
    res = dict(tol=TOL, min_edge=MIN_EDGE, keep=KEEP, noise=NOISE, cases={})
    for m in (2048, 8192, 32768):
        src, dst, true = scene(m)
        out = dict(true_pairs=int(true.sum()))
        out["call_ms"] = timed(lambda: ctx.corr_graph(src, dst, tol=TOL, min_edge=MIN_EDGE), a.reps)
        out["call_with_adj_ms"] = timed(lambda: ctx.corr_graph(src, dst, want=("adj",), tol=TOL, min_edge=MIN_EDGE), max(a.reps // 3, 1), 1)
        got = ctx.corr_graph(src, dst, tol=TOL, min_edge=MIN_EDGE)
        keep = got["core"] == got["max_core"]
        out.update(edges=int(got["degree"].astype(np.int64).sum() // 2), max_core=got["max_core"], kept=int(keep.sum()), kept_true=int(true[keep].sum()),
                   predicates_per_second=float(m) * m / (1e-3 * out["call_ms"]["median"]))
        if m <= a.numpy_max:
            t0 = time.perf_counter()
            degree, core = numpy_route(src, dst)
            out["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            out["numpy_agreement"] = dict(degree_equal=bool(np.array_equal(degree, got["degree"])), core_equal=bool(np.array_equal(core, got["core"])))
        res["cases"][f"m_{m}"] = out
        print(m, json.dumps(out), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
