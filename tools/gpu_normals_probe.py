"""Developer probe (GPU box): what flimo_map_normals costs and what it replaces (profiles/normals/README.md).

A 1M-point map as bench.py builds it, k = 20, no gate:
  (a) 65 536 queries near the surfaces.  The fused call -- normals only, and with all float64 outputs -- against what it replaces,
      in the same process, the candidates taking turns within every repeat: flimo_knn_k with xyz alone (the parent's call:
      20 B per neighbour come back), and that plus the covariance and eigh in numpy on the host.  flimo_knn_k without xyz is
      timed too (the search and its 8 B per neighbour: profiles/knn_k/README.md).
      Condition: normals only takes no longer than flimo_knn_k with xyz, the spread (max - min) of the latter as margin.
  (b) flimo_map_normals_range over the whole map: normals only, and with all float64 outputs.
Milliseconds per call of the C entry: host clock around the call, which ends in a stream wait; arrays sized beforehand; warm-up,
then --reps repeats: median, min, max.
  --trace   a short run (a few calls per case, nothing else) for
            `rocprofv3 --kernel-trace --stats -- python tools/gpu_normals_probe.py --trace`

usage: python tools/gpu_normals_probe.py [--reps N] [--range-reps N] [--trace] [--json FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fast_limo_amd import _lib, synth

N_MAP, BOX, NQ, K = 1000000, 100.0, 65536, 20
INF = float("inf")


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


def host_normals(q, xyz):
    """What a caller of flimo_knn_k does with the coordinates: covariance about the mean (divided by n) and eigh, batched numpy."""
    r = xyz.astype(np.float64) - q.astype(np.float64)[:, None, :]
    d = r - r.mean(1, keepdims=True)
    C = np.einsum("nka,nkb->nab", d, d) / xyz.shape[1]
    w, v = np.linalg.eigh(C)
    return v[:, :, 0], w[:, 0] / w.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--range-reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    reps, range_reps, warm = (3, 2, 1) if a.trace else (a.reps, a.range_reps, 2)

    mp = synth.box_world_map(N_MAP, BOX, 1)
    ctx = _lib.HipCtx(0)
    ctx.map_config()
    ctx.map_add(mp)
    n_map = ctx.map_size()
    rs = np.random.RandomState(7)
    q = np.ascontiguousarray((mp[rs.choice(N_MAP, NQ)] + rs.normal(0, 0.3, (NQ, 3))).astype(np.float32))
    L, h = ctx._L, ctx._h
    idx, sqd, cnt, xyz = np.empty((NQ, K), np.int32), np.empty((NQ, K), np.float32), np.empty(NQ, np.int32), np.empty((NQ, K, 3), np.float32)
    nrm, ncnt = np.empty((NQ, 4), np.float32), np.empty(NQ, np.int32)
    cen, cov, eig = np.empty((NQ, 3)), np.empty((NQ, 6)), np.empty((NQ, 6))

    def knn_k(with_xyz):
        assert L.flimo_knn_k(h, q.ctypes.data, NQ, K, INF, idx.ctypes.data, sqd.ctypes.data, xyz.ctypes.data if with_xyz else None, cnt.ctypes.data) == 0

    def normals(full):
        assert L.flimo_map_normals(h, q.ctypes.data, NQ, K, INF, 3, None, nrm.ctypes.data, ncnt.ctypes.data, cen.ctypes.data if full else None,
                                   cov.ctypes.data if full else None, eig.ctypes.data if full else None) == 0

    cases = {"knn_k_idx_sqd": lambda: knn_k(False), "knn_k_xyz": lambda: knn_k(True), "knn_k_xyz_plus_numpy": lambda: (knn_k(True), host_normals(q, xyz)),
             "normals_only": lambda: normals(False), "normals_all_outputs": lambda: normals(True)}
    if a.trace:
        cases.pop("knn_k_xyz_plus_numpy")
    res = dict(map_points=n_map, box=BOX, queries=NQ, k=K, a_ms=taking_turns(cases, reps, warm))
    ref, new = res["a_ms"]["knn_k_xyz"], res["a_ms"]["normals_only"]
    res["a_condition"] = dict(normals_only_median_ms=new["median"], knn_k_xyz_median_ms=ref["median"], margin_ms=ref["max"] - ref["min"],
                              holds=bool(new["median"] <= ref["median"] + (ref["max"] - ref["min"])))
    # the two routes give the same planes (up to sign), where the plane is well determined
    normals(True); knn_k(True)
    hn, hc = host_normals(q, xyz)
    well = (eig[:, 1] - eig[:, 0]) >= 1e-3 * eig[:, 2]
    e = np.minimum(np.abs(eig[:, 3:] - hn).max(1), np.abs(eig[:, 3:] + hn).max(1))
    res["a_agreement"] = dict(well_determined=float(well.mean()), normal_max_abs_diff=float(e[well].max()), curvature_max_abs_diff=float(np.abs(nrm[:, 3] - hc).max()),
                              cnt_equal=bool(np.array_equal(cnt, ncnt)))
    print("(a)", json.dumps(res["a_ms"]), json.dumps(res["a_condition"]), json.dumps(res["a_agreement"]), flush=True)

    rn, rc = np.empty((n_map, 4), np.float32), np.empty(n_map, np.int32)
    rcen, rcov, reig = np.empty((n_map, 3)), np.empty((n_map, 6)), np.empty((n_map, 6))

    def whole(full):
        assert L.flimo_map_normals_range(h, 0, n_map, K, INF, 3, None, rn.ctypes.data, rc.ctypes.data, rcen.ctypes.data if full else None,
                                         rcov.ctypes.data if full else None, reig.ctypes.data if full else None) == 0
    res["b_ms"] = taking_turns({"range_normals_only": lambda: whole(False), "range_all_outputs": lambda: whole(True)}, range_reps, 1)
    res["b_points_per_second_normals_only"] = n_map / (1e-3 * res["b_ms"]["range_normals_only"]["median"])
    print("(b)", json.dumps(res["b_ms"]), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
