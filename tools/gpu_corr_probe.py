"""Developer probe (GPU box): what flimo_corr_poses costs and what it replaces (profiles/corr_poses/README.md).

8 192 putative correspondences of a 100 m box scene (30 % true, their mates displaced by N(0, 0.01) m; the rest random points of the
box), 2^17 samples of api.corr_triplets, min_edge 0.5 m, max_dist 0.15 m; with pre-rejection (edge_sim 0.9) and without (0).  In the
same process, the candidates taking turns within every repeat:
  call         flimo_corr_poses, status + inliers + sum_sqd + pose come back
  torch        a batched torch formulation on the device: TRIAD in float64 for all samples, then per chunk of survivors the
               float32 transform of all pairs, the gate, count and sum (clouds resident; triplets uploaded, four arrays downloaded)
  host         the route without a GPU: flimo_corr_pose_host per triplet, numpy over the pairs per surviving hypothesis -- timed
               on the first --host-nh samples only (default 2048) and scaled to 2^17
Milliseconds per batch: host clock around the calls, each of which ends in a stream wait; warm-up, then --reps repeats: median, min,
max.  The routes are compared and the comparison is recorded, nothing is asserted: whether the statuses are equal, the largest
difference of an inlier count (the torch and numpy routes form the world point in another association, so a pair whose float32
distance sits at the gate may fall on the other side) and the largest difference of a sum (which moves by up to max_dist^2 = 0.0225
with every such pair).

usage: python tools/gpu_corr_probe.py [--reps N] [--host-nh N] [--no-torch] [--json FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
try:
    import torch      # (before the library: one HIP runtime in the process, torch's)
except ImportError:
    torch = None
from fast_limo_amd import _lib, api, synth
from gpu_scan_fitness_probe import taking_turns

M, NH, BOX, MIN_EDGE, GATE = 8192, 1 << 17, 100.0, 0.5, 0.15


def scene(seed=0):
    rs = np.random.RandomState(seed)
    src = np.ascontiguousarray(synth.box_world_scan_random(M, BOX, 2)[:, :3], dtype=np.float32)
    R = synth.rpy_to_R(*np.radians(synth.T_STAR_RPY_DEG))
    true = rs.rand(M) < 0.3
    world = src.astype(np.float64) @ R.T + np.asarray(synth.T_STAR_T) + rs.randn(M, 3) * 0.01
    wrong = (rs.rand(M, 3) - 0.5) * BOX
    return src, np.ascontiguousarray(np.where(true[:, None], world, wrong), dtype=np.float32), true


def torch_route(src, dst, tri_host, edge_sim, chunk=2048):
    """status, inliers, sum_sqd, pose of all samples by batched tensor arithmetic (no bit-for-bit claim)."""
    dev = src.device
    tri = torch.from_numpy(tri_host.astype(np.int64)).to(dev)
    S, D = src[tri].double(), dst[tri].double()      # [nh, 3, 3]
    edges = lambda P: torch.stack([((P[:, 1] - P[:, 0]) ** 2).sum(1), ((P[:, 2] - P[:, 1]) ** 2).sum(1), ((P[:, 0] - P[:, 2]) ** 2).sum(1)], 1)
    es, ed = edges(S), edges(D)
    degenerate = ~((es >= MIN_EDGE ** 2).all(1) & (ed >= MIN_EDGE ** 2).all(1))
    rejected = ~(torch.minimum(es, ed) >= edge_sim ** 2 * torch.maximum(es, ed)).all(1)

    def frame(P):
        u1 = torch.nn.functional.normalize(P[:, 1] - P[:, 0], dim=1)
        u3 = torch.nn.functional.normalize(torch.linalg.cross(u1, P[:, 2] - P[:, 0]), dim=1)
        return torch.stack([u1, torch.linalg.cross(u3, u1), u3], 2)      # columns
    Rm = frame(D) @ frame(S).transpose(1, 2)
    t = D.mean(1) - (Rm @ S.mean(1)[:, :, None])[:, :, 0]
    status = torch.where(degenerate, 1, torch.where(rejected, 2, 0)).int()
    ok = torch.nonzero(status == 0)[:, 0]
    inliers = torch.zeros(tri.shape[0], dtype=torch.int32, device=dev)
    sums = torch.zeros(tri.shape[0], dtype=torch.float64, device=dev)
    Rf, tf = Rm.float(), t.float()
    for a in range(0, ok.numel(), chunk):
        j = ok[a:a + chunk]
        w = torch.einsum("jrc,ic->jir", Rf[j], src) + tf[j][:, None, :]      # [chunk, m, 3]
        d2 = ((w - dst[None]) ** 2).sum(2)
        inl = d2 < GATE * GATE
        inliers[j] = inl.sum(1).int()
        sums[j] = torch.where(inl, d2, torch.zeros_like(d2)).double().sum(1)
    return status.cpu().numpy(), inliers.cpu().numpy(), sums.cpu().numpy(), Rm.cpu().numpy(), t.cpu().numpy()


def host_route(src, dst, tri, edge_sim):
    """flimo_corr_pose_host per triplet, numpy over the pairs per survivor."""
    status, inliers = np.zeros(len(tri), np.int32), np.zeros(len(tri), np.int32)
    sums = np.zeros(len(tri))
    gate2 = np.float32(GATE) * np.float32(GATE)
    for j, abc in enumerate(tri):
        st, _, rt = api.corr_pose_host(src[abc], dst[abc], edge_sim=edge_sim, min_edge=MIN_EDGE, max_dist=GATE)
        status[j] = st
        if st == 0:
            d = (src @ rt[:, :3].T + rt[:, 3]) - dst
            d2 = (d * d).sum(1)
            inl = d2 < gate2
            inliers[j], sums[j] = inl.sum(), d2[inl].astype(np.float64).sum()
    return status, inliers, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-nh", type=int, default=2048)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    src, dst, true = scene()
    tri = api.corr_triplets(M, NH, 0)
    with_torch = torch is not None and not a.no_torch and torch.cuda.is_available()
    if with_torch:
        t_src, t_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    ctx = _lib.HipCtx(0)
    L, h = ctx._L, ctx._h
    status, inl, s, pose = np.empty(NH, np.int32), np.empty(NH, np.int32), np.empty(NH), np.empty((NH, 7))
    res = dict(pairs=M, true_pairs=int(true.sum()), samples=NH, min_edge=MIN_EDGE, max_dist=GATE, host_nh=a.host_nh, cases={})
    for edge_sim in (0.9, 0.0):
        k = _lib.corr_cfg(edge_sim, MIN_EDGE, GATE)

        def call():
            assert L.flimo_corr_poses(h, src.ctypes.data, dst.ctypes.data, M, tri.ctypes.data, NH, _lib.C.byref(k), status.ctypes.data,
                                      inl.ctypes.data, s.ctypes.data, pose.ctypes.data, None) == 0
        cases = {"call": call}
        if with_torch:
            def by_torch():
                torch_route(t_src, t_dst, tri, edge_sim)
                torch.cuda.synchronize()
            cases["torch"] = by_torch
        out = dict(ms=taking_turns(cases, a.reps, 2))
        call()
        ok = status == 0
        out["survivors"] = int(ok.sum())
        out["rejected"] = int((status == 2).sum())
        out["degenerate"] = int((status == 1).sum())
        out["best_inliers"] = int(inl.max())
        out["pairs_evaluated_per_second"] = float(ok.sum()) * M / (1e-3 * out["ms"]["call"]["median"])
        if with_torch:
            t_status, t_inl, t_sum, _, _ = torch_route(t_src, t_dst, tri, edge_sim)
            out["torch_agreement"] = dict(status_equal=bool(np.array_equal(t_status, status)),
                                          inliers_max_abs_diff=int(np.abs(t_inl.astype(np.int64) - inl).max()),
                                          sum_max_abs_diff=float(np.abs(t_sum - s).max()))
        t0 = time.perf_counter()
        h_status, h_inl, h_sum = host_route(src, dst, tri[:a.host_nh], edge_sim)
        dt = 1e3 * (time.perf_counter() - t0)
        out["host"] = dict(ms_measured=dt, samples_measured=a.host_nh, ms_scaled_to_all=dt * NH / a.host_nh,
                           status_equal=bool(np.array_equal(h_status, status[:a.host_nh])),
                           inliers_max_abs_diff=int(np.abs(h_inl.astype(np.int64) - inl[:a.host_nh]).max()))
        res["cases"][f"edge_sim_{edge_sim}"] = out
    print(json.dumps(res), flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
