"""Point-to-plane normal equations of the resident scan per pose hypothesis (flimo_scan_linearize) and the host loop over them
(api.scan_align), as far as they can be checked without a GPU: the entry points are exported and declared, a NULL context is
rejected by both libraries, the mirror header carries Mapper::linearize, the Jacobian of flimo_c.h is the derivative of the
residual, api.scan_align's update lands where a hand-made system says, and the premise of the GPU convergence test holds for the
numpy yardstick itself.  The call runs on the GPU: tests/test_gpu_scan_linearize.py."""
import os
import subprocess
import tempfile

import numpy as np

import scan_fitness_common as sf
import scan_linearize_common as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_linearize_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    for name in ("flimo_scan_linearize", "flimo_set_linearize_chunk"):
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS, name
    hdr = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    assert "flimo_scan_linearize(" in hdr and "flimo_map_normals(q = w(j, i)" in hdr and "H xi = -g" in hdr
    assert "flimo_set_linearize_chunk(" in open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    H = api.load_host()
    assert hasattr(H, "flimo_loc_scan_linearize") and "flimo_loc_scan_linearize" in api.HOST_SYMBOLS
    assert "flimo_loc_scan_linearize(" in open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for cls, names in ((_lib.HipCtx, ("scan_linearize", "set_linearize_chunk")), (api.Localizer, ("scan_linearize",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert callable(api.scan_align) and callable(api.pose_retract) and callable(api.sym6)
    # the equality of the headers and the symbol lists (tests/test_host_logic.py) holds with the new names in
    import test_host_logic
    test_host_logic.test_c_abi_exports_every_declared_symbol(True)


def test_scan_linearize_rejects_a_null_context(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    x = sf.standard_poses()[:2].copy()
    out = dict(valid=np.full(2, 7, np.int32), H=np.full((2, 21), 7.0), g=np.full((2, 6), 7.0), cost=np.full(2, 7.0), rows=np.full((2, 4, 7), 7.0),
               cnt=np.full((2, 4), 7, np.int32))
    args = (x.ctypes.data, 2, 5, 1.0, 3, 0.05) + tuple(out[k].ctypes.data for k in ("valid", "H", "g", "cost", "rows", "cnt"))
    assert L.flimo_scan_linearize(None, *args) == -2      # FLIMO_ERR_INVALID
    assert L.flimo_set_linearize_chunk(None, 128) == -2
    assert api.load_host().flimo_loc_scan_linearize(None, *args) == -2
    for a in out.values():
        assert np.all(a == 7)


def test_mirror_header_declares_linearize():
    """The mirror's Mapper carries linearize in both forms (compile-only)."""
    tu = """#include "fast_limo/Modules/Mapper.hpp"
int f(fast_limo::Mapper& map, const double* x26) {
  std::vector<int32_t> valid, pair_cnt;
  std::vector<double> H, g, cost, rows;
  int rc = map.linearize(x26, 64, 5, 1.0f, 3, 0.05f, valid, H, g, cost);
  rc += map.linearize(x26, 64, 20, INFINITY, 5, INFINITY, valid, H, g, cost, &rows, &pair_cnt);
  return rc;
}
"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "linearize.cpp")
        open(src, "w").write(tu)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-include", "cmath", "-I", os.path.join(ROOT, "fast_limo_amd", "csrc", "host"),
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def _map_points(oracle):
    oc = oracle.Octree()
    for b in sf.standard_batches():
        oc.update(b)
    mp = oc.points()
    assert 0 < mp.shape[0] == oc.size() <= sf.N_MAP
    return mp


def test_the_jacobian_is_the_derivative_of_the_residual(oracle):
    """Central finite differences in float64 with the plane held fixed: for 50 valid pairs of the standard scene each of the six
    components of xi is perturbed by +-1e-6 (t <- t + R drho, R <- R Exp(dphi)) and (d+ - d-) / 2e-6 is held to J within
    1e-8 * (1 + |p|): the second-order term is about |p| * 1e-12 / 1e-6, the rest is rounding."""
    from fast_limo_amd import api
    mp, scan = _map_points(oracle), sf.standard_scan()
    x = sf.displaced(dx=0.2, dy=-0.1, dyaw_deg=2.0)
    w = sf.world_points(x, scan)
    pl = sl.planes_ref(w, mp, 5, 1.0)
    rows, valid = sl.terms(x, scan, w, pl["cnt"], pl["centroid"], pl["evals"], pl["normal"], 3, 0.05)
    pick = np.nonzero(valid)[0][:: max(1, int(valid.sum()) // 50)][:50]
    assert pick.size == 50
    # the residual at a perturbed pose, all in float64 from the float32 matrix the rows were formed with
    M = sf.pose_rt(x).astype(np.float64)
    R, t = M[:, :3], M[:, 3]
    p = scan[pick].astype(np.float64)
    nr, c = pl["normal"][pick], pl["centroid"][pick]

    def resid(xi):
        xi = np.asarray(xi, np.float64)
        th = np.linalg.norm(xi[3:])
        K = np.array([[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]])
        E = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * K @ K
        wv = p @ (R @ E).T + (t + R @ xi[:3])
        return np.einsum("ij,ij->i", nr, wv - c)
    worst = 0.0
    for a in range(6):
        e = np.zeros(6)
        e[a] = 1e-6
        fd = (resid(e) - resid(-e)) / 2e-6
        err = np.abs(fd - rows[pick, a])
        bound = 1e-8 * (1.0 + np.linalg.norm(p, axis=1))
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), f"component {a}: off by {err.max()!r}"
    print(f"finite differences against J: worst {worst:.3g} of the bound")
    # ... and the update of scan_align moves the pose by exactly that perturbation
    xi = np.array([1e-3, -2e-3, 3e-3, 1e-3, 2e-3, -1e-3])
    y = api.pose_retract(x, xi)
    assert np.array_equal(y[7:], x[7:]) and abs(np.linalg.norm(y[3:7]) - 1.0) < 1e-15
    K = np.array([[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]])
    th = np.linalg.norm(xi[3:])
    E = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * K @ K
    Rx = sl.quat_R(x[3:7])
    assert np.abs(sl.quat_R(y[3:7]) - Rx @ E).max() < 1e-14 and np.abs(y[:3] - (x[:3] + Rx @ xi[:3])).max() < 1e-15


def test_scan_align_on_a_hand_made_system():
    """Points on three orthogonal planes with analytic normals, injected through scan_align's `linearize` argument: the problem is
    linear in the translation and quadratic in the rotation, so ONE Gauss-Newton step from a 1e-3 displacement lands within 1e-6
    (what the step leaves is the second-order term, about |dphi|^2 * |p| / 2 < 1e-6 for points within 1.8 m of the origin)."""
    from fast_limo_amd import api
    rs = np.random.RandomState(3)
    body = []
    for axis in range(3):
        q = rs.uniform(-1, 1, (40, 3))
        q[:, axis] = 0.5 + 0.25 * axis      # the plane x_axis = 0.5 + axis / 4 in the world, the true pose being the identity
        body.append(q)
    body = np.concatenate(body)
    nrm = np.repeat(np.eye(3), 40, axis=0)
    offs = np.repeat([0.5, 0.75, 1.0], 40)

    def linearize(x26s):
        out = dict(valid=[], H=[], g=[], cost=[])
        for x in np.asarray(x26s).reshape(-1, 26):
            R = sl.quat_R(x[3:7])
            w = body @ R.T + x[:3]
            d = np.einsum("ij,ij->i", nrm, w) - offs
            a = nrm @ R
            J = np.concatenate([a, np.cross(body, a)], axis=1)
            Hm = J.T @ J
            out["valid"].append(len(d))
            out["H"].append([Hm[i, j] for i, j in sl.PAIRS21])
            out["g"].append(J.T @ d)
            out["cost"].append(float(d @ d))
        return {k: np.array(v) for k, v in out.items()}
    ident = np.zeros(26)
    ident[6] = 1.0
    ident[7:] = np.arange(19)      # (copied through)
    xi0 = 1e-3 * np.array([0.5, -0.4, 0.3, 0.4, -0.5, 0.6]) / np.linalg.norm([0.5, -0.4, 0.3, 0.4, -0.5, 0.6])
    start = np.stack([api.pose_retract(ident, xi0), api.pose_retract(ident, -xi0)])
    res = api.scan_align(None, start, iters=1, linearize=linearize)
    assert list(res["iters"]) == [1, 1] and list(res["status"]) == [api.ALIGN_RUNNING] * 2 and list(res["valid"]) == [120, 120]
    for x in res["x26"]:
        assert np.abs(x[:3]).max() <= 1e-6 and np.abs(sl.quat_R(x[3:7]) - np.eye(3)).max() <= 1e-6, x[:7]
        assert np.array_equal(x[7:], ident[7:])
    # a pose with too few pairs, and one whose H is singular, stop where they are and are flagged
    few = api.scan_align(None, start, iters=3, min_valid=121, linearize=linearize)
    assert list(few["status"]) == [api.ALIGN_FEW] * 2 and list(few["iters"]) == [0, 0] and np.array_equal(few["x26"], start)

    def singular(x26s):
        out = linearize(x26s)
        for j, x in enumerate(np.asarray(x26s).reshape(-1, 26)):      # (only the poses still running are passed)
            if np.array_equal(x, start[1]):
                out["H"][j] = 0.0
        return out
    sing = api.scan_align(None, start, iters=2, linearize=singular)
    assert list(sing["status"]) == [api.ALIGN_RUNNING, api.ALIGN_SINGULAR] and list(sing["iters"]) == [2, 0]
    assert np.array_equal(sing["x26"][1], start[1])


def test_the_yardstick_converges_from_the_four_starts(oracle):
    """The premise of the GPU convergence test, for the yardstick alone: api.scan_align's own update code, fed by the numpy yardstick
    over the oracle octree's points, k = 5, gate 1 m, max_curv 0.05, 12 iterations.  The bars are conditions, ten times what a
    float64 prototype measured (1.4 mm, 0.011 deg, 1 016 valid pairs)."""
    from fast_limo_amd import api
    mp, scan = _map_points(oracle), sf.standard_scan()
    start = sl.start_poses(sl.HOST_STARTS)
    lin = lambda xs: sl.linearize_ref(xs, scan, mp, 5, 1.0, 3, 0.05)
    res = api.scan_align(None, start, iters=12, linearize=lin)
    end = lin(res["x26"])
    for j, s in enumerate(sl.HOST_STARTS):
        dp, dr = sl.pose_error(res["x26"][j])
        print(f"start {s}: {dp * 1e3:.2f} mm, {dr:.4f} deg, valid {end['valid'][j]}, cost {end['cost'][j]:.3f}, iterations {res['iters'][j]}")
    for j in range(len(sl.HOST_STARTS)):
        dp, dr = sl.pose_error(res["x26"][j])
        assert res["status"][j] == api.ALIGN_RUNNING and res["iters"][j] == 12
        assert dp <= sl.POS_BAR and dr <= sl.ROT_BAR_DEG and end["valid"][j] >= 900
