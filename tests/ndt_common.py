"""Shared helpers of the NDT tests (flimo_ndt_build, flimo_scan_ndt): the numpy restatement of include/flimo_c.h.

The model.  A voxel of ``map_voxels`` (key, count, centroid, cov) is a CELL iff count >= min_pts and l2 > 0.0; floor = eig_ratio * l2
(one float64 product), lk' = lk < floor ? floor : lk, wk = 1.0 / lk' (``weights``: exact given the eigenvalues).  The eigen-solve is
held to numpy ``eigh`` of the same cov by the bounds of normals_common (U_EIG: residual, unit norm, eigenvalues); orthogonality
between the vectors is not covered by that derivation and has its own bar (test_gpu_ndt.py measures it).

The terms.  ``lookup`` restates the cell lookup (voxels_common.keys is voxel_key; the neighbour slots -x +x -y +y -z +z; a binary
search of the model's keys), ``terms`` m and x = c * m in the stated association, ``contributions`` the 28 numbers of every
(point, neighbour slot, k) given an e, ``shape_sums`` the two-level shape of the sums in numpy (sums_common), ``shape_sums_plain`` the same
in plain Python floats, ``fsum_sums`` the independent math.fsum value with the sums of absolute values for
scan_linearize_common.sum_bound.

exp.  e is compared with np.exp(x) within EXP_ULPS = 4 spacings: 1 ulp documented for OCML's float64 exp plus 1 ulp for glibc's,
doubled.  The ROCm installation this was written against ships no OCML document that states another figure."""
import math

import numpy as np

import scan_fitness_common as sf
import sums_common
import voxels_common as vc
from sums_common import RED, SEG          # SUM_RED, SUM_SEG of flimo_sums.h

D = np.float64
EXP_ULPS = 4
PAIRS21 = [(a, b) for a in range(6) for b in range(a, 6)]
HALF = vc.HALF


def key_of(ijk):
    c = np.asarray(ijk, np.int64).reshape(-1, 3)
    return ((c[:, 2] + HALF).astype(np.uint64) << np.uint64(42)) | ((c[:, 1] + HALF).astype(np.uint64) << np.uint64(21)) | \
        (c[:, 0] + HALF).astype(np.uint64)


def sym3(c6):
    c6 = np.asarray(c6, D)
    return np.array([[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]])


def weights(evals, eig_ratio):
    l = np.asarray(evals, D).reshape(-1, 3)
    floor = D(eig_ratio) * l[:, 2]
    return 1.0 / np.where(l < floor[:, None], floor[:, None], l)


def cell_rows(vox, min_pts):
    """The rows of a ``map_voxels`` listing (with cov) that are cells, by numpy's own largest eigenvalue."""
    keep = []
    for v in range(vox["count"].shape[0]):
        if vox["count"][v] >= min_pts and np.linalg.eigvalsh(sym3(vox["cov"][v]))[2] > 0.0:
            keep.append(v)
    return np.asarray(keep, np.int64)


def model_numpy(pts, leaf, min_pts, eig_ratio):
    """A whole model without a device: voxels_common.restate's voxels, numpy eigh's axes (row k of evec: the vector of lk)."""
    r = vc.restate(pts, leaf=leaf)
    vox = dict(count=r["count"], cov=r["cov"])
    rows = cell_rows(vox, min_pts)
    ev, vec = np.zeros((len(rows), 3)), np.zeros((len(rows), 3, 3))
    for t, v in enumerate(rows):
        l, V = np.linalg.eigh(sym3(r["cov"][v]))
        ev[t], vec[t] = np.maximum(l, 0.0), V.T
    return dict(ijk=r["ijk"][rows], count=r["count"][rows], mean=r["centroid"][rows], evec=vec, eval=ev, wgt=weights(ev, eig_ratio),
                nc=len(rows), leaf=leaf)


def lookup(w, leaf, model_ijk, hood):
    """cell [n, 7] int32: the row of the model for every neighbour slot of every float32 world point, -1 when absent."""
    w = np.asarray(w, np.float32).reshape(-1, 3)
    n = w.shape[0]
    ijk, _, inside = vc.keys(w, leaf)
    mk = key_of(model_ijk)
    assert np.all(mk[1:] > mk[:-1]), "the model's keys ascend"
    cell = np.full((n, 7), -1, np.int32)
    for s in range(hood):
        c = ijk.astype(np.int64).copy()
        ok = inside.copy()
        if s:
            a = (s - 1) >> 1
            c[:, a] += -1 if (s & 1) else 1
            ok &= np.abs(c[:, a]) < HALF
        k = key_of(np.where(ok[:, None], c, 0))
        at = np.searchsorted(mk, k)
        hit = ok & (at < len(mk))
        hit[hit] = mk[at[hit]] == k[hit]
        cell[hit, s] = at[hit]
    return cell


def terms(w, model, cell, d2):
    """m and x = c * m [n, 7] (NaN where absent) and the residuals d [n, 7, 3], in the association of flimo_c.h.  w: the float32
    world points (widened here, as the call does; a float64 array is taken as it is: the finite-difference test moves w smoothly)."""
    wd = np.asarray(w).astype(D)
    n = wd.shape[0]
    have = cell >= 0
    at = np.where(have, cell, 0)
    mean, v, wg = model["mean"][at], model["evec"][at], model["wgt"][at]          # [n, 7, 3], [n, 7, 3, 3], [n, 7, 3]
    r = wd[:, None, :] - mean
    d = np.stack([v[:, :, k, 0] * r[:, :, 0] + (v[:, :, k, 1] * r[:, :, 1] + v[:, :, k, 2] * r[:, :, 2]) for k in range(3)], axis=2)
    m = wg[:, :, 0] * (d[:, :, 0] * d[:, :, 0]) + (wg[:, :, 1] * (d[:, :, 1] * d[:, :, 1]) + wg[:, :, 2] * (d[:, :, 2] * d[:, :, 2]))
    c = -0.5 * D(d2)
    x = c * m
    nan = np.full((n, 7), np.nan)
    return np.where(have, m, nan), np.where(have, x, nan), d


def contributions(x26, scan, model, cell, d, e, d2):
    """C [n, 7, 3, 28]: the contributions of (point, neighbour slot, k), +0.0 where the term is not live; live [n, 7].  The score's
    e sits at k = 0 (one add per term)."""
    R = sf.pose_rt(x26)[:, :3].astype(D)
    p = np.asarray(scan, np.float32).astype(D)
    n = p.shape[0]
    have = cell >= 0
    with np.errstate(invalid="ignore"):
        live = have & (np.nan_to_num(e, nan=0.0) > 0.0)
    at = np.where(have, cell, 0)
    v, wg = model["evec"][at], model["wgt"][at]
    ee = np.where(live, e, 0.0)
    ed = ee * D(d2)
    C = np.zeros((n, 7, 3, 28))
    px, py, pz = p[:, None, 0], p[:, None, 1], p[:, None, 2]
    for k in range(3):
        nx, ny, nz = v[:, :, k, 0], v[:, :, k, 1], v[:, :, k, 2]
        J = [R[0, t] * nx + (R[1, t] * ny + R[2, t] * nz) for t in range(3)]
        J += [py * J[2] - pz * J[1], pz * J[0] - px * J[2], px * J[1] - py * J[0]]
        s = ed * wg[:, :, k]
        for t, (a, b) in enumerate(PAIRS21):
            C[:, :, k, t] = (s * J[a]) * J[b]
        sd = s * d[:, :, k]
        for a in range(6):
            C[:, :, k, 21 + a] = sd * J[a]
    C[:, :, 0, 27] = ee
    C[~live] = 0.0
    return C, live


def shape_sums(C):
    """The 28 sums of one pose in the shape of the call: C [n, 7, 3, 28] -> [28]."""
    return sums_common.shape_sums(np.asarray(C).reshape(C.shape[0], 21, 28))


def shape_sums_plain(C):
    """shape_sums in plain Python floats."""
    C = np.asarray(C)
    n = C.shape[0]
    total = [0.0] * 28
    for s0 in range(0, n, SEG):
        acc = [[0.0] * 28 for _ in range(RED)]
        for t in range(RED):
            for i in range(s0 + t, min(n, s0 + SEG), RED):
                for s in range(7):
                    for k in range(3):
                        row = C[i, s, k].tolist()
                        a = acc[t]
                        for q in range(28):
                            a[q] = a[q] + row[q]
        part = []
        for wave in range(4):
            lanes = [acc[64 * wave + l][:] for l in range(64)]
            o = 1
            while o < 64:
                lanes = [[lanes[l][q] + lanes[l ^ o][q] for q in range(28)] for l in range(64)]
                o <<= 1
            part.append(lanes[0])
        for q in range(28):
            total[q] = total[q] + ((part[0][q] + part[1][q]) + (part[2][q] + part[3][q]))
    return np.array(total)


def fsum_sums(C):
    """(sums [28] by math.fsum, sums of absolute values [28], the number of added terms)."""
    flat = C.reshape(-1, 28)
    flat = flat[np.any(flat != 0.0, axis=1)]
    return (np.array([math.fsum(flat[:, q]) for q in range(28)]), np.array([math.fsum(np.abs(flat[:, q])) for q in range(28)]),
            max(flat.shape[0], 1))


def restate(x26, scan, model, hood, d2, e=None, exp=np.exp):
    """One pose: dict(cell, m, x, e, C, live, valid, cells).  e: the e to use [n, 7] (the device's); None: exp(x)."""
    w = sf.world_points(x26, scan)
    cell = lookup(w, model["leaf"], model["ijk"], hood)
    m, x, d = terms(w, model, cell, d2)
    if e is None:
        with np.errstate(invalid="ignore", under="ignore"):
            e = exp(x)
    C, live = contributions(x26, scan, model, cell, d, e, d2)
    return dict(cell=cell, m=m, x=x, e=e, C=C, live=live, valid=int(np.any(live, axis=1).sum()), cells=int(live.sum()), w=w)


def gauss_newton(starts, scan, models, hood=7, outlier_ratio=0.55, iters=30, min_valid=30):
    """api.ndt_align with the restatement in place of the device: the end poses [len(starts), 26]."""
    from fast_limo_amd import api

    def make(model):
        d2 = api.ndt_params(outlier_ratio, model["leaf"])[1]

        def linearize(xs):
            out = dict(valid=[], H=[], g=[], cost=[])
            for x in xs:
                r = restate(x, scan, model, hood, d2)
                S, _, _ = fsum_sums(r["C"])
                out["valid"].append(r["valid"]); out["H"].append(S[:21]); out["g"].append(S[21:27]); out["cost"].append(-S[27])
            return {k: np.asarray(v) for k, v in out.items()}
        return linearize
    x = np.asarray(starts, D).reshape(-1, 26)
    for model in models:
        x = api.scan_align(None, x, iters=iters, min_valid=min_valid, linearize=make(model))["x26"]
    return x
