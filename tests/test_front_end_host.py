"""CPU: the references and inputs of the sweep front end's GPU tests (tests/test_gpu_front_end.py).

The numpy restatement of the input stage against a point-by-point loop; the inputs' arranged properties (NaN tiles, the tile inside
the crop box, where the ties sit, which quaternion branch a point takes); the oracle's float32 deskew against an independent float64
reference over the very inputs the GPU test uses; the numpy voxel grid (int64 lattice, sequential float32 sums) against the
oracle's, bit for bit."""
import numpy as np
import pytest

import front_end_common as fc
from front_end_common import F32


# ---- input filter ----------------------------------------------------------------------------------------------------------------
def _filter_loop(xyz, cfg):
    """Localizer.cpp:262-302 one point after the other."""
    keep, rank = [], 0
    mn, mx = np.asarray(cfg["crop_min"], F32), np.asarray(cfg["crop_max"], F32)
    for i, p in enumerate(xyz):
        if not np.all(np.isfinite(p)):
            continue
        if cfg["crop_active"] and not (np.any(p < mn) or np.any(p > mx)):
            continue
        ok = True
        if cfg["dist_active"]:
            with np.errstate(over="ignore"):
                ok = ok and bool(np.sqrt(F32(p[0] * p[0]) + F32(F32(p[1] * p[1]) + F32(p[2] * p[2]))) > F32(cfg["min_dist"]))
        if cfg["rate_active"]:
            ok = ok and rank % cfg["rate_value"] == 0
        if cfg["fov_active"]:
            ok = ok and bool(np.abs(fc.atan2f_host(p[1], p[0])[0]) < F32(cfg["fov_angle"]))
        rank += 1
        if ok:
            keep.append(i)
    return np.array(keep, np.int64)


@pytest.mark.parametrize("rate", [0, 1, 3, 7])
def test_filter_reference_equals_the_point_loop(rate):
    xyz, rel = fc.sweep(3000, 5, scale=8.0)
    xyz[::53] = np.nan
    xyz[7] = (np.inf, 0, 0)
    cfg = fc.filter_cfg(crop_active=1, crop_min=(-2, -2, -2), crop_max=(2, 2, 2), dist_active=1, min_dist=5.0, rate_active=int(rate > 0),
                        rate_value=max(rate, 1), fov_active=1, fov_angle=2.5)
    ref = fc.filter_reference(xyz, rel, cfg)
    np.testing.assert_array_equal(np.flatnonzero(ref["keep"]), _filter_loop(xyz, cfg))
    assert 0 < ref["n_kept"] < 3000 and ref["xyz"].shape == (ref["n_kept"], 3)
    np.testing.assert_array_equal(ref["stamps"][ref["order"]], np.sort(ref["stamps"]))
    assert ref["last_stamp"] == ref["stamps"].max() and ref["tied"] == 0


def test_big_sweep_is_arranged_as_stated():
    assert fc.N_MAX == 130 * fc.TILE + 37 and (fc.N_MAX + fc.TILE - 1) // fc.TILE == 131        # look-back rounds of 64, 64 and 2 tiles
    cfg = fc.filter_cfg(crop_active=1, crop_min=(-2, -2, -2), crop_max=(2, 2, 2), dist_active=1, min_dist=5.0)
    for variant in ("all", "last", "first"):
        xyz, rel = fc.big_sweep(variant)
        assert xyz.shape == (fc.N_MAX, 3) and np.unique(rel).size == fc.N_MAX
        ref = fc.filter_reference(xyz, rel, cfg)
        per_tile = np.add.reduceat(ref["keep"].astype(np.int64), np.arange(0, fc.N_MAX, fc.TILE))
        for t in (5, 64, 129):
            assert not np.isfinite(xyz[t * fc.TILE:(t + 1) * fc.TILE]).all(axis=1).any()
            assert per_tile[t] == 0
        assert np.all(np.abs(xyz[70 * fc.TILE:71 * fc.TILE]) <= 2.0) and per_tile[70] == 0
        if variant == "all":
            assert (per_tile > 0).sum() == 131 - 4
        else:
            only = 130 if variant == "last" else 0
            assert per_tile[only] > 0 and per_tile.sum() == per_tile[only]
            no_dist = fc.filter_reference(xyz, rel, dict(cfg, dist_active=0))
            assert no_dist["n_kept"] > 100000                                      # the distance alone removes the rest


def test_stamp_cases_place_ties_where_stated():
    cases = {c["name"]: c for c in fc.stamp_cases()}
    n = fc.N_STAMPS
    for name, c in cases.items():
        ref = fc.filter_reference(c["xyz"], c["tw"], fc.filter_cfg(time_kind=c["kind"], end_of_sweep=c["eos"], sweep_ref_time=c["ref"]))
        assert ref["n_kept"] == len(c["tw"])
        if ref["nan_stamp"]:
            assert "nan" in name
            continue
        key = np.asarray(c["tw"])[ref["order"]]
        eq = np.flatnonzero(key[1:] == key[:-1])
        if "tie-255-256" in name:
            assert eq.tolist() == ([n - 257] if c["eos"] and c["kind"] <= 1 else [255])      # (descending: the same pair, counted from the end)
        elif "tie-last-pair" in name:
            assert eq.tolist() == ([0] if c["eos"] and c["kind"] <= 1 else [n - 2])
        elif "all-" in name or "two-equal" in name:
            assert eq.size == len(c["tw"]) - 1
        elif "zeros" in name:
            assert eq.size == 1 and key[eq[0]] == 0 and np.signbit(key[eq[0]]) != np.signbit(key[eq[0] + 1])
        else:
            assert eq.size == 0 and ref["tied"] == 0
        assert ref["tied"] == int(eq.size > 0)
    # where the ties sit among the sorted keys: one pair at 255 / 256 straddles the 256-thread blocks of the tie detection
    d = cases["velodyne-zeros-denormals-eos0"]["tw"]
    assert np.unique(bits_nonzero(d)).size == d.size - 0 and (np.abs(d[2:8]) < 1.2e-38).all() and (d < 0).sum() > 30
    assert fc.filter_reference(cases["velodyne-denormals-no-tie-eos0"]["xyz"], cases["velodyne-denormals-no-tie-eos0"]["tw"],
                               fc.filter_cfg())["tied"] == 0


def bits_nonzero(a):
    """The bit patterns, which tell -0.0 from +0.0."""
    return fc.bits(np.asarray(a, F32))


def test_stamp_decodings_by_hand():
    """pt.t * 1e-9f is a float product, pt.timestamp * 1e-9f a double one; end of sweep subtracts."""
    xyz = np.zeros((1, 3), F32) + 9
    r = fc.filter_reference(xyz, np.array([0xffffffff], np.uint32), fc.filter_cfg(time_kind=0, end_of_sweep=1, sweep_ref_time=10.0))
    assert r["last_stamp"] == 10.0 - float(F32(4294967296.0) * F32(1e-9))
    r = fc.filter_reference(xyz, np.array([0.1], F32), fc.filter_cfg(time_kind=1, sweep_ref_time=10.0))
    assert r["last_stamp"] == 10.0 + float(F32(0.1))
    r = fc.filter_reference(xyz, np.array([1.5e18]), fc.filter_cfg(time_kind=3))
    assert r["last_stamp"] == 1.5e18 * float(F32(1e-9)) != 1.5e9


# ---- deskew ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deskew_data(oracle):
    out = {}
    for nf, case in fc.deskew_cases().items():
        body, world = oracle.deskew_points(case["xyz"], case["t"], case["frames"], case["L2B"], case["x26"])
        out[nf] = dict(case=case, body=body, world=world, ref=fc.deskew_f64(case))
    return out


def test_deskew_inputs_cover_what_they_claim(deskew_data):
    total = np.zeros(4, np.int64)
    assert all(min(abs(c) for c in a) > 0.15 for a in fc.AXES)                       # no pure axis: every off-diagonal sum of a branch counts
    for nf, d in deskew_data.items():
        case, ref = d["case"], d["ref"]
        fr, t = case["frames"], case["t"]
        n_fr = 72 if nf == 73 else nf
        assert fr.shape[0] == nf and case["xyz"].shape == (fc.N_DESKEW, 3) and np.all(np.diff(t) >= 0)
        assert np.all(np.diff(fr["time"]) > 0)
        assert (t < fr["time"][0]).sum() == 64 and np.isclose(fr["time"][0] - t.min(), 0.3)
        assert np.isclose(t.max() - fr["time"][n_fr - 1], 0.3)
        assert np.isin(fr["time"][:n_fr], t).all()                                   # a stamp equal to every frame's time
        if nf == 73:
            assert t.max() < fr["time"][72] - 9 and ref["i_f"].max() == 71            # no stamp reaches the appended frame
        assert not np.allclose(fr["q"][:, 3], 1) and all(np.abs(fr[k]).min() > 0 for k in ("v", "a", "ba", "g"))
        # |w - bg| as the float32 code forms it, either side of the threshold and on it
        wv = (fr["w"] - fr["bg"]).astype(F32)
        wn = np.sqrt(wv[:, 0] * wv[:, 0] + (wv[:, 1] * wv[:, 1] + wv[:, 2] * wv[:, 2]))
        if nf >= 72:
            assert (wn == F32(0.9e-7)).any() and (wn == F32(1.1e-7)).any() and (wn == 0).any()
            on = wn == fc.THR
            assert on.any() and np.all(wn[on].astype(np.float64) > 1e-7) and not np.any(wn[on] > F32(1e-7))
        # the angles |w| dt the points see
        ang = np.linalg.norm((fr["w"].astype(np.float64) - fr["bg"])[ref["i_f"]], axis=1) * ref["dt"]
        for a in (2.0, 2.2, 3.1, 3.2, 6.0):
            assert (np.abs(ang + a) < 1e-3).any(), (nf, -a)                         # before the first frame: negative dt
            assert (np.abs(ang - a) < 1e-3).any(), (nf, a)
        if nf >= 72:
            assert (np.abs(ang - 0.01) < 1e-5).any() and (ang == 0).any()
        br = np.array(fc.quat_branches(ref))
        print(f"deskew nf = {nf}: points per quaternion branch [tr > 0, x, y, z] = {br.tolist()}")
        if nf >= 72:
            assert np.all(br >= 100), (nf, br)
        total += br
    assert np.all(total >= 100), total


def test_oracle_deskew_against_the_float64_reference(deskew_data):
    worst = 0.0
    for nf, d in deskew_data.items():
        ref = d["ref"]
        unit = 2.0**-24 * ref["scale"]
        rb = np.linalg.norm(d["body"].astype(np.float64) - ref["body"], axis=1) / unit
        rw = np.linalg.norm(d["world"][:, :3].astype(np.float64) - ref["world"], axis=1) / unit
        print(f"deskew nf = {nf}: worst |float32 - float64| / (2^-24 scale): body {rb.max():.3f}, world {rw.max():.3f}")
        assert np.all(d["world"][:, 3] == 1.0)
        worst = max(worst, rb.max(), rw.max())
    print(f"deskew: measured worst ratio {worst:.3f} (front_end_common.DESKEW_F64_RATIO = {fc.DESKEW_F64_RATIO})")
    assert worst <= 4.0 * fc.DESKEW_F64_RATIO


def test_oracle_deskew_entry_is_the_localizers_loop(oracle):
    """oracle_deskew_points is the factored loop body: State::update of the chosen frame, through oracle_state_update, then the
    three matrix products in float32 give the same bits."""
    case = fc.deskew_case(3)
    body, world = oracle.deskew_points(case["xyz"], case["t"], case["frames"], case["L2B"], case["x26"])
    fr, i_f = case["frames"], fc.deskew_f64(case)["i_f"]
    RTi = oracle.pose_mats(case["x26"])[1]
    L = case["L2B"]
    for i in range(0, fc.N_DESKEW, 37):
        F = fr[i_f[i]]
        s = np.concatenate([F[k] for k in ("p", "q", "v", "g", "w", "a", "bg", "ba")]).astype(F32)
        s = oracle.state_update(s, F["time"], case["t"][i])
        x26 = np.zeros(26); x26[0:3] = s[0:3]; x26[3:7] = s[3:7]; x26[10] = 1
        X = oracle.pose_mats(x26)[0]
        T = np.zeros((4, 4), F32)
        for r in range(4):
            for c in range(4):
                acc = F32(X[r, 0] * L[0, c])
                for k in (1, 2, 3):
                    acc = F32(acc + F32(X[r, k] * L[k, c]))
                T[r, c] = acc
        p = np.append(case["xyz"][i], F32(1))
        pw = np.array([F32(F32(F32(T[r, 0] * p[0]) + F32(T[r, 1] * p[1])) + F32(T[r, 2] * p[2])) + F32(T[r, 3] * p[3]) for r in range(4)], F32)
        pb = np.array([F32(F32(F32(RTi[r, 0] * pw[0]) + F32(RTi[r, 1] * pw[1])) + F32(RTi[r, 2] * pw[2])) + F32(RTi[r, 3] * pw[3]) for r in range(3)], F32)
        assert pw.tobytes() == world[i].tobytes() and pb.tobytes() == body[i].tobytes(), i


# ---- voxel grid ------------------------------------------------------------------------------------------------------------------
def test_voxel_reference_equals_the_oracle_bit_for_bit(oracle):
    inputs = fc.voxel_inputs()
    for nf in (0, 1, 3):
        for m in (1, 8, 9, 16, 17):
            inputs.append((f"tail-run-{m}-nonfinite-{nf}", fc.voxel_tail_run(m, nf), 0.25))
    for name, scan, leaf in inputs:
        ref, orc = fc.voxel_reference(scan, leaf), oracle.voxel_grid(scan, leaf)
        assert ref.shape == orc.shape and 0 < ref.shape[0] <= scan.shape[0], name
        assert ref.tobytes() == orc.tobytes(), name
    one = fc.voxel_reference(fc.voxel_one_cell(), 0.25)
    assert one.shape == (1, 3)
    # the largest key's run is the sorted keys' last: the m points at (5, 5, 5) make the last output point
    for m in (1, 8, 9, 16, 17):
        scan = fc.voxel_tail_run(m, 3)
        top = scan[300:300 + m]
        last = fc.voxel_reference(scan, 0.25)[-1]
        np.testing.assert_array_equal(last, np.cumsum(top, axis=0, dtype=F32)[-1] / F32(m))
    # points exactly on faces went in
    assert (np.mod(fc.voxel_scan(256, 0.25, 1) / F32(0.25), 1) == 0).all(axis=1).sum() >= 60


def test_voxel_edge_returns(oracle):
    assert fc.voxel_reference(fc.NONFINITE, 0.25).shape == (0, 3) and oracle.voxel_grid(fc.NONFINITE, 0.25).shape == (0, 3)
    for name, scan, leaf in fc.voxel_passthrough_inputs():
        ref, orc = fc.voxel_reference(scan, leaf), oracle.voxel_grid(scan, leaf)
        assert ref.tobytes() == scan.tobytes() == orc.tobytes(), name                # the input unchanged, non-finite points included
    # the lattices are what the names say, in 64-bit
    inv = F32(1) / F32(0.1)
    corners = fc.voxel_passthrough_inputs()[0][1]
    fin = corners[np.isfinite(corners).all(axis=1)]
    div = np.floor(fin.max(axis=0) * inv).astype(np.int64) - np.floor(fin.min(axis=0) * inv).astype(np.int64) + 1
    assert np.all(div < 2**31) and int(div[0]) * int(div[1]) * int(div[2]) > fc.INT_MAX
    axis = fc.voxel_passthrough_inputs()[1][1]
    fin = axis[np.isfinite(axis).all(axis=1)]
    d0 = int(np.floor(fin[:, 0].max())) - int(np.floor(fin[:, 0].min())) + 1
    assert d0 > 2**31 and np.int32(np.int64(d0) & 0xffffffff) < 0                  # as an int difference it wraps below zero
