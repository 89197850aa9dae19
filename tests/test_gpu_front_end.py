"""GPU: the four device stages every registration starts with, each driven through the C ABI at its edges.

  input filter   filt_onepass_kernel<16|32> (flimo_raw_scan_filter_order_set): tile and look-back boundaries, partial and empty
                 tiles, rates, descriptor regrowth, predicates on the faces
  time order     time_order_raw / tied_keys_kernel / gather_time_order_kernel: every stamp format at its extremes, tie layouts
  deskew         deskew_world / deskew_body on their three paths (own launch; riding on the first pass with the frames in shared
                 memory; with the frames in global memory), all four quaternion branches, stamps on, before and after the frames
  voxel grid     voxelkey / voxelhead / voxelcentroid (flimo_scan_voxel_filter): run lengths around the batch of 8, the tail of the
                 sorted keys, both early returns, lattices beyond an int

References (tests/front_end_common.py; tests/test_front_end_host.py checks them on the CPU): the numpy restatement of the input
stage, the oracle's deskew_points and voxel_grid.  Every comparison is exact.

How the resident raw sweep is read: a deskew with the IMU frames of a body at rest returns every kept point as it is; a deskew with
one frame of velocity (1, 0, 0) and a lidar2baselink_T without rotation returns float32(stamp - frame time) per point."""
import struct

import numpy as np
import pytest

import front_end_common as fc
from front_end_common import F32

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4096, 131072, 131073, fc.N_MAX)
CROP = dict(crop_active=1, crop_min=(-2.0, -2.0, -2.0), crop_max=(2.0, 2.0, 2.0))
EYE4 = np.eye(4, dtype=F32)


@pytest.fixture(scope="module")
def lib(built):
    from fast_limo_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def hip(lib):
    """One context with a small map (a pass needs one) for the tests that do not need a fresh context."""
    ctx = lib.HipCtx(0)          # raises without a gfx950 device
    ctx.map_config()
    ctx.map_add(np.random.RandomState(1).uniform(-30, 30, (3000, 3)).astype(F32))
    assert not ctx.fine_stats()["active"]
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def big():
    """The 266 277-point sweeps, built once."""
    return {v: fc.big_sweep(v) for v in ("all", "last", "first")}


def _same_double(a, b):
    return struct.pack("d", a) == struct.pack("d", b)


def _read_points(ctx):
    ctx.deskew_resident_offset(fc.rest_frames(0.0), EYE4, fc.REST_X26, 0.0)
    return ctx.scan_get()


def _read_stamps(ctx, t0):
    ctx.deskew_resident_offset(fc.stamp_readback_frames(t0), fc.stamp_readback_l2b(), fc.REST_X26, 0.0)
    return ctx.scan_get()


def _filter_and_check(ctx, lib, xyz, tw, cfg, time_order, rec_bytes, tag):
    """One flimo_raw_scan_filter_order_set against filter_reference: kept count, last stamp, NaN mark, tie mark; what is resident
    afterwards (points, stamps, time order), or that nothing is."""
    ref = fc.filter_reference(xyz, tw, cfg)
    kind = cfg["time_kind"]
    rec = fc.records16(xyz, tw, kind) if rec_bytes == 16 else fc.records32(xyz, tw, kind)
    kept, last, nan, tied = ctx.raw_scan_filter_order_set(rec, time_order | (4 if rec_bytes == 16 else 0), **cfg)
    ordered = bool(time_order & 1)
    assert (kept, nan) == (ref["n_kept"], ref["nan_stamp"]), (tag, kept, nan)
    assert _same_double(last, ref["last_stamp"]), (tag, last, ref["last_stamp"])
    assert tied == (ref["tied"] if ordered else 0), (tag, tied)
    resident = kept > 0 and not nan and not (ordered and ref["tied"] and not (time_order & 8))
    if not resident:
        ctx.deskew_resident_offset(fc.rest_frames(0.0), EYE4, fc.REST_X26, 0.0)
        assert ctx.scan_size() == 0 and ctx.scan_get().shape[0] == 0, tag
        assert ctx.raw_scan_order().size == 0, tag
        return ref
    perm = ref["order"] if ordered else np.arange(kept)
    np.testing.assert_array_equal(ctx.raw_scan_order(), perm.astype(np.uint32), err_msg=f"{tag} (time order)")
    np.testing.assert_array_equal(_read_points(ctx), ref["xyz"][perm], err_msg=f"{tag} (kept points)")
    t0 = float(np.floor(ref["stamps"].min()))
    st = _read_stamps(ctx, t0)
    np.testing.assert_array_equal(st[:, 0], (ref["stamps"][perm] - t0).astype(F32), err_msg=f"{tag} (stamps)")
    assert not st[:, 1:].any(), tag
    return ref


# ---- 1. filter sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0, 1, 3, 7])
@pytest.mark.parametrize("rec_bytes", [32, 16])
def test_filter_sizes_on_one_context(lib, big, rec_bytes, rate):
    """Tile boundaries (2 048 points), look-back rounds (64 tiles: 131 072 points), a last tile of 1 and of 37 points, tiles that keep
    nothing; then a small sweep, the largest again and an empty one on the same context: the descriptors are re-allocated on the way
    up and reused on the way down."""
    cfg = fc.filter_cfg(dist_active=1, min_dist=5.0, rate_active=int(rate > 0), rate_value=max(rate, 1), time_kind=1,
                        sweep_ref_time=fc.SWEEP_REF, **CROP)
    ctx = lib.HipCtx(0)
    try:
        xyz, rel = big["all"]
        seen = {}
        for step, (variant, n, order) in enumerate([("all", n, 1) for n in SIZES] + [("last", fc.N_MAX, 1), ("first", fc.N_MAX, 0),
                                                    ("all", 3000, 1), ("all", fc.N_MAX, 0), ("all", 0, 1)]):
            xyz, rel = big[variant]
            ref = _filter_and_check(ctx, lib, xyz[:n], rel[:n], cfg, order, rec_bytes, f"step {step}: {variant} n = {n}")
            seen[(variant, n)] = ref["n_kept"]
        assert seen[("all", fc.N_MAX)] > 60000 // max(rate, 1) and seen[("all", 0)] == 0
        assert 0 < seen[("last", fc.N_MAX)] <= 37 and 0 < seen[("first", fc.N_MAX)] <= fc.TILE
    finally:
        ctx.close()


@pytest.mark.parametrize("what", ["nan", "cropped", "near"])
def test_everything_removed_leaves_an_empty_scan(hip, lib, what):
    n = 5000
    xyz = np.random.RandomState(2).uniform(-1.5, 1.5, (n, 3)).astype(F32)
    if what == "nan":
        xyz[:, 1] = np.nan
    cfg = fc.filter_cfg(dist_active=int(what == "near"), min_dist=5.0, rate_active=1, rate_value=3, **(CROP if what == "cropped" else {}))
    rel = fc.sweep(n, 3)[1]
    for rec_bytes in (32, 16):
        ref = _filter_and_check(hip, lib, xyz, rel, cfg, 1, rec_bytes, what)
        assert ref["n_kept"] == 0
        hip.deskew_resident_offset(fc.rest_frames(0.0), EYE4, fc.REST_X26, 0.0)
        assert hip.scan_size() == 0
        _, _, M = hip.match_reduce(fc.REST_X26, lib.default_match_cfg())
        assert M == 0


def test_descriptor_regrowth_right_after_the_first_call(lib, big):
    """A context whose FIRST sweep is small and whose second needs more tile descriptors: the second call's launch number must not
    start again at the first call's, whose results still sit in the host's mail words (a stale kept count came back).  The same for
    the tie mark, which only time-ordered calls write."""
    cfg = fc.filter_cfg(dist_active=1, min_dist=5.0, rate_active=1, rate_value=3, sweep_ref_time=fc.SWEEP_REF, **CROP)
    xyz, rel = big["all"]
    ctx = lib.HipCtx(0)
    try:
        a = _filter_and_check(ctx, lib, xyz[:3000], rel[:3000], cfg, 1, 32, "first call")
        b = _filter_and_check(ctx, lib, xyz, rel, cfg, 1, 32, "second call, more tiles")
        assert a["n_kept"] != b["n_kept"]
    finally:
        ctx.close()
    ctx = lib.HipCtx(0)
    try:
        tied = rel[:3000].copy(); tied[:] = tied[0]
        a = _filter_and_check(ctx, lib, xyz[:3000], tied, cfg, 1 | 8, 32, "first call, tied, time order")
        _filter_and_check(ctx, lib, xyz[:3000], rel[:3000], cfg, 0, 32, "second call, arrival order")
        b = _filter_and_check(ctx, lib, xyz, rel, cfg, 1, 32, "third call, more tiles, no ties")
        assert a["tied"] == 1 and b["tied"] == 0
    finally:
        ctx.close()


# ---- 2. filter predicates --------------------------------------------------------------------------------------------------------
def test_crop_faces_and_min_distance_are_strict(hip, lib):
    mn, mx = (-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)
    pts, expect = [], []
    for a in range(3):
        for bound, away in ((mx[a], np.inf), (mn[a], -np.inf)):
            on = np.zeros(3, F32); on[a] = bound
            off = on.copy(); off[a] = np.nextafter(F32(bound), F32(away))
            pts += [on, off]; expect += [False, True]                               # on a face is inside the box: removed
    pts += [np.array(mx, F32), np.array(mn, F32), np.array([0, 0, 0], F32)]; expect += [False, False, False]
    # min distance 5: |(3, 4, 0)| = 5 exactly is not beyond it
    pts += [np.array([3, 4, 0], F32), np.array([3, 4, 0.01], F32), np.array([-3, -4, 0], F32), np.array([0, 5, np.nextafter(F32(0.01), F32(1))], F32)]
    expect += [False, True, False, True]
    xyz = np.array(pts, F32)
    rel = fc.sweep(len(pts), 4)[1]
    cfg = fc.filter_cfg(crop_active=1, crop_min=mn, crop_max=mx, dist_active=0, min_dist=5.0)
    ref = _filter_and_check(hip, lib, xyz, rel, cfg, 0, 32, "faces")
    np.testing.assert_array_equal(ref["keep"][:15], np.array(expect[:15]))
    ref = _filter_and_check(hip, lib, xyz[15:], rel[15:], dict(cfg, crop_active=0, dist_active=1), 0, 16, "min distance")
    np.testing.assert_array_equal(ref["keep"], np.array(expect[15:]))


def test_fov_on_the_axes_and_one_ulp_either_side(hip, lib):
    """fabs(atan2f(y, x)) < fov_angle with the host's atan2f: the +x axis (angle +-0) is inside, the -x axis (+-pi) is not below
    float32(pi), (0, 0, z) has angle 0; an angle one ulp either side of a point's own decides it."""
    y, x = F32(4.5), F32(3.0)
    a = fc.atan2f_host(y, x)[0]
    xyz = np.array([[10, 0.0, 1], [10, -0.0, 1], [-10, 0.0, 1], [-10, -0.0, 1], [0, 0, 7], [0.0, -0.0, -7], [x, y, 1], [x, -y, 1],
                    [-3, 4.5, 1], [0, 9, 0], [0, -9, 0]], F32)
    rel = fc.sweep(xyz.shape[0], 6)[1]
    seen = {}
    for name, angle in (("pi", F32(3.14159265)), ("at", a), ("above", np.nextafter(a, F32(4))), ("below", np.nextafter(a, F32(0)))):
        cfg = fc.filter_cfg(fov_active=1, fov_angle=float(angle))
        for rec_bytes in (32, 16):
            try:
                ref = _filter_and_check(hip, lib, xyz, rel, cfg, 0, rec_bytes, f"fov {name}")
            except lib.FlimoError as e:
                if str(e).startswith("unsupported"):
                    pytest.skip(str(e))
                raise
        seen[name] = ref["keep"]
    np.testing.assert_array_equal(seen["pi"], [1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1])
    assert not seen["at"][6] and not seen["at"][7] and seen["above"][6] and seen["above"][7] and not seen["below"][6]
    assert seen["above"][:2].all() and seen["above"][4:6].all() and not seen["above"][2:4].any()


@pytest.mark.parametrize("rate_value", [0, -1])
def test_rate_below_one_is_invalid_and_touches_nothing(hip, lib, rate_value):
    xyz, rel = fc.sweep(100, 8)
    _filter_and_check(hip, lib, xyz, rel, fc.filter_cfg(), 0, 32, "resident sweep")
    with pytest.raises(lib.FlimoError, match="invalid argument"):
        hip.raw_scan_filter_order_set(fc.records32(xyz[:50], rel[:50], 1), 0, **fc.filter_cfg(rate_active=1, rate_value=rate_value))
    np.testing.assert_array_equal(_read_points(hip), xyz)


# ---- 3. stamps and the time order ------------------------------------------------------------------------------------------------
STAMP_CASES = fc.stamp_cases()


@pytest.mark.parametrize("case", STAMP_CASES, ids=[c["name"] for c in STAMP_CASES])
def test_stamps_last_stamp_and_ties(hip, lib, case):
    """Every decoding, its extremes, and the tie layouts: without bit 3 a tied sweep is reported and nothing is resident, with it
    the order is the stable one; in arrival order (time_order 0) no tie is looked for."""
    cfg = fc.filter_cfg(time_kind=case["kind"], end_of_sweep=case["eos"], sweep_ref_time=case["ref"])
    for rec_bytes in ((32, 16) if case["kind"] <= 1 else (32,)):
        for time_order in (1, 1 | 8, 0, 1 | 2 | 8):
            _filter_and_check(hip, lib, case["xyz"], case["tw"], cfg, time_order, rec_bytes, f"{case['name']} order {time_order} rec {rec_bytes}")


# ---- 4. deskew -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deskew_cases():
    return fc.deskew_cases()


def _deskew_three_ways(ctx, lib, oracle, case, tag):
    """deskew_kernel on its own; riding on the first pass; through the debug clouds: the same bits, the oracle's."""
    body, world = oracle.deskew_points(case["xyz"], case["t"], case["frames"], case["L2B"], case["x26"])
    ctx.raw_scan_set(case["xyz"], case["t"])
    ctx.deskew_resident(case["frames"], case["L2B"], case["x26"])
    own = ctx.scan_get()                                                             # a pending deskew is run by its own launch
    assert own.tobytes() == body.tobytes(), f"{tag}: deskew_kernel"
    passes = ctx.pass_count()
    ctx.deskew_resident(case["frames"], case["L2B"], case["x26"])
    ctx.match_reduce(case["x26"], lib.default_match_cfg())                           # the first pass of the scan carries the deskew
    assert ctx.pass_count() == passes + 1
    ride = ctx.scan_get()
    assert ride.tobytes() == body.tobytes(), f"{tag}: deskew on the first pass"
    ctx.deskew_resident(case["frames"], case["L2B"], case["x26"])
    dw, fr = ctx.scan_debug_clouds(fc.REST_X26)
    assert dw.tobytes() == world.tobytes(), f"{tag}: deskewed_scan (world frame)"
    np.testing.assert_array_equal(fr[:, :3], body, err_msg=f"{tag}: final_raw_scan under the identity pose")
    assert np.all(fr[:, 3] == 1.0)
    assert ctx.scan_get().tobytes() == body.tobytes(), tag
    return own


@pytest.mark.parametrize("nf", fc.NF_CASES)
def test_deskew_three_ways_equal_the_oracle(hip, lib, oracle, deskew_cases, nf):
    """nf <= 72: the frames go through the host-stored slot and shared memory; from 73: through the staged copy and global memory.
    Stamps before, on, between and after the frames; all four quaternion-from-matrix branches (test_front_end_host counts them)."""
    _deskew_three_ways(hip, lib, oracle, deskew_cases[nf], f"nf = {nf}")


def test_deskew_frame_paths_agree_at_the_slot_limit(hip, lib, oracle, deskew_cases):
    a, b = deskew_cases[72], deskew_cases[73]
    assert b["frames"].shape[0] == 73 and b["frames"][:72].tobytes() == a["frames"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
    assert 72 * 112 + 128 <= 8192 < 73 * 112 + 128
    out72 = _deskew_three_ways(hip, lib, oracle, a, "72 frames")
    out73 = _deskew_three_ways(hip, lib, oracle, b, "72 frames + one no stamp reaches")
    assert out72.tobytes() == out73.tobytes()


# ---- 5. voxel grid ---------------------------------------------------------------------------------------------------------------
ORDINARY = fc.voxel_scan(257, 0.25, 99)


def _voxel(ctx, scan, leaf):
    ctx.scan_set(scan)
    n = ctx.scan_voxel_filter(leaf)
    got = ctx.scan_get()
    assert n == got.shape[0] == ctx.scan_size()
    return got


def _voxel_check(ctx, oracle, name, scan, leaf):
    ref = oracle.voxel_grid(scan, leaf)
    got = _voxel(ctx, scan, leaf)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
    # the flags words and the box are re-armed: an ordinary call on the same context is still right
    assert _voxel(ctx, ORDINARY, 0.25).tobytes() == oracle.voxel_grid(ORDINARY, 0.25).tobytes(), f"after {name}"
    return got


def test_voxel_sizes_leaves_and_faces(hip, oracle):
    for name, scan, leaf in fc.voxel_inputs():
        got = _voxel_check(hip, oracle, name, scan, leaf)
        assert 0 < got.shape[0] <= scan.shape[0]
        if name.startswith("one-cell"):
            assert got.shape[0] == 1


def test_voxel_last_run_against_the_end_of_the_keys(hip, oracle):
    """The voxel with the largest key -- the last run of the sorted keys -- holds 1, 8, 9, 16 and 17 points in turn, up and down on
    one context, followed by 0, 1 and 3 non-finite points: the run ends exactly at n, at n - 1, before the non-finite tail; the
    walk's batches of 8 end on it, one short of it and one past it."""
    for nonfinite in (0, 1, 3):
        for m in (1, 8, 9, 16, 17, 16, 9, 8, 1):
            scan = fc.voxel_tail_run(m, nonfinite)
            ref = oracle.voxel_grid(scan, 0.25)
            got = _voxel(hip, scan, 0.25)
            assert got.tobytes() == ref.tobytes(), (m, nonfinite)
            np.testing.assert_array_equal(got[-1], np.cumsum(scan[300:300 + m], axis=0, dtype=F32)[-1] / F32(m))


def test_voxel_no_finite_point_is_empty_not_a_pass_through(hip, oracle):
    for scan in (fc.NONFINITE, fc.NONFINITE[:1], np.repeat(fc.NONFINITE, 100, axis=0)):
        got = _voxel_check(hip, oracle, "no finite point", scan, 0.25)
        assert got.shape[0] == 0


@pytest.mark.parametrize("which", range(4), ids=[x[0] for x in fc.voxel_passthrough_inputs()])
def test_voxel_lattice_beyond_an_int_passes_through(hip, oracle, which):
    """More than INT_MAX cells -- as the product of three counts that each fit, or on one axis alone (an int difference would wrap) --
    leaves the scan as it is, non-finite points included."""
    name, scan, leaf = fc.voxel_passthrough_inputs()[which]
    got = _voxel_check(hip, oracle, name, scan, leaf)
    assert got.tobytes() == scan.tobytes()
