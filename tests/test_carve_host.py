"""Map carving (forget the stored points a sweep looks through) as far as it can be checked without a GPU: both libraries export and
declare the new entry points, the policy's counting rule -- flimo_carve_rule, the pure host function Localizer::set_map_carving
applies after every map insert -- agrees with its Python restatement api.CarveRule, and the numpy yardstick of the predicate
(tests/carve_common.py) has the properties the definition promises.  The kernels run on the GPU: tests/test_gpu_carve.py."""
import ctypes as C
import os

import numpy as np
import pytest

import carve_common as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -2


def test_new_entry_points_are_exported_and_declared(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    pub = open(os.path.join(ROOT, "include", "flimo_c.h")).read()
    for name in ("flimo_map_seen_through", "flimo_map_carve"):
        assert hasattr(L, name), name
        assert name in _lib.HIP_SYMBOLS and name in pub
    assert "flimo_carve_cfg" in pub
    assert hasattr(L, "flimo_map_carve_stats") and "flimo_map_carve_stats" in _lib.HIP_SYMBOLS
    assert "flimo_map_carve_stats" in open(os.path.join(ROOT, "include", "flimo_dev.h")).read()
    H = api.load_host()
    decl = open(os.path.join(ROOT, "include", "flimo_localizer_c.h")).read()
    for name in ("flimo_loc_set_map_carving", "flimo_carve_rule", "flimo_carve_sensor", "flimo_loc_map_seen_through", "flimo_loc_map_carve",
                 "flimo_loc_last_carve_removed"):
        assert hasattr(H, name), name
        assert name in api.HOST_SYMBOLS and name in decl
    for name in ("map_seen_through", "map_carve", "map_carve_stats"):
        assert hasattr(_lib.HipCtx, name), name
    for name in ("set_map_carving", "map_seen_through", "map_carve"):
        assert hasattr(api.Localizer, name), name
    assert hasattr(api, "CarveRule")


def test_the_calls_reject_a_null_context_and_leave_their_outputs(built):
    from fast_limo_amd import _lib
    L = _lib.load_hip()
    x = np.zeros(26); x[6] = 1
    s = np.zeros(3, np.float32)
    k = _lib.carve_cfg()
    out = C.c_size_t(5)
    assert L.flimo_map_seen_through(None, x.ctypes.data, s.ctypes.data, C.byref(k), None, 0, C.byref(out)) == ERR_INVALID
    assert L.flimo_map_carve(None, x.ctypes.data, s.ctypes.data, C.byref(k), None, None, C.byref(out)) == ERR_INVALID
    assert out.value == 5


@pytest.mark.parametrize("every", [-3, 0, 1, 2, 3, 7])
def test_the_counting_rule_agrees_with_its_python_twin(built, every):
    from fast_limo_amd import api
    L = api.load_host()
    twin = api.CarveRule(every)
    count = C.c_int(0)
    fired = []
    for sweep in range(30):
        before = count.value
        rc = L.flimo_carve_rule(every, C.byref(count))
        want = twin.step()
        if every <= 0:
            assert rc == -1 and twin.off and not want and count.value == before      # off: nothing written
        else:
            assert rc == (1 if want else 0), (every, sweep)
            assert count.value == twin.count
            fired.append(rc)
    if every > 0:
        # every n-th inserted sweep: sweeps n, 2n, .. (counted from 1)
        assert [i + 1 for i, f in enumerate(fired) if f] == list(range(every, 31, every))
    assert L.flimo_carve_rule(3, None) == -1


def test_the_policy_sensor_origin_agrees_with_its_python_twin(built):
    from fast_limo_amd import api
    L = api.load_host()
    rng = np.random.default_rng(3)
    for _ in range(50):
        x = np.zeros(26)
        x[0:3] = rng.uniform(-500, 500, 3)
        q = rng.normal(size=4); x[3:7] = q / np.linalg.norm(q)
        x[10] = 1.0
        x[11:14] = rng.uniform(-2, 2, 3)
        out = np.zeros(3, np.float32)
        L.flimo_carve_sensor(x, out)
        np.testing.assert_array_equal(out, api.carve_sensor(x))
        # the lidar's origin moved by the pose, in float64, rounded once
        ref = x[0:3] + _rot(x[3:7]) @ x[11:14]
        assert np.abs(out.astype(np.float64) - ref).max() <= 2.0 ** -23 * 512
    x = np.zeros(26); x[6] = 1; x[10] = 1; x[0:3] = (0.30, -0.20, 0.05)
    np.testing.assert_array_equal(api.carve_sensor(x), np.float32([0.30, -0.20, 0.05]))      # identity extrinsics: float(t)


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- the yardstick's own properties, on the standard scene -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    static, ghost, scan, x26, sensor = cc.standard_scene()
    return dict(static=static, ghost=ghost, world=cc.standard_world(scan, x26), sensor=sensor, q=np.concatenate([static, ghost]))


@pytest.mark.parametrize("win", [0, 1])
def test_the_scans_own_points_are_never_seen_through(scene, win):
    for res in (8, 64, 256):
        m = cc.yardstick(scene["world"], scene["world"], scene["sensor"], res, win, 0.0, 0.0)
        assert m.sum() == 0, (res, win, m.sum())


def test_the_mask_is_monotone_in_margin_rel_margin_and_win(scene):
    D = cc.range_image(scene["world"], scene["sensor"], 64)

    def mask(win=1, margin=0.2, rel=0.02):
        return cc.seen_through(scene["q"], D, scene["sensor"], win, margin, rel)

    for lo, hi in zip((0.0, 0.05, 0.2, 1.0), (0.05, 0.2, 1.0, 5.0)):
        assert not np.any(mask(margin=hi) & ~mask(margin=lo)), ("margin", lo, hi)
        assert not np.any(mask(rel=hi) & ~mask(rel=lo)), ("rel_margin", lo, hi)
    for w in range(3):
        assert not np.any(mask(win=w + 1) & ~mask(win=w)), ("win", w)
    assert mask(margin=0.0).sum() > mask(margin=5.0).sum()            # (and it does fall)


def test_permuting_the_scan_leaves_the_image_bit_equal(scene):
    w = scene["world"]
    perm = np.random.default_rng(1).permutation(len(w))
    for res in (8, 64, 300):
        a, b = cc.range_image(w, scene["sensor"], res), cc.range_image(w[perm], scene["sensor"], res)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.isfinite(a).any()


def test_the_standard_scene_keeps_the_static_map_and_loses_the_ghost(scene):
    n = len(scene["static"])
    m = cc.yardstick(scene["world"], scene["q"], scene["sensor"], **cc.STD_CFG)
    print("standard scene: static removed %d, ghost removed %d of %d" % (m[:n].sum(), m[n:].sum(), cc.N_GHOST))
    assert m[:n].sum() == 0
    assert m[n:].sum() >= 0.7 * cc.N_GHOST
    m2 = cc.yardstick(scene["world"], scene["q"], scene["sensor"], res=128, win=2, margin=0.2, rel_margin=0.0)
    print("res 128 / win 2 / margin 0.2 / rel 0: static removed %d, ghost removed %d" % (m2[:n].sum(), m2[n:].sum()))
    assert m2[:n].sum() == 0
    assert m2[n:].sum() >= 0.7 * cc.N_GHOST
    # why win >= 1 is the documented default: with no window and no margin a grazing surface is carved by its neighbours' returns
    m0 = cc.yardstick(scene["world"], scene["q"], scene["sensor"], res=64, win=0, margin=0.0, rel_margin=0.0)
    print("win 0, margins 0: static removed %d" % m0[:n].sum())
    assert m0[:n].sum() > 100
