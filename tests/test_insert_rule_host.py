"""CPU suite: the host statement of the map's insert rule (fast_limo_amd/csrc/hip/flimo_insert.cpp, through
flimo_insert_rule_replay) against the oracle's octree on the edge fixtures of insert_rule_common.py -- leaf counts at 32 / 33 and
4 / 5, half == 2 min_extent, points on centre planes, groups around 2048 points, root growth, deep chains, zero-size roots,
non-finite points.  The device restates the same lines (flimo_gbook.hip); its test is test_gpu_insert_rule.py.

The zero-size-root cases and the batches of only NaNs run in a child process under a time limit and an address-space limit: the
growth loop they once sent spinning allocated a node per turn, and a regression must fail the test, not take the machine's
memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

import insert_rule_common as irc
from common import sort_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = irc.groups()
CHILD_GROUPS = ("zero_root", "nan_and_tiny")
CHILD_SECONDS = 120
CHILD_BYTES = 6 << 30


def _compare(case, downsample, keep, stored, oracle):
    om = irc.OracleMap(oracle, case["min_extent"], downsample)
    for b in case["batches"]:
        om.update(b)
    what = "%s downsample=%s" % (case["name"], downsample)
    assert stored == om.oc.size(), what
    kept = np.concatenate([b[k] for b, k in zip(case["batches"], keep)])
    np.testing.assert_array_equal(sort_rows(kept), sort_rows(om.oc.points()), err_msg=what)
    np.testing.assert_array_equal(kept, om.expect, err_msg=what)            # and in insertion order
    if case["stored"] is not None:
        assert stored == case["stored"][downsample], (what, "the count worked out by hand")
    return om


@pytest.mark.parametrize("downsample", [True, False])
@pytest.mark.parametrize("group", [g for g in GROUPS if g not in CHILD_GROUPS])
def test_host_insert_rule_at_its_edges(built, oracle, group, downsample):
    from fast_limo_amd import _lib
    for case in GROUPS[group]:
        keep, stored = _lib.insert_rule_replay(case["batches"], case["min_extent"], downsample)
        _compare(case, downsample, keep, stored, oracle)


def test_the_fixtures_reach_their_branches(built, oracle):
    """What the builders promise, from the oracle alone: the 32 / 33 pairs differ in what the probe leaves, down-sampling drops
    where the hand count says so, the deep chains are as deep as their names."""
    by = {c["name"]: c for g in GROUPS.values() for c in g}
    for c in by.values():
        if c["stored"] is None:
            continue
        for ds in (True, False):
            om = irc.OracleMap(oracle, c["min_extent"], ds)
            for b in c["batches"]:
                om.update(b)
            assert om.oc.size() == c["stored"][ds], (c["name"], ds)
    assert by["leaf_splittable_31+1"]["stored"][True] - by["leaf_splittable_31+2"]["stored"][True] == 48 - 42 - 1
    assert by["leaf_minimal_4+40_s0.25"]["stored"][True] - by["leaf_minimal_5+40_s0.25"]["stored"][True] == 40 - 1
    for name in ("zero_root_one_point", "zero_root_40_copies", "zero_root_one_finite_among_nans", "zero_root_second_copy_first"):
        om = irc.OracleMap(oracle, by[name]["min_extent"], True)
        for b in by[name]["batches"]:
            om.update(b)
        assert om.reinits == 1, name
    # a chain of `depth` splits: depth + 1 cubes from the root to the bottom leaf, whose half edge is R 2^-depth <= 2 min_extent
    for depth in (17, 18, 19, 24):
        for s in (0.2, 0.01):
            p, pin, R = irc._deep_points(depth, s, 7)
            two_min = float(np.float32(2) * np.float32(s))
            assert R * 2.0 ** -(depth - 1) > two_min >= R * 2.0 ** -depth
            assert len(p) == 7 * depth + 33


_CHILD = r'''
import os, resource, sys
sys.path.insert(0, os.environ["FLIMO_ROOT"])
sys.path.insert(0, os.path.join(os.environ["FLIMO_ROOT"], "tests"))
import numpy as np
import insert_rule_common as irc
from fast_limo_amd import _lib
_lib.load_hip()
lim = int(os.environ["FLIMO_CHILD_BYTES"])
resource.setrlimit(resource.RLIMIT_AS, (lim, lim))
out = {}
for case in irc.groups()[os.environ["FLIMO_GROUP"]]:
    for ds in (True, False):
        keep, stored = _lib.insert_rule_replay(case["batches"], case["min_extent"], ds)
        out["%s|%d|keep" % (case["name"], ds)] = np.concatenate(keep)
        out["%s|%d|stored" % (case["name"], ds)] = np.int64(stored)
np.savez(os.environ["FLIMO_CHILD_OUT"], **out)
print("CHILD_DONE")
'''


@pytest.mark.parametrize("group", CHILD_GROUPS)
def test_host_insert_rule_in_a_bounded_child(built, oracle, group, tmp_path):
    out_file = str(tmp_path / "keep.npz")
    env = dict(os.environ, FLIMO_ROOT=ROOT, FLIMO_GROUP=group, FLIMO_CHILD_OUT=out_file, FLIMO_CHILD_BYTES=str(CHILD_BYTES))
    run = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
    assert run.returncode == 0 and "CHILD_DONE" in run.stdout, (run.returncode, run.stderr[-2000:])
    got = np.load(out_file)
    for case in GROUPS[group]:
        for ds in (True, False):
            flat = got["%s|%d|keep" % (case["name"], ds)].astype(bool)
            keep, off = [], 0
            for b in case["batches"]:
                keep.append(flat[off:off + len(b)])
                off += len(b)
            _compare(case, ds, keep, int(got["%s|%d|stored" % (case["name"], ds)]), oracle)


def test_the_longest_root_growth_ends_like_the_oracles(built, oracle):
    """The growth loop is bounded at 300 doublings (flimo_insert.h kMaxRootDoublings) and refuses before it changes anything.  No
    finite float32 input gets there: from the smallest subnormal half edge, 2^-149, a root reaches any finite coordinate in at
    most 277.  The longest growth asked for here, about 250 doublings, ends and stores what the oracle stores."""
    from fast_limo_amd import _lib
    tiny = np.array([[0.0, 0.0, 0.0], [3e-45, 0.0, 0.0]], np.float32)            # two subnormal steps apart: half edge 2^-149
    assert tiny[1, 0] > 0 and np.float32(0.5) * tiny[1, 0] > 0
    far = np.array([[1.0e30, -3.0e29, 2.0e29]], np.float32)
    rng = np.random.default_rng(1)
    case = dict(name="longest_growth", batches=[tiny, far, irc.dense_over(rng, -4, 4, 500)], min_extent=0.25, stored=None)
    for ds in (True, False):
        keep, stored = _lib.insert_rule_replay(case["batches"], 0.25, ds)
        assert _compare(case, ds, keep, stored, oracle).reinits == 0
