"""CPU suite, part 2: the product's host-side logic (no GPU compute is called here).
  * libflimo_hip.so / libfast_limo.so load and export every symbol the headers declare
  * context creation fails loudly without a gfx950 device (no CPU fallback)
  * host IESKF (csrc/host/flimo_ikfom.cpp) == oracle on fixed measurements, both update branches
  * map insert rule (csrc/hip/flimo_insert.cpp) == oracle octree stored set
  * the N>1 bench plumbing (barrier + max over ranks) with world_size 2 on gloo
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from common import sort_rows
from fast_limo_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(flimo_[A-Za-z0-9_]+)\s*\(", txt)))


def test_c_abi_exports_every_declared_symbol(built):
    from fast_limo_amd import _lib, api
    L = _lib.load_hip()
    hip_decl = sorted(set(_declared("flimo_c.h") + _declared("flimo_dev.h")))     # the drop-in boundary + the developer instrumentation
    assert len(_declared("flimo_c.h")) >= 25
    for name in hip_decl:
        assert hasattr(L, name), name
    assert sorted(_lib.HIP_SYMBOLS) == hip_decl
    H = api.load_host()
    host_decl = [n for n in _declared("flimo_localizer_c.h") if n not in hip_decl]
    for name in host_decl:
        assert hasattr(H, name), name
    assert sorted(api.HOST_SYMBOLS) == sorted(host_decl)
    assert b"gfx950" in L.flimo_version()


# a process that sees no device: none on a CPU-only machine, and on a GPU machine the runtime is told to show it none (the check
# runs in a fresh child process: a HIP runtime already loaded in the test process keeps the devices it found)
_NO_DEVICE_ENV = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}

_NO_DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FLIMO_ROOT"])
from fast_limo_amd import _lib, api
for make in (lambda: _lib.HipCtx(0), lambda: api.Localizer(api.default_cfg())):
    try:
        make()
    except _lib.FlimoError:
        continue
    sys.exit("created without a device")
print("NO_DEVICE_RAISED")
'''


def test_no_device_fails_loudly(built):
    env = dict(os.environ, FLIMO_ROOT=ROOT, **_NO_DEVICE_ENV)
    out = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "NO_DEVICE_RAISED" in out.stdout


def test_host_ieskf_equals_oracle(built, oracle):
    from fast_limo_amd import api
    rs = np.random.RandomState(3)
    x0 = oracle.identity_x26(pos=(1, 2, 3))
    x0[3:7] = [0.01, -0.02, 0.03, 1.0]; x0[3:7] /= np.linalg.norm(x0[3:7])
    x0[7:11] = [0.0, 0.01, 0.0, 1.0]; x0[7:11] /= np.linalg.norm(x0[7:11])
    x0[14:17] = [0.1, 0.2, -0.1]
    P = np.eye(23); P[6:12, 6:12] *= 1e-6; P[21:, 21:] *= 1e-6
    for M in (500, 23, 22, 10, 1, 0):
        n = rs.normal(size=(M, 3))
        if M:
            n /= np.linalg.norm(n, axis=1, keepdims=True)
        H = np.hstack([n, rs.normal(size=(M, 3)) * 5, rs.normal(size=(M, 3)), n]) if M else np.zeros((0, 12))
        h = rs.normal(size=M) * 0.05
        xo, Po, no = oracle.eskf_update_fixed(x0, P, H, h)
        xp, Pp, npp = api.eskf_update_fixed(x0, P, H, h)
        assert no == npp
        np.testing.assert_allclose(xp, xo, rtol=0, atol=1e-13)
        np.testing.assert_allclose(Pp, Po, rtol=0, atol=1e-13)
    Q = [6e-4] * 3 + [1e-2] * 3 + [1e-5] * 3 + [3e-4] * 3
    xo, Po = oracle.eskf_predict(x0, P, 0.005, Q, [0.1, 0.2, 9.8], [0.01, -0.02, 0.03])
    xp, Pp = api.eskf_predict(x0, P, 0.005, Q, [0.1, 0.2, 9.8], [0.01, -0.02, 0.03])
    np.testing.assert_allclose(xp, xo, rtol=0, atol=1e-14)
    np.testing.assert_allclose(Pp, Po, rtol=0, atol=1e-14)
    assert np.abs(xo - x0).max() > 1e-4


def test_host_eigen_solver_and_degenerate_update_equal_oracle(built, oracle):
    """The host filter's restatement of Eigen::EigenSolver<Matrix6d> against the oracle's (two independent statements of the same
    published algorithm, compiled separately): eigenvalue order, eigenvector signs and values bit for bit; then whole updates on
    degenerate scenes (corridor, single plane, open field), where the row-zeroing projector makes that order observable."""
    from fast_limo_amd import api
    rs = np.random.RandomState(11)
    for trial in range(800):
        B = rs.randn(rs.randint(1, 30), 6) * rs.uniform(0.01, 50)
        if trial % 3 == 0:
            B[:, rs.choice(6, rs.randint(1, 6), replace=False)] *= 1e-5
        A = B.T @ B
        for a, b in zip(oracle.eigen_solver6(A), api.eigen_solver6(A)):
            np.testing.assert_array_equal(a, b)
    x0 = oracle.identity_x26(pos=(0.5, -0.2, 0.1))
    x0[3:7] = [0.01, -0.02, 0.03, 1.0]; x0[3:7] /= np.linalg.norm(x0[3:7])
    P = np.eye(23) * 1e-2
    for normals in ([(0, 1, 0), (0, -1, 0), (0, 0, 1)], [(0, 0, 1)], [(0, 0, 1), (0, 1, 0)], [(1, 0, 0), (0, 1, 0), (0, 0, 1)]):
        H = np.zeros((300, 12)); h = rs.normal(size=300) * 0.02
        for m in range(300):
            n = np.asarray(normals[m % len(normals)], float)
            p = rs.uniform(-5, 5, 3)
            H[m, 0:3] = n; H[m, 3:6] = np.cross(p, n); H[m, 9:12] = n
        xo, Po, no = oracle.eskf_update_fixed(x0, P, H, h)
        xp, Pp, npp = api.eskf_update_fixed(x0, P, H, h)
        assert no == npp
        np.testing.assert_allclose(xp, xo, rtol=0, atol=1e-12)
        np.testing.assert_allclose(Pp, Po, rtol=0, atol=1e-12)


def test_insert_rule_equals_oracle_octree(built, oracle):
    from fast_limo_amd import _lib
    b0 = synth.box_world_map(30000, 12.0, 1)
    batches = [b0, b0 + np.float32(0.003)]
    batches += [synth.box_world_map(6000, 12.0 + 4 * k, 10 + k) + np.float32([k * 2.5, -k, 0]) for k in range(3)]
    batches.append(np.array([[400.0, 3, 1], [-300.0, 2, 1]], np.float32))          # forces root growth
    for ds in (True, False):
        keep, stored = _lib.insert_rule_replay(batches, 0.2, ds)
        oc = oracle.Octree(0.2, ds)
        for b in batches:
            oc.update(b)
        assert stored == oc.size()
        kept = np.concatenate([b[k] for b, k in zip(batches, keep)])
        np.testing.assert_array_equal(sort_rows(kept), sort_rows(oc.points()))
        if ds:
            assert (~keep[1]).sum() > 1000           # the duplicate batch is largely dropped
        else:
            assert all(k.all() for k in keep)


_WORKER = r'''
import os, sys, time, json
sys.path.insert(0, os.environ["FLIMO_ROOT"])
import numpy as np
import torch, torch.distributed as dist
import bench                                    # the benchmark's own barrier / aggregation code
from fast_limo_amd import api                   # a real product call per "step": the host IESKF update (no GPU needed)
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group(backend=os.environ.get("FLIMO_BENCH_BACKEND", "gloo"), rank=rank, world_size=world)
rs = np.random.RandomState(rank)
H = rs.normal(size=(200, 12)); h = rs.normal(size=200) * 1e-3
x0 = np.zeros(26); x0[6] = 1; x0[10] = 1; x0[25] = -9.809
steps = 10
bench.rank_barrier(dist, torch)
t0 = time.perf_counter()
for _ in range(steps):
    api.eskf_update_fixed(x0, np.eye(23) * 1e-3, H, h)
time.sleep(0.05 * (rank + 1))                   # rank 1 is the slow one
bench.rank_barrier(dist, torch)
mine = time.perf_counter() - t0
elapsed, value = bench.aggregate(dist, torch, mine, world, steps)
if rank == 0:
    print(json.dumps({"value": value, "elapsed": elapsed, "mine": mine, "steps": steps, "world": world}))
dist.destroy_process_group()
'''


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_two_rank_gloo_runs_the_bench_protocol(built, tmp_path):
    """world_size-2 run on CPU (gloo) of bench.py's OWN barrier / max-over-ranks / aggregation helpers around real product calls:
    the slowest rank sets the time, the throughput is the scans of all ranks over that time (weak scaling, no data-path
    collective)."""
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    port = str(_free_port())
    env = dict(os.environ, FLIMO_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, FLIMO_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", port, str(script)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    r = json.loads(line)
    assert r["elapsed"] >= 0.099 and r["elapsed"] >= r["mine"] - 1e-9          # the max over the ranks (rank 1 slept 0.1 s)
    assert abs(r["value"] - r["world"] * r["steps"] / r["elapsed"]) < 1e-9


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_through_gloo(built):
    """The real bench.py under torch.distributed.run with two ranks (gloo for the barrier, both replicas on the one GPU of the box):
    the N > 1 launch path end to end -- one JSON line from rank 0, n_gpus = 2, weak scaling, two independent streams."""
    import json
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, FLIMO_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", port, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--steps", "4", "--warmup", "1", "--rings", "16", "--azimuths", "512", "--map-points", "100000",
                          "--box", "40", "--no-cpu-baseline", "--no-end-to-end"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                        # rank 0 only
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and r["steps"] == 4
    assert r["value"] > 0 and abs(r["value"] - 2 * 4 / (r["ms_per_step"] * 4e-3)) < 1e-6 * r["value"]


@pytest.mark.gpu
def test_bench_launches_its_own_ranks(built):
    """A bare `python bench.py --gpus 2` (no torch.distributed.run, no WORLD_SIZE): bench.py starts the two ranks itself, before
    anything touches the GPU in the parent, and rank 0 reports n_gpus = 2."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--rings", "16",
                          "--azimuths", "512", "--map-points", "100000", "--box", "40", "--no-cpu-baseline", "--no-end-to-end"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and r["steps"] == 4
    assert r["value"] > 0 and abs(r["value"] - 2 * 4 / (r["ms_per_step"] * 4e-3)) < 1e-6 * r["value"]


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_steps_outputs(built, tmp_path):
    """A plain single-GPU run (no --full): the result line carries the headline figures and none of the --full legs, and
    --dump-outputs writes the last timed step's state as float64 .npy files; two runs with the same arguments agree."""
    import json
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rings", "16",
           "--azimuths", "512", "--map-points", "100000", "--box", "40"]
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = subprocess.run(cmd + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        r = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in r, key
        assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "scans/s" and r["higher_is_better"] is True
        assert r["value"] > 0 and abs(r["value"] - 3 / (r["ms_per_step"] * 3e-3)) < 1e-6 * r["value"]
        for key in ("roofline", "cpu_baseline", "end_to_end", "update_layouts", "with_map_insert", "concurrent_streams"):
            assert key not in r, key
        arrs = {n: np.load(str(d / (n + ".npy"))) for n in ("state_x", "state_P", "pose_cov")}
        assert arrs["state_x"].shape == (26,) and arrs["state_P"].shape == (23, 23) and arrs["pose_cov"].shape == (6, 6)
        assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in arrs.values())
        runs.append(arrs)
    for n in runs[0]:
        assert np.allclose(runs[0][n], runs[1][n], rtol=1e-6, atol=1e-8), n


def test_bench_self_launch_fails_loudly_without_a_gpu(built):
    """No visible device (a CPU container, or the devices hidden from the run): the same command starts its ranks, they meet
    through gloo, and the run ends with a non-zero status and no JSON line because there is no gfx950 device (no CPU fallback
    anywhere on the product path)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(_NO_DEVICE_ENV)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--rings", "8",
                          "--azimuths", "64", "--map-points", "2000", "--box", "10", "--no-cpu-baseline", "--no-end-to-end"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert "no gfx950 device" in out.stderr


def test_bench_cli_contract():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in src
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"ms_per_step"', '"higher_is_better"', '"scaling"',
                '"vs_baseline"', '"dtype"', '"data"', '"config"', '"roofline"', '"cpu_baseline"'):
        assert key in src, key
    # the product path never imports the oracle: only the cpu_baseline leg does
    prod = ""
    for dp, _, fs in os.walk(os.path.join(ROOT, "fast_limo_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                prod += open(os.path.join(dp, f)).read()
    assert "oracle_py" not in prod and "rl_octree" not in prod and "liboracle" not in prod


def test_pcd_and_imu_csv_round_trip(tmp_path):
    """Replay harness formats: PCD ascii / binary with each per-point time field, IMU CSV."""
    from fast_limo_amd import replay
    rs = np.random.RandomState(0)
    xyz = rs.uniform(-5, 5, (257, 3)).astype(np.float32)
    inten = rs.uniform(0, 255, 257).astype(np.float32)
    for field, vals in (("time", rs.uniform(0, 0.1, 257).astype(np.float32)), ("t", rs.randint(0, 10**8, 257).astype(np.uint32)),
                        ("timestamp", 1.7e9 + rs.uniform(0, 0.1, 257))):
        for binary in (True, False):
            f = str(tmp_path / f"s_{field}_{int(binary)}.pcd")
            replay.write_pcd(f, xyz, inten, field, vals, binary=binary)
            p = replay.read_pcd(f)
            assert p.dtype.itemsize == 32 and p.shape[0] == 257
            np.testing.assert_array_equal(np.stack([p["x"], p["y"], p["z"]], 1), xyz)
            np.testing.assert_array_equal(p["intensity"], inten)
            raw = p.view(np.uint8).reshape(-1, 32)
            width = {"time": 4, "t": 4, "timestamp": 8}[field]
            got = raw[:, 24:24 + width].copy().view({"time": np.float32, "t": np.uint32, "timestamp": np.float64}[field]).ravel()
            np.testing.assert_array_equal(got, vals)
    st = np.arange(50) * 0.01
    w = rs.normal(0, 0.1, (50, 3)).astype(np.float32); a = rs.normal(0, 1, (50, 3)).astype(np.float32)
    f = str(tmp_path / "imu.csv")
    replay.write_imu_csv(f, st, w, a)
    st2, w2, a2 = replay.read_imu_csv(f)
    np.testing.assert_allclose(st2, st, atol=1e-9); np.testing.assert_array_equal(w2, w); np.testing.assert_array_equal(a2, a)


def test_host_plane_object_equals_oracle(built, oracle):
    """fast_limo::Plane / Match of the host C++ mirror (the object API of reference Objects/Plane.hpp, Match.hpp) evaluate
    the fit kernel's own routines on the host: normals, gates and Match::dist must equal the oracle's bit for bit."""
    import ctypes as C
    from fast_limo_amd import api
    L = api.load_host()
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    L.flimo_host_plane.restype = C.c_int
    L.flimo_host_plane.argtypes = [f32p, f32p, C.c_int, C.c_int, C.c_double, C.c_double, f32p, f32p, C.POINTER(C.c_float)]
    rs = np.random.RandomState(8)
    n_good = 0
    for trial in range(400):
        nrm = rs.normal(size=3); nrm /= np.linalg.norm(nrm)
        base = rs.uniform(-20, 20, 3)
        u = np.cross(nrm, [1, 0, 0]); u /= np.linalg.norm(u); v = np.cross(nrm, u)
        spread = rs.choice([0.2, 0.6, 1.5])
        noise = rs.choice([0.0, 0.005, 0.08])
        pts = (base + rs.uniform(-spread, spread, (5, 1)) * u + rs.uniform(-spread, spread, (5, 1)) * v
               + rs.normal(0, noise, (5, 1)) * nrm).astype(np.float32)
        q = (base + rs.normal(0, 0.05, 3)).astype(np.float32)
        sqd = np.sort(((pts - q) ** 2).sum(1).astype(np.float32))
        n_o, ok_o = oracle.plane_fit(pts, sqd)
        n_h = np.zeros(4, np.float32); dist = C.c_float(0.0)
        ok_h = L.flimo_host_plane(pts, sqd, 5, 5, 2.0, 0.05, q, n_h, C.byref(dist))
        assert bool(ok_h) == bool(ok_o), trial
        if ok_o:
            n_good += 1
            np.testing.assert_array_equal(n_h, n_o)
            expect = np.float32(np.float32(np.float32(np.float32(n_o[0] * q[0]) + np.float32(n_o[1] * q[1])) + np.float32(n_o[2] * q[2])) + n_o[3])
            assert dist.value == expect
    assert 100 < n_good < 400                     # both outcomes of the gates were exercised
    # fewer than NUM_MATCH_POINTS neighbours / 5th squared distance beyond MAX_DIST_PLANE: not a plane
    n_h = np.zeros(4, np.float32)
    assert L.flimo_host_plane(pts[:4].copy(), sqd[:4].copy(), 4, 5, 2.0, 0.05, q, n_h, None) == 0
    far = sqd.copy(); far[4] = 2.5
    assert L.flimo_host_plane(pts, far, 5, 5, 2.0, 0.05, q, n_h, None) == 0


def test_host_state_update_equals_oracle(built, oracle):
    """fast_limo::State::update of the host mirror (const-omega / const-accel propagation, State.cpp:76-119) against the
    oracle restatement: bit-identical p, q, v over random states, including the |w| <= 1e-7 branch."""
    import ctypes as C
    from fast_limo_amd import api
    L = api.load_host()
    L.flimo_host_state_update.restype = None
    L.flimo_host_state_update.argtypes = [np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"), C.c_double, C.c_double]
    rs = np.random.RandomState(12)
    for k in range(300):
        s = np.zeros(25, np.float32)
        s[0:3] = rs.uniform(-50, 50, 3)
        q = rs.normal(size=4); s[3:7] = q / np.linalg.norm(q)
        s[7:10] = rs.uniform(-15, 15, 3)
        s[10:13] = [0, 0, -9.809]
        s[13:16] = rs.uniform(-2, 2, 3) if k % 7 else 0.0
        s[16:19] = rs.uniform(-12, 12, 3)
        s[19:22] = rs.normal(0, 0.01, 3); s[22:25] = rs.normal(0, 0.05, 3)
        if k % 7 == 0:
            s[19:22] = 0.0
        t0 = rs.uniform(0, 100); t1 = t0 + rs.uniform(1e-4, 0.02)
        a = s.copy()
        L.flimo_host_state_update(a, t0, t1)
        b = oracle.state_update(s, t0, t1)
        np.testing.assert_array_equal(a, b, err_msg=str(k))
        assert not np.array_equal(a[0:3], s[0:3])


def test_time_order_equals_library_call(built):
    """The host's heap-order restatement leaves a sweep in exactly the order std::partial_sort_copy does (reference
    Localizer.cpp:789-790), ties included: every key type, both directions, odd and even sizes, heavy / adjacent /
    scattered ties, signed zeros, already ordered and reversed input."""
    import ctypes as C, time
    from fast_limo_amd import api
    L = api.load_host()
    L.flimo_host_time_order.restype = C.c_int
    L.flimo_host_time_order.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_void_p]

    def order(keys, kind, desc, lib):
        out = np.empty(keys.size, np.uint32)
        assert L.flimo_host_time_order(keys.ctypes.data, kind, keys.size, desc, lib, out.ctypes.data) == 0
        return out

    rs = np.random.RandomState(5)
    kinds = [(0, np.uint32), (1, np.float32), (2, np.float64)]
    cases = 0
    for n in [0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 100, 101, 1000, 1023, 1024, 1025, 4097, 20000]:
        for kind, dt in kinds:
            variants = []
            variants.append(rs.randint(0, max(1, n // 8) + 1, n))                       # heavy scattered ties
            variants.append(np.repeat(np.arange((n + 15) // 16), 16)[:n])               # columns: adjacent ties, ascending
            variants.append(np.tile(np.arange((n + 15) // 16), 16)[:n])                 # ring-major: ties far apart
            variants.append(np.arange(n))                                               # strictly ascending
            variants.append(np.arange(n)[::-1].copy())                                  # strictly descending
            variants.append(rs.permutation(n))                                          # unique, shuffled
            variants.append(np.zeros(n))                                                # all equal
            for v in variants:
                if dt == np.uint32:
                    keys = v.astype(np.uint32)
                else:
                    keys = (v.astype(np.float64) * 1e-3 - (0.004 if kind == 1 else 0.0)).astype(dt)   # some negative
                    if n > 4:
                        keys[rs.randint(n)] = -0.0; keys[rs.randint(n)] = 0.0
                for desc in ([0, 1] if kind < 2 else [0]):
                    a = order(keys, kind, desc, 0); b = order(keys, kind, desc, 1)
                    np.testing.assert_array_equal(a, b, err_msg=f"n={n} kind={kind} desc={desc}")
                    if n:
                        k = keys[a].astype(np.float64)
                        assert np.all(np.diff(k) <= 0) if desc else np.all(np.diff(k) >= 0)
                    cases += 1
    assert cases > 500
    # NaN stamps: not a strict weak order, the library call itself runs -- same answer by construction, and no crash
    keys = rs.uniform(0, 0.1, 1000).astype(np.float32); keys[::37] = np.nan
    np.testing.assert_array_equal(order(keys, 1, 0, 0), order(keys, 1, 0, 1))
    # and it is the faster of the two on a sweep-sized cloud with column ties
    keys = np.repeat(np.arange(1024), 64).astype(np.float32) * 1e-4
    t0 = time.perf_counter(); a = order(keys, 1, 0, 0); t1 = time.perf_counter(); b = order(keys, 1, 0, 1); t2 = time.perf_counter()
    np.testing.assert_array_equal(a, b)
    print(f"time order 64k with ties: restatement {1e3 * (t1 - t0):.2f} ms, library {1e3 * (t2 - t1):.2f} ms")


def test_kitti_raw_readers(tmp_path):
    """The replay harness reads the layout of a KITTI raw recording (BASELINE.json config 3): Velodyne `.bin` sweeps (per-point time
    synthesised from the azimuth), `timestamps.txt`, OXTS packets -> the arrays `replay` feeds to a Localizer."""
    from fast_limo_amd import replay
    rs = np.random.RandomState(4)
    vel = tmp_path / "velodyne_points" / "data"; vel.mkdir(parents=True)
    n = 1000
    az = -np.linspace(0.0, 2 * np.pi, n, endpoint=False) + 0.3          # clockwise from 0.3 rad
    rng = rs.uniform(5, 40, n)
    pts = np.stack([rng * np.cos(az), rng * np.sin(az), rs.uniform(-2, 1, n), rs.uniform(0, 1, n)], 1).astype(np.float32)
    pts.tofile(str(vel / "0000000000.bin"))
    p = replay.read_kitti_bin(str(vel / "0000000000.bin"), sweep_s=0.1)
    assert p.dtype.itemsize == 32 and p.shape == (n,)
    np.testing.assert_array_equal(np.stack([p["x"], p["y"], p["z"], p["intensity"]], 1), pts)
    t = (p["tu"] & 0xffffffff).astype(np.uint32).view(np.float32)
    assert t[0] == 0.0 and np.all(np.diff(t) > 0) and abs(t[-1] - 0.1 * (n - 1) / n) < 1e-6
    ox = tmp_path / "oxts"; (ox / "data").mkdir(parents=True)
    stamps = ["2011-09-26 13:02:25.964389445", "2011-09-26 13:02:25.974389445", "2011-09-26 13:02:26.004389445",
              "2011-09-27 00:00:00.004389445"]
    (ox / "timestamps.txt").write_text("\n".join(stamps) + "\n")
    vals = rs.uniform(-1, 1, (4, 30))
    for k in range(4):
        (ox / "data" / ("%010d.txt" % k)).write_text(" ".join(repr(float(v)) for v in vals[k]) + "\n")
    st, w, a = replay.read_kitti_oxts(str(ox))
    np.testing.assert_allclose(st[:3], [0.0, 0.01, 0.04], atol=1e-9)
    assert abs(st[3] - (10 * 3600 + 57 * 60 + 34.04)) < 1e-6                      # across midnight
    np.testing.assert_array_equal(w, vals[:, 17:20].astype(np.float32))
    np.testing.assert_array_equal(a, vals[:, 11:14].astype(np.float32))

    class Rec:                                                                    # replay() drives anything Localizer-shaped
        def __init__(self): self.imu, self.scans = [], []
        def update_imu(self, s, w_, a_): self.imu.append(s)
        def update_pointcloud_points(self, pts_, stamp): self.scans.append((len(pts_), stamp, len(self.imu))); return 0
        def get_x(self): return np.zeros(26)
    r = Rec()
    rcs, poses = replay.replay(r, str(vel), (st, w, a), scan_stamps=[0.0])
    assert rcs == [0] and r.scans == [(n, 0.0, 3)] and poses.shape == (1, 26)


def test_default_gain_against_80_bit_arithmetic(built):
    """The gain of esekfom.hpp:1722-1729.  The reference evaluates  P_inv = ((P/R)^-1 + E H^T H E^T)^-1  with two
    general 23 x 23 inverses.  The product's default takes the same formula through the block-inverse identity
    P_inv E = [I; A21 A11^-1] (A11^-1 + H^T H)^-1  (one 12 x 12 system; what the device filter can solve between a pass's sums and
    the step).  Ground truth: the literal formula in 80-bit extended precision.  On the measured states the default is as close to it as
    the literal float64 form (FLIMO_REFERENCE_SOLVE=1) -- 1e-16 of a 3e-2 m step.  (Rounds 1-3 used A[:, 0:12] (I + H^T H A11)^-1, whose
    identity drowns in H^T H A11 ~ 1e7: 1e-13 here, three digits worse than the reference's own form -- replaced in round 4.)"""
    from fast_limo_amd import api
    rs = np.random.RandomState(5)
    worse = 0
    for trial in range(8):
        # a covariance like the filter's after a few predictions: the initial block scales (Localizer.cpp:672-694) mixed by a rotation-like noise
        d = np.array([1.0] * 6 + [1e-6] * 6 + [1.0] * 3 + [1e-5] * 3 + [1e-4] * 3 + [1e-6] * 2)
        Q = np.linalg.qr(np.eye(23) + 0.05 * rs.randn(23, 23))[0]
        P = (Q * d) @ Q.T
        P = 0.5 * (P + P.T)
        M = 4000
        H = np.zeros((M, 12))
        nrm = rs.randn(M, 3); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        H[:, 0:3] = nrm
        H[:, 3:12] = 8.0 * rs.randn(M, 9)
        h = 0.02 * rs.randn(M) + 0.03 * nrm[:, 0]
        x0 = np.zeros(26); x0[6] = 1.0; x0[10] = 1.0; x0[25] = -9.809
        R = 0.001
        out = {}
        for name, env in (("default", None), ("literal", "1")):
            old = os.environ.pop("FLIMO_REFERENCE_SOLVE", None)
            if env:
                os.environ["FLIMO_REFERENCE_SOLVE"] = env
            try:
                x1, _, _ = api.eskf_update_fixed(x0, P, H, h, max_iters=0, R=R)
            finally:
                os.environ.pop("FLIMO_REFERENCE_SOLVE", None)
                if old is not None:
                    os.environ["FLIMO_REFERENCE_SOLVE"] = old
            out[name] = x1[0:3] - x0[0:3]                       # the position block of the step (boxplus adds it)
        # ground truth: the literal formula in extended precision (Gauss-Jordan with partial pivoting on long doubles)
        LD = np.longdouble
        def inv_ld(A):
            n = A.shape[0]
            A = A.astype(LD).copy(); X = np.eye(n, dtype=LD)
            for k in range(n):
                p = k + int(np.argmax(np.abs(A[k:, k])))
                if p != k:
                    A[[k, p]] = A[[p, k]]; X[[k, p]] = X[[p, k]]
                piv = A[k, k]
                A[k] /= piv; X[k] /= piv
                for r in range(n):
                    if r != k:
                        f = A[r, k]
                        A[r] -= f * A[k]; X[r] -= f * X[k]
            return X
        HTH = H.astype(LD).T @ H.astype(LD)
        HTh = H.astype(LD).T @ h.astype(LD)
        Pt = inv_ld(P.astype(LD) / LD(R))
        Pt[:12, :12] += HTH
        Pinv = inv_ld(Pt)
        truth = np.asarray((Pinv[:, :12] @ HTh)[0:3], dtype=np.float64)
        e_def = float(np.abs(out["default"] - truth).max())
        e_lit = float(np.abs(out["literal"] - truth).max())
        print(f"trial {trial}: |step| {np.abs(truth).max():.3e}  error vs 80-bit: default (block-inverse form) {e_def:.2e}, literal two-inverse {e_lit:.2e}")
        assert e_def < 1e-14 and e_lit < 1e-14
        if e_def > 3.0 * e_lit + 2e-16:
            worse += 1
    assert worse <= 1, worse                                     # (as close as the literal form, trial after trial)
