"""The C++ facade (compiled-language host side over the C ABI) on a real GPU:
  * n-body_amd/lib/facade_tests      the reference's hot-path gtest cases on a mini harness
  * oracle/_ref/example_*            the reference's OWN, unmodified example programs and
                                     ParticleSystem (compiled from /root/reference by
                                     oracle/Makefile.ref in the build container) linked against
                                     libnbody_facade.so -- the drop-in proof.  /root/reference is
                                     not read at run time; the binaries travel with the snapshot.
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "n-body_amd", "lib")
REF = os.path.join(ROOT, "oracle", "_ref")


def _run(exe, cwd, timeout=600):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIB + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)


def test_facade_reference_cases():
    exe = os.path.join(LIB, "facade_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    r = _run(exe, ROOT)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout


def _need(name):
    exe = os.path.join(REF, name)
    if not os.path.exists(exe):
        pytest.skip(f"{exe} not built (needs /root/reference at build time)")
    return exe


# examples/example_energy_conservation.cpp, unmodified: E0 ~ -0.25, "excellent" (< 0.1 %) drift
def test_reference_example_energy_conservation(tmp_path):
    r = _run(_need("example_energy_conservation"), str(tmp_path))
    out = r.stdout
    assert r.returncode == 0, out[-2000:] + r.stderr[-2000:]
    e0 = float(re.search(r"Initial Energy:\s+(-?[\d.eE+-]+)", out).group(1))
    drift = float(re.search(r"Max Drift:\s+([\d.eE+-]+)%", out).group(1))
    assert abs(e0 - (-0.25)) < 1e-3
    assert drift < 0.1 and "Excellent energy conservation" in out
    assert (tmp_path / "energy_data.csv").exists()


# examples/example_force_methods.cpp, unmodified: ParticleSystem::initialize / setForceMethod /
# getState / setState / update over all three strategies and four sizes
def test_reference_example_force_methods(tmp_path):
    r = _run(_need("example_force_methods"), str(tmp_path))
    out = r.stdout
    assert r.returncode == 0, out[-2000:] + r.stderr[-2000:]
    for name in ("Direct N", "Barnes-Hut", "Spatial Hash", "Performance Scaling", "20000"):
        assert name in out


# The reference's OWN CPU force loop (computeReferenceForces, examples/example_force_methods.cpp:34-67), compiled
# from /root/reference and run here: its forces equal the committed fixture (tests/golden/direct_refloop.npz, made
# by the same driver) and the oracle's mode 0 BIT FOR BIT, and the HIP Direct path agrees with it within the
# bound of an fp32 running sum over N terms (2e-5; the fp64-accumulated oracle is the 1e-5 bar elsewhere).
@pytest.mark.parametrize("name", ["plummer4096", "sphere3000"])
def test_reference_cpu_force_loop_pins_oracle_and_hip(tmp_path, name):
    import sys

    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_refloop_fixture as mk
    import nbody_amd as nb
    import oracle_bind
    from gpu_util import acc_of, rel_err, to_device
    _need("ref_force_loop_driver")
    fix = np.load(os.path.join(ROOT, "tests", "golden", "direct_refloop.npz"))
    ic, G, eps = next((ic, G, eps) for nm, ic, G, eps in mk.cases() if nm == name)
    live, log = mk.run_reference_loop(ic, G, eps, str(tmp_path))
    assert f"bodies {ic['pos_x'].size}" in log
    assert np.array_equal(live, fix[f"{name}_acc_refloop"])          # the committed fixture is what the reference computes
    o = oracle_bind.load()
    e32 = np.float32(eps)
    a0 = np.stack(o.direct_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], G, float(e32 * e32), 0), 1)
    assert np.array_equal(a0, live)                                   # oracle mode 0 == the reference's loop
    d, _ = to_device(nb, {k: np.ascontiguousarray(v, np.float32) for k, v in ic.items()})
    calc = nb.DirectForceCalculator()
    calc.setGravitationalConstant(G)
    calc.setSofteningParameter(eps)
    calc.computeForces(d)
    err = rel_err(acc_of(d), live)
    assert err.max() < 2e-5 and np.median(err) < 2e-6, err.max()


# A caller compiled against the REFERENCE's headers that constructs BarnesHutTree / SpatialHashGrid
# itself (as ref: tests/test_barnes_hut.cpp:29,54,118 and tests/test_spatial_hash.cpp:29,110 do) and
# a user ForceCalculator subclass through Integrator::integrate.  The _asan build has the driver AND
# the facade source instrumented: a facade method writing past the reference's 96 bytes aborts it.
@pytest.mark.parametrize("exe", ["ref_tree_grid_driver", "ref_tree_grid_driver_asan"])
def test_reference_header_caller_builds_tree_and_grid_itself(exe, tmp_path):
    path = _need(exe)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIB + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    # the HIP runtime keeps process-lifetime allocations: leak reports are not what is tested
    env["ASAN_OPTIONS"] = "detect_leaks=0:protect_shadow_gap=0:abort_on_error=0"
    r = subprocess.run([path], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout and "AddressSanitizer" not in r.stderr
    for case in ("tree_build_and_mass", "tree_convergence", "grid_build_and_cells", "plugin_contract"):
        assert f"PASS {case}" in r.stdout


# the multi-GPU code paths (process group, RCCL all-gather, barrier, all-reduce) with ONE rank
# under torch.distributed.run: everything except the cross-rank traffic itself
@pytest.mark.parametrize("workload,n", [("direct", 65536), ("hash", 131072), ("bh", 100000)])
def test_sharded_bench_rehearsal_one_rank(workload, n):
    import json
    import socket
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", "2", "--warmup", "1", "--force-sharded", "--full", "--no-cpu-baseline",
           "--workload", workload, "--bodies", str(n), "--kernel-iters", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout  # exactly one JSON line on stdout
    doc = json.loads(lines[0])
    assert doc["n_gpus"] == 1 and doc["value"] > 0 and doc["steps"] == 2
    if workload == "direct":
        assert doc["metric"] == "pair_interactions_per_s" and "roofline" in doc


# bench.py's safety net for the first real multi-rank run: when the C-ABI host's a(0) fails its self-check (injected
# here through the environment), every rank falls back to the torch.distributed host, the timed steps run there, and the
# record says so in config.path; the 180 s watchdog of the failed attempt is cancelled (it would end the run with rc 3)
def test_sharded_bench_falls_back_when_the_cabi_selfcheck_fails():
    import json
    import socket
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", "2", "--warmup", "1", "--force-sharded", "--no-cpu-baseline",
           "--workload", "direct", "--bodies", "65536", "--kernel-iters", "1"]
    docs = {}
    for inject in ("0", "1"):
        env = dict(os.environ, NBODY_BENCH_INJECT_SELFCHECK_FAILURE=inject)
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        docs[inject] = json.loads(lines[0])
    ok, fell = docs["0"]["config"]["path"], docs["1"]["config"]["path"]
    assert ok.startswith("C ABI (nbody_hip_sharded_direct_step)") and "max relative error" in ok
    assert fell.startswith("torch.distributed host") and "self-check of the sharded a(0) failed" in fell
    assert docs["1"]["value"] > 0 and docs["1"]["steps"] == 2


# the N-rank branches of bench.py (shard-pair roofline leg, rank-0-only JSON, max over ranks) with TWO
# ranks on the one test GPU: gloo transport, everything else as in the driver's N-GPU run
@pytest.mark.parametrize("workload,n", [("direct", 100000), ("hash", 200000), ("bh", 150000)])
def test_sharded_bench_rehearsal_two_ranks(workload, n):
    import json
    import socket
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--dist-backend", "gloo",
           "--one-device", "--workload", workload, "--bodies", str(n), "--kernel-iters", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    doc = json.loads(lines[0])
    assert doc["n_gpus"] == 2 and doc["value"] > 0 and doc["steps"] == 2
    if workload == "direct":
        assert doc["metric"] == "pair_interactions_per_s" and doc["scaling"] == "strong"
        assert "shard pair" in doc["roofline"]["kernel"] and doc["roofline"]["frac"] > 0


# a13 end to end: the REFERENCE's own ParticleSystem (its unmodified particle_system.cpp on the facade,
# oracle/ref_system_driver.cpp) against the Python ParticleSystem, same config, same steps; both write
# the reference's checkpoint format.  Uniform-box bodies are bit-identical on both sides (libstdc++
# stream restated in api.ParticleInitializer), so the whole trajectory must be; sphere / disk bodies
# go through cbrt / sin / cos / acos, where numpy and glibc may differ in the last ulp.
@pytest.mark.parametrize("method,dist,n,steps", [(0, 0, 3000, 5), (1, 0, 3000, 5), (2, 0, 3000, 5),
                                                 (1, 1, 2000, 3), (0, 2, 2000, 3), (0, 0, 40000, 2)])
def test_reference_particle_system_equals_python_system(tmp_path, method, dist, n, steps):
    import sys

    import numpy as np
    sys.path.insert(0, ROOT)
    import nbody_amd as nb
    exe = _need("ref_system_driver")
    out = tmp_path / "ref.nbody"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIB + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    dt = 0.001
    r = subprocess.run([exe, str(method), str(dist), str(n), str(steps), str(dt), str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = nb.Serializer.load(str(out))
    ps = nb.ParticleSystem()
    ps.initialize(nb.SimulationConfig(particle_count=n, force_method=nb.ForceMethod(method),
                                      init_distribution=nb.InitDistribution(dist), dt=dt))
    for _ in range(steps):
        ps.update(dt)
    mine = ps.getState()
    assert mine.particle_count == ref.particle_count == n
    assert abs(mine.simulation_time - ref.simulation_time) < 1e-9
    assert mine.force_method == ref.force_method
    assert np.float32(mine.G) == np.float32(ref.G) and np.float32(mine.softening) == np.float32(ref.softening)
    for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass"):
        a, b = getattr(mine, k), getattr(ref, k)
        if dist == 0:   # uniform box: identical bodies on both sides, and every force path is bitwise reproducible
            assert np.array_equal(a, b), k  # (the symmetric direct kernel too: deterministic slot sums, round 2)
        else:
            assert np.allclose(a, b, rtol=2e-5, atol=2e-5), k
    # the energies the reference program printed
    m = re.search(r"KE ([-0-9.e+]+) PE ([-0-9.e+]+)", r.stdout)
    ke, pe = float(m.group(1)), float(m.group(2))
    assert abs(ps.computeKineticEnergy() - ke) <= 1e-5 * abs(ke) + 1e-7
    assert abs(ps.computePotentialEnergy() - pe) <= 1e-5 * abs(pe)


# The setters mid-run (ref: particle_system.cpp:137-207), same cross-check: after half the steps the
# reference's ParticleSystem and the Python one get the same setter calls.  Pins in particular that
# setSpatialHashCellSize on a RUNNING spatial-hash system is a plain store (force_calculator.hpp:199:
# the grid that exists keeps the size it was constructed with), while a method switch creates a new
# calculator from the updated config.
@pytest.mark.parametrize("method,setters", [
    (2, ["cell=0.5"]), (2, ["cutoff=1.25", "cell=3"]), (2, ["G=2.5", "eps=0.05"]),
    (1, ["theta=0.9", "eps=0.2"]), (0, ["cell=0.5", "cutoff=1.0", "method=2"]), (2, ["theta=0.25", "method=1"]),
])
def test_reference_particle_system_setters_mid_run(tmp_path, method, setters):
    import sys

    import numpy as np
    sys.path.insert(0, ROOT)
    import nbody_amd as nb
    exe = _need("ref_system_driver")
    out = tmp_path / "ref.nbody"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIB + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    n, steps, dt = 3000, 6, 0.001
    r = subprocess.run([exe, str(method), "0", str(n), str(steps), str(dt), str(out)] + setters, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = nb.Serializer.load(str(out))
    ps = nb.ParticleSystem()
    ps.initialize(nb.SimulationConfig(particle_count=n, force_method=nb.ForceMethod(method),
                                      init_distribution=nb.InitDistribution.UNIFORM, dt=dt))
    apply = {"cell": ps.setSpatialHashCellSize, "cutoff": ps.setSpatialHashCutoff, "theta": ps.setBarnesHutTheta,
             "G": ps.setGravitationalConstant, "eps": ps.setSofteningParameter,
             "method": lambda v: ps.setForceMethod(nb.ForceMethod(int(v)))}
    for s in range(steps):
        if s == steps // 2:
            for kv in setters:
                k, v = kv.split("=")
                apply[k](float(np.float32(float(v))))
        ps.update(dt)
    mine = ps.getState()
    assert mine.force_method == ref.force_method
    assert np.float32(mine.G) == np.float32(ref.G) and np.float32(mine.softening) == np.float32(ref.softening)
    for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass"):
        assert np.array_equal(getattr(mine, k), getattr(ref, k)), k
