"""bench.py: the --dump-outputs writer, and a plain run end to end (its line, its outputs against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_bind import host_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    rng = np.random.default_rng(1)
    small = {k: rng.random(1000) for k in ("pos_x", "mass")}
    bench.dump_outputs(str(tmp_path / "whole"), small)
    for k, v in small.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))
    # over the budget: the same seeded rows of every array, in body order, the same from run to run
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4 * 100)
    big = {"a": np.arange(5000, dtype=np.float32), "b": -np.arange(5000, dtype=np.float32)}
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), big)
    a1, b1 = (np.load(tmp_path / "s1" / f"{k}.npy") for k in "ab")
    assert a1.size == 100 and np.array_equal(b1, -a1) and np.all(np.diff(a1) > 0)
    assert np.array_equal(a1, np.load(tmp_path / "s2" / "a.npy"))


@pytest.mark.gpu
def test_plain_bench_run_line_and_dumped_state(nb, oracle, tmp_path):
    n, steps, warmup = 4096, 2, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--bodies", str(n), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    doc = json.loads(lines[0])
    assert doc["metric"] == "pair_interactions_per_s" and doc["unit"] == "pair-interactions/s"
    assert doc["higher_is_better"] is True and doc["dtype"] == "f32"
    assert doc["steps"] == steps and doc["warmup"] == warmup and doc["ms_per_step"] > 0 and doc["value"] > 0
    assert not {"roofline", "cpu_baseline", "extra"} & doc.keys()  # measured with --full only
    got = {f: np.load(tmp_path / f"{f}.npy") for f in nb._lib.FIELDS}
    assert all(v.dtype == np.float32 and v.shape == (n,) and np.isfinite(v).all() for v in got.values())
    # bench.py's bodies and constants: a(0), then warmup + steps Velocity-Verlet steps on the oracle
    ic = nb.ic.plummer(n, seed=42)
    G, eps, dt = 1.0, 1e-3, 1e-3
    s = host_state(ic)
    a0 = oracle.direct_forces(s["pos_x"], s["pos_y"], s["pos_z"], s["mass"], G, float(np.float32(eps) ** 2), 1)
    s["acc_x"], s["acc_y"], s["acc_z"] = a0
    oracle.integrate_direct(s, G, eps, dt, warmup + steps, 1)
    assert np.array_equal(got["mass"], s["mass"])
    for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert np.allclose(got[k], s[k], rtol=1e-5, atol=1e-6), k
