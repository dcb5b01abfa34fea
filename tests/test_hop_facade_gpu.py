"""The C++ facade's SpatialHashGrid::hopGroups on a real GPU: the test program of the facade (two clumps and a stray body,
the refusals, what every catalogue satisfies), and its catalogue on one box, array by array, against the Python API and
against the numpy restatement of tests/hop_ref.py on the lists that call produced."""
import os
import re
import subprocess

import numpy as np
import pytest

import hop_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checksum(words):
    s = 0
    for w in np.asarray(words, np.int32).reshape(-1).view(np.uint32).tolist():
        s = (s * 1099511628211 + w) % 2 ** 64
    return s


def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hop_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"^hop uniform ([0-9a-f]{16}) (\d+) (\d+) (\d+) (\d+)" + r" ([0-9a-f]{16})" * 5 + "$", r.stdout, re.M)
    assert m, r.stdout
    delta_outer = float(np.array([int(m.group(1), 16)], np.uint64).view(np.float64)[0])
    # the same bodies through the Python API
    n = 2000
    h, d = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateHost(h, n)
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleInitializer.initUniform(h, nb.UniformDistParams((-5, -5, -5), (5, 5, 5)), 42)
    nb.ParticleDataManager.copyToDevice(d, h)
    grid = nb.SpatialHashGrid(n, 0.75, ctx)
    grid.build(d)
    cat = grid.hopGroups(8, n_merge=4)  # delta_outer: the median, which the program took from the same densities
    ctx.synchronize()
    assert cat.delta_outer == delta_outer
    arrays = dict(labels=cat.labels.cpu().numpy(), peak=cat.peak.cpu().numpy(), offsets=cat.offsets.cpu().numpy(),
                  members=cat.members.cpu().numpy(), group_peak=cat.group_peak.cpu().numpy())
    want = ref.reference(cat.neighbours.index.cpu().numpy(), cat.neighbours.rho.cpu().numpy(), 8, 4, delta_outer)
    for key, a in arrays.items():
        assert np.array_equal(a, want[key]), key
    assert [int(m.group(i)) for i in (2, 3, 4, 5)] == [cat.n_groups, cat.n_members, cat.n_peaks, cat.rounds] == want["counts"][:4].tolist()
    got = [int(m.group(i), 16) for i in range(6, 11)]
    assert got == [_checksum(arrays[key]) for key in ("labels", "peak", "offsets", "members", "group_peak")]
    assert want["counts"][0] >= 2 and want["n_records"] > 0
