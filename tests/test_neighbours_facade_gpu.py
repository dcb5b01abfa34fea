"""The C++ facade's SpatialHashGrid::findNeighbours on a real GPU: the test program of the facade (lattice known answers,
coincident and lone bodies, the refusals), and its lists and densities on one box bit for bit against the Python API."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "neighbours_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"^neighbours uniform (\d+) ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16})$", r.stdout, re.M)
    assert m, r.stdout
    # the same bodies through the Python API
    n = 2000
    h, d = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateHost(h, n)
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleInitializer.initUniform(h, nb.UniformDistParams((-5, -5, -5), (5, 5, 5)), 42)
    nb.ParticleDataManager.copyToDevice(d, h)
    grid = nb.SpatialHashGrid(n, 0.75, ctx)
    grid.build(d)
    res = grid.neighbours(8, lists=True, density=True)
    ctx.synchronize()

    def checksum(words):
        s = 0
        for w in words.tolist():
            s = (s * 1099511628211 + w) % 2 ** 64
        return s

    got = (int((res.status == 0).sum()), checksum(res.index.cpu().numpy().reshape(-1).view(np.uint32)),
           checksum(res.dist2.cpu().numpy().reshape(-1).view(np.uint32)), checksum(res.rho.cpu().numpy().view(np.uint64)))
    assert (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16)) == got
