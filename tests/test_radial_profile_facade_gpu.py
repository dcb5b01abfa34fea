"""The C++ facade's SpatialHashGrid::radialProfiles on a real GPU: the test program of the facade (lattice known answers in
the three modes, bad groups, error paths), and its structs on one catalogue byte for byte against the Python API."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "radial_profile_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"^radial profile uniform (\d+) ([0-9a-f]{16})$", r.stdout, re.M)
    assert m, r.stdout
    # the same bodies through the Python API
    n = 2000
    h, d = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateHost(h, n)
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleInitializer.initUniform(h, nb.UniformDistParams((-5, -5, -5), (5, 5, 5)), 42)
    f = np.float32
    h.vel_x[:], h.vel_y[:], h.vel_z[:] = f(0.5) * h.pos_y, f(-0.25) * h.pos_z, f(0.125) * h.pos_x
    nb.ParticleDataManager.copyToDevice(d, h)
    grid = nb.SpatialHashGrid(n, 0.75, ctx)
    grid.build(d)
    cat = grid.findGroups(0.6, 1)
    props = cat.properties(d, None, ctx)
    groups, shells = cat.radialProfile(d, props["com"].copy(), [0.25, 0.5, 0.75, 1.0], "mass", props["vel"].copy(), ctx=ctx)
    assert (groups["status"] == 0).all() and groups["n"].sum() == n
    by_grid = grid.groupRadialProfile(d, props["com"].copy(), [0.25, 0.5, 0.75, 1.0], "mass", props["vel"].copy())
    assert by_grid[0].tobytes() == groups.tobytes() and by_grid[1].tobytes() == shells.tobytes()
    checksum = 0
    for word in np.frombuffer(groups.tobytes() + shells.tobytes(), "<u8").tolist():
        checksum = (checksum * 1099511628211 + word) % 2 ** 64
    assert (int(m.group(1)), int(m.group(2), 16)) == (cat.n_groups, checksum)
