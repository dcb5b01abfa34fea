"""Friends-of-friends groups on the spatial-hash grid (nbody_hip_grid_groups, include/nbody_hip_groups.h) on a real GPU.
Every case compares labels, offsets and members EXACTLY with the CPU restatement of tests/groups_ref.py, which takes
bit-identical pair decisions (fp32 fma chain < fl(b * b)) on the cell ids the grid itself assigned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import groups_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(nb, pos, mass=None, vel=None):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    d, h = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.allocateHost(h, n)
    h.pos_x[:], h.pos_y[:], h.pos_z[:] = pos[:, 0], pos[:, 1], pos[:, 2]
    h.mass[:] = 1.0 if mass is None else mass
    if vel is not None:
        h.vel_x[:], h.vel_y[:], h.vel_z[:] = vel[:, 0], vel[:, 1], vel[:, 2]
    nb.ParticleDataManager.copyToDevice(d, h)
    return d


def _grid(nb, ctx, pos, cell):
    d = _device(nb, pos)
    grid = nb.SpatialHashGrid(d.count, float(cell), ctx)
    grid.build(d)
    return grid, d


def _reference(grid, pos, b):
    _, _, cells, _ = grid.copyCellDataToHost()
    return groups_ref.fof_labels(np.asarray(pos, np.float32).reshape(-1, 3), b, cells, grid.getGridDims())


def _same(cat, labels, min_members):
    offsets, members = groups_ref.catalogue(labels, min_members)
    got = cat.labels.cpu().numpy(), cat.offsets.cpu().numpy(), cat.members.cpu().numpy()
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert np.array_equal(got[0], labels), "labels"
    assert np.array_equal(got[1], offsets), "offsets"
    assert np.array_equal(got[2], members), "members"
    assert cat.n_groups == len(offsets) - 1 and cat.n_members == len(members)
    assert np.array_equal(cat.sizes().cpu().numpy(), np.diff(offsets))


def _check(nb, ctx, pos, cell, b, min_members=(1,)):
    """build, find, compare with the restatement; returns (labels, grid)"""
    grid, _ = _grid(nb, ctx, pos, cell)
    labels = _reference(grid, pos, b)
    for m in min_members:
        _same(grid.findGroups(float(b), m), labels, m)
    return labels, grid


# ---- 1. the smallest systems -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos, want", [
    ([[0.0, 0.0, 0.0]], [0]),
    ([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], [0, 0]),
    ([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0]], [0, 1]),
    ([[1.5, -2.0, 0.25], [1.5, -2.0, 0.25]], [0, 0]),  # coincident bodies are linked, whatever eps would say
], ids=["one", "two_linked", "two_apart", "two_coincident"])
def test_smallest_systems(nb, ctx, pos, want):
    labels, _ = _check(nb, ctx, pos, 1.0, 1.0, (1, 2))
    assert labels.tolist() == want


# ---- 2. the exact edge ----------------------------------------------------------------------------------------------
def test_exact_edge_on_an_integer_lattice(nb, ctx):
    pos = np.array([[x, y, z] for z in range(5) for y in range(5) for x in range(5)], np.float32)
    grid, _ = _grid(nb, ctx, pos, 1.5)
    one = np.float32(1.0)
    for b, groups in ((one, 125), (np.nextafter(one, np.float32(2.0)), 1), (np.float32(1.5), 1)):
        labels = _reference(grid, pos, b)
        assert len(np.unique(labels)) == groups  # d2 = 1 is not below 1; the next float above links the faces
        _same(grid.findGroups(float(b), 1), labels, 1)
    # b = 1.5: fl(b * b) = 2.25 links face (d2 = 1) and edge (d2 = 2) neighbours, not the corner ones (d2 = 3)
    i, j = groups_ref.linked_pairs(pos, np.float32(1.5))
    d2 = ((pos[i] - pos[j]) ** 2).sum(1)
    assert set(d2.tolist()) == {1.0, 2.0} and len(i) == 3 * 100 + 6 * 80


# ---- 3. the 26 window directions ---------------------------------------------------------------------------------------
def test_one_pair_across_every_window_direction(nb, ctx):
    b = 1.0
    dirs = [(sx, sy, sz) for sz in (-1, 0, 1) for sy in (-1, 0, 1) for sx in (-1, 0, 1) if (sx, sy, sz) != (0, 0, 0)]
    pos = [[0.001, 0.001, 0.001]]  # the anchor: the box starts at 0 (to a rounding), so cell faces lie on the integers
    for p, s in enumerate(dirs):
        s = np.array(s, np.float64)
        centre = np.array([4 + 5 * (p % 3), 4 + 5 * ((p // 3) % 3), 4 + 5 * (p // 9)], np.float64) + 0.5 * (s == 0)
        u = s / np.linalg.norm(s)
        pos += [centre - 0.45 * b * u, centre + 0.45 * b * u]
    pos = np.array(pos, np.float32)
    grid, _ = _grid(nb, ctx, pos, 1.0)
    assert grid.copyCellStartArray() is not None
    _, _, cells, _ = grid.copyCellDataToHost()
    gx, gy, _ = grid.getGridDims()
    xyz = np.stack([cells % gx, (cells // gx) % gy, cells // (gx * gy)], 1)
    assert [tuple(v) for v in (xyz[2::2] - xyz[1::2]).tolist()] == dirs  # each pair straddles its face, edge or corner
    labels = _reference(grid, pos, b)
    want = np.arange(len(pos), dtype=np.int32)
    want[2::2] = want[1::2]
    assert np.array_equal(labels, want)
    _same(grid.findGroups(b, 1), labels, 1)
    cat = grid.findGroups(b, 2)
    _same(cat, labels, 2)
    assert cat.n_groups == 26 and cat.sizes().cpu().tolist() == [2] * 26


# ---- 4. a filament ------------------------------------------------------------------------------------------------------
def test_filament_through_many_cells(nb, ctx):
    b, n = 1.0, 1000
    u = np.array([3.0, 2.0, 1.0]) / np.sqrt(14.0)
    line = (np.arange(n)[:, None] * (0.9 * b) * u[None, :]).astype(np.float32)
    order = np.random.default_rng(11).permutation(n)
    pos = line[order]
    labels, grid = _check(nb, ctx, pos, 3.0 * b, b)
    assert (labels == 0).all()
    assert grid.getTotalCells() > 1000000
    cut = np.delete(pos, 500, 0)  # the body at one place of the chain: a gap of 1.8 b
    labels, _ = _check(nb, ctx, cut, 3.0 * b, b)
    assert len(np.unique(labels)) == 2 and np.bincount(labels).max() < n - 1


# ---- 5. crowded cells ---------------------------------------------------------------------------------------------------
def test_crowded_cells(nb, ctx):
    rng = np.random.default_rng(5)

    def ball(centre, radius, count):
        v = rng.normal(size=(count, 3))
        v *= (radius * rng.random(count) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
        return (np.asarray(centre) + v).astype(np.float32)

    pos = ball([0.5, 0.5, 0.5], 0.2, 300)
    labels, grid = _check(nb, ctx, pos, 1.0, 1.0, (1, 300, 301))
    assert (labels == 0).all() and len(set(grid.copyCellDataToHost()[2].tolist())) == 1
    pos = np.concatenate([ball([0.2, 0.2, 0.2], 0.05, 150), ball([0.7, 0.2, 0.2], 0.05, 150)])
    pos = pos[rng.permutation(300)]
    labels, grid = _check(nb, ctx, pos, 1.0, 0.25, (1, 150, 151))
    assert len(set(grid.copyCellDataToHost()[2].tolist())) == 1  # two balls in ONE cell of 4 b, more than b apart
    assert len(np.unique(labels)) == 2 and np.bincount(labels).max() == 150


# ---- 6. a sparse grid: no start array, the binary search ----------------------------------------------------------------
def test_sparse_grid_takes_the_binary_search(nb, ctx):
    rng = np.random.default_rng(6)
    corners = np.array([[x, y, z] for x in (0, 100) for y in (0, 100) for z in (0, 100)], np.float64)
    pos = (np.repeat(corners, 8, 0) + 0.3 * rng.random((64, 3))).astype(np.float32)
    pos = pos[rng.permutation(64)]
    labels, grid = _check(nb, ctx, pos, 1.0, 1.0, (1, 8, 9))
    assert grid.getTotalCells() > 16 * 64 + 4096 and grid.copyCellStartArray() is None
    assert len(np.unique(labels)) == 8 and (np.bincount(labels)[np.unique(labels)] == 8).all()


# ---- 7. the random box --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac, groups, largest", [(0.2, 19660, 3), (0.6, 12179, 18), (0.9, 2109, 12155)])
def test_random_box(nb, ctx, frac, groups, largest):
    pos, spacing = groups_ref.uniform_box()
    b = np.float32(frac * spacing)
    seen = []
    for factor in (1.0, 1.7, 4.0):
        labels, grid = _check(nb, ctx, pos, np.float32(b * np.float32(factor)), b, (1, 8))
        seen.append(labels)
    assert len(np.unique(seen[0])) == groups and np.bincount(seen[0]).max() == largest
    # (on this input the cell restriction drops no link: tests/test_groups_cpu.py confirms it on the CPU)
    assert np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])


# ---- 8. determinism -----------------------------------------------------------------------------------------------------
def test_determinism_and_the_force_call_is_left_alone(nb, ctx):
    pos, spacing = groups_ref.uniform_box()
    b = np.float32(0.9 * spacing)
    cell = float(np.float32(b * np.float32(1.7)))
    d = _device(nb, pos)
    grid = nb.SpatialHashGrid(d.count, cell, ctx)
    grid.build(d)

    def forces():
        grid.computeForces(d, cell, 1.0, 0.01)
        ctx.synchronize()
        return np.stack([d.acc_x.cpu().numpy(), d.acc_y.cpu().numpy(), d.acc_z.cpu().numpy()])

    before = forces()
    acc_old = d.acc_x.clone()
    a = grid.findGroups(float(b), 2)
    assert torch.equal(d.acc_x, acc_old)  # no acc_* is written
    c = grid.findGroups(float(b), 2)
    for x, y in ((a.labels, c.labels), (a.offsets, c.offsets), (a.members, c.members)):
        assert torch.equal(x, y)
    after = forces()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    labels = a.labels.cpu().numpy()
    # the same bodies in another order: the same partition (each new group's lowest OLD index is the old label)
    perm = np.random.default_rng(8).permutation(len(pos))
    grid2, _ = _grid(nb, ctx, pos[perm], cell)
    new = grid2.findGroups(float(b), 1).labels.cpu().numpy()
    lowest = np.full(len(pos), len(pos), np.int64)
    np.minimum.at(lowest, new, perm)
    assert np.array_equal(lowest[new], labels[perm])


# ---- 9. entry points and bridges ----------------------------------------------------------------------------------------
def test_drift_build_and_packed_build(nb, ctx):
    pos, spacing = groups_ref.uniform_box(5000, 9)
    b = np.float32(0.7 / 5000 ** (1 / 3))
    cell = float(np.float32(b * np.float32(1.3)))
    vel = np.random.default_rng(10).normal(size=(5000, 3)).astype(np.float32)
    d = _device(nb, pos, vel=vel)
    grid = nb.SpatialHashGrid(d.count, cell, ctx)
    grid.driftBuild(d, 0.003)
    drifted = np.stack([d.pos_x.cpu().numpy(), d.pos_y.cpu().numpy(), d.pos_z.cpu().numpy()], 1)
    assert not np.array_equal(drifted, pos)
    labels = _reference(grid, drifted, b)
    _same(grid.findGroups(float(b), 3), labels, 3)
    # the packed build (no slab): float4 bodies on the device
    posm = torch.from_numpy(np.concatenate([pos, np.ones((5000, 1), np.float32)], 1)).cuda().contiguous()
    lib = ctx._lib
    nb._lib.check(lib.nbody_hip_grid_build_packed(grid._h, posm.data_ptr(), 5000, None))
    with pytest.raises(nb.StateException):  # the catalogue of the earlier build is gone
        nb._lib.check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    labels = _reference(grid, pos, b)
    _same(grid.findGroups(float(b), 1), labels, 1)


def test_systems_bridge_into_the_diagnostics(nb, ctx):
    pos, spacing = groups_ref.uniform_box()
    b = np.float32(0.6 * spacing)
    mass = np.random.default_rng(12).uniform(0.5, 2.0, len(pos)).astype(np.float32)
    d = _device(nb, pos, mass=mass)
    grid = nb.SpatialHashGrid(d.count, float(b), ctx)
    grid.build(d)
    cat = grid.findGroups(float(b), 2)
    members, offsets = cat.members.cpu().numpy(), cat.offsets.cpu().numpy()
    sub, off = cat.systems(d)
    assert sub.count == cat.n_members and off.dtype == torch.int64 and off.cpu().tolist() == offsets.tolist()
    assert np.array_equal(sub.pos_y.cpu().numpy(), pos[members, 1]) and np.array_equal(sub.mass.cpu().numpy(), mass[members])
    diag = nb.systems_diagnostics(ctx, sub, off, 1.0, 0.01)
    assert len(diag) == cat.n_groups and (diag["status"] == 0).all()
    assert np.array_equal(diag["n"], np.diff(offsets))
    want = np.add.reduceat(mass[members].astype(np.float64), offsets[:-1])
    assert np.allclose(diag["mass"], want, rtol=1e-14, atol=0.0)  # an fp64 sum of at most 18 fp32 masses, in another order


@pytest.mark.parametrize("method", ["DIRECT_N2", "BARNES_HUT"])
def test_particle_system_under_every_force_method(nb, ctx, method):
    n = 3000
    pos, _ = groups_ref.uniform_box(n, 13)
    b = float(np.float32(0.8 / n ** (1 / 3)))
    ic = {"pos_x": pos[:, 0], "pos_y": pos[:, 1], "pos_z": pos[:, 2], "mass": np.full(n, 1.0 / n, np.float32)}
    ps = nb.ParticleSystem()
    ps.initialize(nb.SimulationConfig(particle_count=n, force_method=getattr(nb.ForceMethod, method)), ic)
    acc = ps.d_particles_.acc_x.clone()
    cat = ps.findGroups(b, 2)
    grid = ps.group_grid_
    assert grid.copyCellStartArray() is not None  # the private grid follows the density rule
    cell = grid.getCellSize()
    assert cell == nb.ParticleSystem.groupCellSize(pos.min(0), pos.max(0), n, b) and cell >= b
    _same(cat, _reference(grid, pos, b), 2)
    assert np.array_equal(cat.labels.cpu().numpy(), groups_ref.fof_labels(pos, b))  # plain friends-of-friends
    assert torch.equal(ps.d_particles_.acc_x, acc)
    ps.update(ps.getTimeStep())  # the force calculator goes on as before


def test_calculator_builds_its_own_grid(nb, ctx):
    pos, spacing = groups_ref.uniform_box(4000, 14)
    b = float(np.float32(0.8 / 4000 ** (1 / 3)))
    d = _device(nb, pos)
    calc = nb.SpatialHashCalculator(cell_size=2 * b, cutoff_radius=2 * b, ctx=ctx)
    cat = calc.findGroups(d, b, 1)
    _same(cat, _reference(calc.getGrid(), pos, b), 1)
    with pytest.raises(nb.ValidationException, match="setCellSize"):
        calc.findGroups(d, 3 * b)


def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "groups_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"^groups uniform (\d+) (\d+) (\d+) ([0-9a-f]{16})$", r.stdout, re.M)
    assert m, r.stdout
    h = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(h, 2000)
    nb.ParticleInitializer.initUniform(h, nb.UniformDistParams((-5, -5, -5), (5, 5, 5)), 42)
    pos = np.stack([h.pos_x, h.pos_y, h.pos_z], 1)
    grid, _ = _grid(nb, ctx, pos, 0.75)
    cat = grid.findGroups(0.6, 2)
    _same(cat, _reference(grid, pos, 0.6), 2)
    checksum = 0
    for label in cat.labels.cpu().tolist():
        checksum = (checksum * 1099511628211 + label) % 2 ** 64
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4), 16)) == (
        cat.n_groups, cat.n_members, int(cat.sizes().max()), checksum)


# ---- 10. errors ---------------------------------------------------------------------------------------------------------
def test_errors(nb, ctx):
    lib, check = ctx._lib, nb._lib.check
    counts = (C.c_longlong * 2)()
    S, V = nb.StateException, nb.ValidationException
    with pytest.raises(S, match="null grid"):
        check(lib.nbody_hip_grid_groups(None, 1.0, 1, None, C.byref(counts)))
    with pytest.raises(S, match="null grid"):
        check(lib.nbody_hip_grid_groups_copy(None, None, None))
    pos, _ = groups_ref.uniform_box(500, 15)
    d = _device(nb, pos)
    grid = nb.SpatialHashGrid(500, 0.25, ctx)
    with pytest.raises(S, match="not been built"):
        grid.findGroups(0.1)
    with pytest.raises(S, match="no group catalogue"):
        check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    grid.build(d)
    with pytest.raises(S, match="no group catalogue"):  # built, but no search yet
        check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(V, match="positive and finite"):
            grid.findGroups(bad)
    with pytest.raises(V, match=r"0\.3.*0\.25"):  # both values are named
        grid.findGroups(0.3)
    for bad in (0, -3):
        with pytest.raises(V, match="min_members"):
            grid.findGroups(0.1, bad)
    with pytest.raises(V, match="counts_host"):
        check(lib.nbody_hip_grid_groups(grid._h, 0.1, 1, None, None))
    with pytest.raises(S):  # not capturable
        with ctx.capture():
            grid.findGroups(0.1)
    # labels may be NULL; a refused call touches nothing; the catalogue lives until the next build
    check(lib.nbody_hip_grid_groups(grid._h, 0.1, 1, None, C.byref(counts)))
    assert counts[1] == 500 and 1 <= counts[0] <= 500
    check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    with pytest.raises(V):
        grid.findGroups(0.3)
    check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    grid.build(d)
    with pytest.raises(S, match="no group catalogue"):
        check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    # a slab set: single-GPU grids only
    check(lib.nbody_hip_grid_set_slab(grid._h, 0, 2))
    with pytest.raises(S, match="slab"):
        grid.findGroups(0.1)
    check(lib.nbody_hip_grid_set_slab(grid._h, 0, 0))
    _same(grid.findGroups(0.1), _reference(grid, pos, 0.1), 1)
