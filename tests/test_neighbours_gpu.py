"""The k nearest neighbours, the local density and the density centre (include/nbody_hip_neighbours.h) on a real GPU.
Every list comparison is np.array_equal against the CPU restatement of tests/neighbours_ref.py, which orders the same
keys (bits of the fp32 fma chain, body index) over the cell ids the grid itself assigned; rho and the density centre are
compared bit for bit too (fp64, in the stated order)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import neighbours_ref as ref

pytestmark = pytest.mark.gpu


def _device(nb, pos, mass=None):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    d, h = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.allocateHost(h, n)
    h.pos_x[:], h.pos_y[:], h.pos_z[:] = pos[:, 0], pos[:, 1], pos[:, 2]
    h.mass[:] = 1.0 if mass is None else mass
    nb.ParticleDataManager.copyToDevice(d, h)
    return d


def _grid(nb, ctx, pos, cell, mass=None):
    d = _device(nb, pos, mass)
    grid = nb.SpatialHashGrid(d.count, float(cell), ctx)
    grid.build(d)
    return grid, d


def _host(ctx, res):
    ctx.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (res.index, res.dist2, res.rho, res.status))


def _want(grid, pos, mass, k, cell):
    _, _, cells, _ = grid.copyCellDataToHost()
    n = len(np.asarray(pos).reshape(-1, 3))
    m = np.full(n, 1.0, np.float32) if mass is None else np.asarray(mass, np.float32)
    return ref.search(pos, m, k, np.float32(cell), cells, grid.getGridDims())


def _same(got, want):
    names = ("index", "dist2", "rho", "status")
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.float64 and got[3].dtype == np.int32
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())


def _check(nb, ctx, pos, cell, ks, mass=None):
    """build, search with all outputs for every k, compare with the restatement; -> ({k: host arrays}, grid)"""
    grid, _ = _grid(nb, ctx, pos, cell, mass)
    out = {}
    for k in ks:
        got = _host(ctx, grid.neighbours(k, lists=True, density=True))
        _same(got, _want(grid, pos, mass, k, cell))
        out[k] = got
    return out, grid


# ---- 1. the smallest systems -------------------------------------------------------------------------------------------
def test_smallest_systems(nb, ctx):
    got, _ = _check(nb, ctx, [[0.25, 0.5, -1.0]], 1.0, (1, 3))
    index, dist2, rho, status = got[3]
    assert status.tolist() == [2] and index.tolist() == [[-1] * 3] and np.isposinf(dist2).all() and rho.tolist() == [0.0]
    got, _ = _check(nb, ctx, [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], 1.0, (1,))
    index, dist2, rho, status = got[1]
    assert index.tolist() == [[1], [0]] and dist2.tolist() == [[0.25], [0.25]] and status.tolist() == [0, 0]
    assert rho.tolist() == [0.0, 0.0]  # k = 1: no mass inside the first neighbour
    got, _ = _check(nb, ctx, [[1.5, -2.0, 0.25], [1.5, -2.0, 0.25]], 1.0, (1,))
    index, dist2, rho, status = got[1]
    assert index.tolist() == [[1], [0]] and dist2.tolist() == [[0.0], [0.0]] and status.tolist() == [3, 3]
    assert rho.tolist() == [0.0, 0.0]
    pos = np.random.default_rng(1).random((5, 3)).astype(np.float32)
    got, _ = _check(nb, ctx, pos, 1.0, (32, 4, 5))
    index, dist2, rho, status = got[32]
    assert status.tolist() == [2] * 5 and (index[:, :4] >= 0).all() and (index[:, 4:] == -1).all()
    assert np.isposinf(dist2[:, 4:]).all() and np.isfinite(dist2[:, :4]).all() and not rho.any()
    assert got[4][3].tolist() == [0] * 5 and got[5][3].tolist() == [2] * 5


# ---- 2. the integer lattice: massive ties ------------------------------------------------------------------------------
LATTICE = np.array([[x, y, z] for z in range(5) for y in range(5) for x in range(5)], np.float32)


@pytest.mark.parametrize("masses", ["unit", "random"])
def test_integer_lattice_resolves_its_ties_by_index(nb, ctx, masses):
    mass = None if masses == "unit" else np.random.default_rng(2).uniform(0.5, 2.0, 125).astype(np.float32)
    got, _ = _check(nb, ctx, LATTICE, 1.5, (1, 6, 7, 26, 32), mass)
    centre = 2 + 5 * 2 + 25 * 2
    index, dist2, _, status = got[26]
    # the centre body: 6 faces at d2 = 1, 12 edges at 2, 8 corners at 3, each run ascending by index
    assert dist2[centre].tolist() == [1.0] * 6 + [2.0] * 12 + [3.0] * 8
    for run in (index[centre, :6], index[centre, 6:18], index[centre, 18:]):
        assert (np.diff(run) > 0).all()
    assert got[6][0][centre].tolist() == sorted(centre + s * o for o in (1, 5, 25) for s in (-1, 1))
    assert got[7][0][centre, 6] == centre - 25 - 5  # the first edge neighbour: the lowest index at d2 = 2


# ---- 3. the status edge -------------------------------------------------------------------------------------------------
def test_status_edge_at_the_cell_size(nb, ctx):
    interior = np.array([i for i, p in enumerate(LATTICE) if ((p >= 1) & (p <= 3)).all()])
    one = np.float32(1.0)
    got, grid = _check(nb, ctx, LATTICE, one, (6,))
    assert grid.getGridDims() == (6, 6, 6)
    index, dist2, rho, status = got[6]
    assert (dist2[interior] == 1.0).all() and (status[interior] == 1).all()  # d2_k = 1 is not below fl(1 * 1)
    above = np.nextafter(one, np.float32(2.0))
    got, _ = _check(nb, ctx, LATTICE, above, (6,))
    assert (got[6][1][interior] == 1.0).all() and (got[6][3][interior] == 0).all()
    assert np.array_equal(got[6][0][interior], index[interior]) and np.array_equal(got[6][2][interior], rho[interior])
    assert (rho[interior] == 5.0 / ref.SPHERE).all()  # flagged, but computed from what the window holds


# ---- 4. the 26 window directions ---------------------------------------------------------------------------------------
def test_one_neighbour_across_every_window_direction(nb, ctx):
    b = 1.0
    dirs = [(sx, sy, sz) for sz in (-1, 0, 1) for sy in (-1, 0, 1) for sx in (-1, 0, 1) if (sx, sy, sz) != (0, 0, 0)]
    pos = [[0.001, 0.001, 0.001]]  # the anchor: the box starts at 0 (to a rounding), so cell faces lie on the integers
    for p, s in enumerate(dirs):
        s = np.array(s, np.float64)
        centre = np.array([4 + 5 * (p % 3), 4 + 5 * ((p // 3) % 3), 4 + 5 * (p // 9)], np.float64) + 0.5 * (s == 0)
        u = s / np.linalg.norm(s)
        pos += [centre - 0.45 * b * u, centre + 0.45 * b * u]
    pos = np.array(pos, np.float32)
    got, grid = _check(nb, ctx, pos, 1.0, (1, 2))
    assert grid.copyCellStartArray() is not None
    _, _, cells, _ = grid.copyCellDataToHost()
    xyz = ref.cell_xyz(cells, grid.getGridDims())
    assert [tuple(v) for v in (xyz[2::2] - xyz[1::2]).tolist()] == dirs  # each pair straddles its face, edge or corner
    index, dist2, _, status = got[1]
    want = np.arange(len(pos))
    want[1::2], want[2::2] = np.arange(2, len(pos), 2), np.arange(1, len(pos), 2)
    want[0] = -1
    assert index[:, 0].tolist() == want.tolist()
    assert status.tolist() == [2] + [0] * 52 and (dist2[1:, 0] < 0.82).all()
    assert got[2][3].tolist() == [2] * 53 and got[2][0][:, 0].tolist() == want.tolist()


# ---- 5. a neighbour two cells away: refinement on a coarser build ----------------------------------------------------------
def test_refinement_resolves_a_body_whose_neighbours_are_two_cells_away(nb, ctx):
    rng = np.random.default_rng(5)
    x = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.55, 0.6])
    cluster = np.stack([x, 0.2 * rng.random(8), 0.2 * rng.random(8)], 1)
    pos = np.concatenate([cluster, [[2.05, 0.1, 0.1]]]).astype(np.float32)
    mass = rng.uniform(0.5, 2.0, 9).astype(np.float32)
    d = _device(nb, pos, mass)
    grid = nb.SpatialHashGrid(9, 1.0, ctx)
    grid.build(d)
    res = grid.neighbours(2, lists=True, density=True)
    first = _host(ctx, res)
    _same(first, _want(grid, pos, mass, 2, 1.0))
    assert first[3].tolist() == [0] * 8 + [2] and first[0][8].tolist() == [-1, -1]  # its window is empty
    res.index[:8], res.dist2[:8], res.rho[:8] = -7, -1.0, -5.0  # poison in the rows that are exact
    grid.setCellSize(2.0)
    grid.build(d)
    assert max(grid.getGridDims()) > 2
    again = grid.neighbours(2, lists=True, density=True, out=res)
    assert again is res
    index, dist2, rho, status = _host(ctx, res)
    assert (index[:8] == -7).all() and (dist2[:8] == -1.0).all() and (rho[:8] == -5.0).all()  # skipped: nothing written
    assert status.tolist() == [0] * 9
    want = ref.topk(pos, 2, rows=[8])
    assert index[8].tolist() == want[0][0].tolist() == [7, 6] and np.array_equal(dist2[8], want[1][0])
    full = _want(grid, pos, mass, 2, 2.0)
    assert rho[8] == full[2][8] and rho[8] > 0
    # a status tensor alone: fresh tensors, the skipped rows hold -1 / +inf / 0
    st = torch.tensor([0] * 8 + [2], dtype=torch.int32, device=res.status.device)
    fresh = _host(ctx, grid.neighbours(2, lists=True, density=True, status=st))
    assert (fresh[0][:8] == -1).all() and np.isposinf(fresh[1][:8]).all() and not fresh[2][:8].any()
    assert fresh[0][8].tolist() == [7, 6] and fresh[3].tolist() == [0] * 9


# ---- 6. the list lengths ---------------------------------------------------------------------------------------------------
def test_every_k_is_a_prefix_of_k_32(nb, ctx):
    pos = np.random.default_rng(6).random((2000, 3)).astype(np.float32)
    mass = np.random.default_rng(7).uniform(0.5, 2.0, 2000).astype(np.float32)
    got, _ = _check(nb, ctx, pos, 0.2, (32, 4, 5, 8, 9, 16, 17), mass)
    for k in (4, 5, 8, 9, 16, 17):
        assert np.array_equal(got[k][0], got[32][0][:, :k]) and np.array_equal(got[k][1], got[32][1][:, :k])
    assert {0, 1} <= set(got[32][3].tolist())


# ---- 7. crowded and sparse ---------------------------------------------------------------------------------------------
def test_crowded_cell_among_a_sparse_rest(nb, ctx):
    rng = np.random.default_rng(8)
    v = rng.normal(size=(300, 3))
    v *= (0.2 * rng.random(300) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    pos = np.concatenate([np.array([0.5, 0.5, 0.5]) + v, 6.0 * rng.random((200, 3))]).astype(np.float32)
    pos = pos[rng.permutation(500)]
    mass = rng.uniform(0.5, 2.0, 500).astype(np.float32)
    got, grid = _check(nb, ctx, pos, 1.0, (6, 32), mass)
    assert np.bincount(grid.copyCellDataToHost()[2]).max() >= 300
    assert {0, 1, 2} <= set(got[32][3].tolist())


def test_filament_on_a_grid_without_start_array(nb, ctx):
    b, n = 1.0, 1000
    u = np.array([3.0, 2.0, 1.0]) / np.sqrt(14.0)
    line = (np.arange(n)[:, None] * (0.9 * b) * u[None, :]).astype(np.float32)
    pos = line[np.random.default_rng(11).permutation(n)]
    got, grid = _check(nb, ctx, pos, 3.0 * b, (2, 6))
    assert grid.getTotalCells() > 1000000 and grid.copyCellStartArray() is None  # the binary search in the sorted keys
    # 0.9 b, 1.8 b, 2.7 b on both sides: exact inside the line; near its ends the sixth neighbour is beyond 3 b
    assert (got[2][3] == 0).all() and (got[6][3] == 0).sum() >= 990 and (got[6][3] != 0).sum() >= 2


# ---- 8. reproducibility -------------------------------------------------------------------------------------------------
def test_two_calls_and_a_permuted_body_order(nb, ctx):
    pos = np.random.default_rng(9).random((3000, 3)).astype(np.float32)
    grid, _ = _grid(nb, ctx, pos, 0.15)
    a = grid.neighbours(8, lists=True, density=True)
    c = grid.neighbours(8, lists=True, density=True)
    ctx.synchronize()
    for x, y in ((a.index, c.index), (a.dist2, c.dist2), (a.rho, c.rho), (a.status, c.status)):
        assert torch.equal(x, y)
    perm = np.random.default_rng(10).permutation(3000)
    grid2, _ = _grid(nb, ctx, pos[perm], 0.15)
    p = _host(ctx, grid2.neighbours(8, lists=True, density=True))
    o = _host(ctx, a)
    assert np.array_equal(p[1], o[1][perm]) and np.array_equal(p[3], o[3][perm]) and np.array_equal(p[2], o[2][perm])
    untied = (np.diff(o[1], axis=1) > 0).all(1)[perm]  # without equal distances the bodies are the same ones too
    assert untied.sum() > 2900 and np.array_equal(perm[p[0][untied]], o[0][perm][untied])


# ---- 9. the grid is left alone; refusals ---------------------------------------------------------------------------------
def test_grid_is_left_alone_and_refusals_touch_nothing(nb, ctx):
    lib, check = ctx._lib, nb._lib.check
    S, V = nb.StateException, nb.ValidationException
    pos = np.random.default_rng(12).random((5000, 3)).astype(np.float32)
    cell = 0.1
    d = _device(nb, pos)
    grid = nb.SpatialHashGrid(d.count, cell, ctx)
    with pytest.raises(S, match="null grid"):
        check(lib.nbody_hip_grid_neighbours(None, 6, 0, None, None, None, None))
    with pytest.raises(S, match="not been built"):
        grid.neighbours(6)
    grid.build(d)

    def forces():
        grid.computeForces(d, cell, 1.0, 0.01)
        ctx.synchronize()
        return np.stack([d.acc_x.cpu().numpy(), d.acc_y.cpu().numpy(), d.acc_z.cpu().numpy()])

    before = forces()
    cat = grid.findGroups(0.05, 2)
    acc_old = d.acc_x.clone()
    res = grid.neighbours(6, lists=True, density=True)
    first = _host(ctx, res)
    assert torch.equal(d.acc_x, acc_old)  # no acc_* is written
    offsets, members = torch.empty_like(cat.offsets), torch.empty_like(cat.members)
    check(lib.nbody_hip_grid_groups_copy(grid._h, offsets.data_ptr(), members.data_ptr()))  # the catalogue survives
    ctx.synchronize()
    assert torch.equal(offsets, cat.offsets) and torch.equal(members, cat.members) and cat.n_groups > 0
    assert np.array_equal(before.view(np.uint32), forces().view(np.uint32))
    # the refusals, each with every output given: nothing is written
    p = [t.data_ptr() for t in (res.index, res.dist2, res.rho, res.status)]
    for k in (0, -1, 33):
        with pytest.raises(V, match="k must lie in 1 .. 32"):
            check(lib.nbody_hip_grid_neighbours(grid._h, k, 0, *p))
    with pytest.raises(V, match="every output is NULL"):
        check(lib.nbody_hip_grid_neighbours(grid._h, 6, 0, None, None, None, None))
    with pytest.raises(V, match="status_dev may not be NULL"):
        check(lib.nbody_hip_grid_neighbours(grid._h, 6, 1, p[0], p[1], p[2], None))
    check(lib.nbody_hip_grid_set_slab(grid._h, 0, 2))
    with pytest.raises(S, match="slab"):
        check(lib.nbody_hip_grid_neighbours(grid._h, 6, 0, *p))
    check(lib.nbody_hip_grid_set_slab(grid._h, 0, 0))
    with pytest.raises(V):
        grid.neighbours(6, status=torch.zeros(5000, dtype=torch.int64, device="cuda"))
    with pytest.raises(V):
        grid.neighbours(2.5)
    _same(_host(ctx, res), first)
    check(lib.nbody_hip_grid_groups_copy(grid._h, None, None))
    # each output alone, and the density-only form: the same values
    rho_only = grid.localDensity(6)
    assert rho_only.index is None and rho_only.dist2 is None
    ctx.synchronize()
    assert torch.equal(rho_only.rho, res.rho) and torch.equal(rho_only.status, res.status)
    lists_only = grid.neighbours(6)
    assert lists_only.rho is None
    ctx.synchronize()
    assert torch.equal(lists_only.index, res.index) and torch.equal(lists_only.dist2, res.dist2)
    only = torch.full_like(res.dist2, -1.0)
    check(lib.nbody_hip_grid_neighbours(grid._h, 6, 0, None, only.data_ptr(), None, None))
    ctx.synchronize()
    assert torch.equal(only, res.dist2)
    _same(first, _want(grid, pos, None, 6, cell))


def test_calculator_builds_its_own_grid(nb, ctx):
    pos = np.random.default_rng(13).random((1500, 3)).astype(np.float32)
    d = _device(nb, pos)
    calc = nb.SpatialHashCalculator(cell_size=0.2, cutoff_radius=0.2, ctx=ctx)
    got = _host(ctx, calc.neighbours(d, 5, lists=True, density=True))
    _same(got, _want(calc.getGrid(), pos, None, 5, 0.2))


# ---- 10. the density against an independent fp64 route ---------------------------------------------------------------------
def test_density_against_a_kd_tree_in_fp64(nb, ctx):
    """4,096 equal-mass uniform bodies, the status-0 bodies: rho within 1e-6 (relative) of msum / (4 pi / 3 r_k^3) with
    r_k from scipy's kd-tree on the widened coordinates.  The bound is derived: d2 carries at most 5 u relative error
    (u = 2^-24: three differences, their squares, the chain), rho ~ d2^-1.5 turns that into 7.5 u = 4.5e-7; a near-tie
    swap of the k-th neighbour moves r_k by no more; equal masses keep msum exact.  1e-6 leaves a factor 2."""
    n, k = 4096, 6
    pos = np.random.default_rng(14).random((n, 3)).astype(np.float32)
    m = np.float32(1.0 / n)
    grid, _ = _grid(nb, ctx, pos, 0.15, np.full(n, m, np.float32))
    _, _, rho, status = _host(ctx, grid.neighbours(k, lists=True, density=True))
    dist, _ = cKDTree(pos.astype(np.float64)).query(pos.astype(np.float64), k + 1)
    want = (k - 1) * float(m) / (4.0 * np.pi / 3.0 * dist[:, k] ** 3)
    exact = status == 0
    assert exact.sum() > n // 2
    rel = np.abs(rho[exact] - want[exact]) / want[exact]
    print("density vs kd-tree: max relative difference", rel.max(), "over", int(exact.sum()), "bodies")
    assert rel.max() <= 1e-6


# ---- 11. the density centre ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_set():
    return ref.seeded_set(70000)


def _centre_same(got, want):
    assert got.dtype == ref.DTYPE
    for name in ref.DTYPE.names:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])


@pytest.mark.parametrize("n", [1, 32, 33, 1024, 1025, 65537])
def test_density_centre_in_all_three_summation_regimes(nb, ctx, n):
    rho, pos = _big_set()
    # all bodies of a particle set of n (members NULL)
    d = _device(nb, pos[:n])
    w = torch.from_numpy(rho[:n].copy()).cuda()
    got = nb.density_centre(ctx, d, w)
    want = ref.density_centre(pos[:n], rho[:n])
    _centre_same(got, want)
    assert got["n"] == n and got["status"] == 0 and got["core_radius"] > 0 or n == 1
    # an index list into the larger set, as a device tensor and as a host array
    big = _device(nb, pos)
    wb = torch.from_numpy(rho).cuda()
    members = np.random.default_rng(n).permutation(70000)[:n].astype(np.int32)
    want = ref.density_centre(pos, rho, members)
    _centre_same(nb.density_centre(ctx, big, wb, torch.from_numpy(members).cuda()), want)
    _centre_same(nb.density_centre(ctx, big, wb, members), want)
    # a bad index: status 1 and zeros
    for bad in (70000, -1):
        broken = members.copy()
        broken[n // 2] = bad
        got = nb.density_centre(ctx, big, wb, broken)
        assert got["status"] == 1 and got["n"] == 0 and not got["centre"].any() and got["core_radius"] == 0
        assert got["rho_sum"] == 0 and got["rho2_sum"] == 0
        _centre_same(got, ref.density_centre(pos, rho, broken))
    # ... and the next good call is not affected by it
    _centre_same(nb.density_centre(ctx, big, wb, members), want)


def test_density_centre_without_weight_and_errors(nb, ctx):
    rho, pos = _big_set()
    d = _device(nb, pos[:100])
    zero = torch.zeros(100, dtype=torch.float64, device="cuda")
    for members in (None, np.arange(40, dtype=np.int32)):
        got = nb.density_centre(ctx, d, zero, members)
        _centre_same(got, ref.density_centre(pos[:100], np.zeros(100), members))
        assert got["n"] == (100 if members is None else 40) and got["status"] == 0 and got["rho_sum"] == 0
    got = nb.density_centre(ctx, d, zero, np.zeros(0, np.int32))
    assert got["n"] == 0 and got["status"] == 0
    with pytest.raises(nb.ValidationException):
        nb.density_centre(ctx, d, zero.float())
    with pytest.raises(nb.ValidationException):
        nb.density_centre(ctx, d, zero[:50])
    lib, check = ctx._lib, nb._lib.check
    s = d.struct()
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(nb.StateException, match="null context"):
        check(lib.nbody_hip_density_centre(None, C.byref(s), zero.data_ptr(), None, 0, out.data_ptr()))
    with pytest.raises(nb.StateException, match="null rho"):
        check(lib.nbody_hip_density_centre(ctx.handle, C.byref(s), None, None, 0, out.data_ptr()))
    with pytest.raises(nb.StateException, match="null output"):
        check(lib.nbody_hip_density_centre(ctx.handle, C.byref(s), zero.data_ptr(), None, 0, None))
    with pytest.raises(nb.ValidationException, match="n_members"):
        check(lib.nbody_hip_density_centre(ctx.handle, C.byref(s), zero.data_ptr(), zero.data_ptr(), -1, out.data_ptr()))


# ---- 12. ParticleSystem.localDensity on a Plummer sphere ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plummer(nb):
    ic = {k: np.asarray(v, np.float32).copy() for k, v in nb.ic.plummer(4096, seed=17).items()}
    for key, shift in (("pos_x", 3.0), ("pos_y", -2.0), ("pos_z", 1.0)):
        ic[key] = (ic[key] + np.float32(shift)).astype(np.float32)
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)
    index, dist2 = ref.topk(pos, 6)  # unrestricted brute force
    status = np.zeros(4096, np.int32)
    return ic, pos, index, dist2, ref.density_of(index, dist2, status, ic["mass"])


@pytest.mark.parametrize("method", ["DIRECT_N2", "BARNES_HUT", "SPATIAL_HASH"])
def test_particle_system_resolves_a_plummer_sphere_by_levels(nb, ctx, method):
    ic, pos, index, dist2, rho = _plummer(nb)
    ps = nb.ParticleSystem()
    ps.initialize(nb.SimulationConfig(particle_count=4096, force_method=getattr(nb.ForceMethod, method)), ic)
    acc = ps.d_particles_.acc_x.clone()
    res = ps.localDensity(6)
    got = _host(ctx, res)
    assert (got[3] == 0).all()
    assert np.array_equal(got[0], index) and np.array_equal(got[1], dist2) and np.array_equal(got[2], rho)
    level = res.level.cpu().numpy()
    assert res.levels >= 2 and level.max() == res.levels - 1 and len(np.unique(level)) >= 2
    grid = ps.neighbour_grid_
    assert res.cells[0] == nb.ParticleSystem.neighbourCellSize(pos.min(0), pos.max(0), 4096)
    assert grid.getCellSize() == res.cells[-1] == res.cells[0] * 2 ** (res.levels - 1)
    centre = ps.densityCentre(6)
    _centre_same(centre, ref.density_centre(pos, got[2]))
    assert np.abs(centre["centre"] - np.array([3.0, -2.0, 1.0])).max() < 0.2 and 0.1 < centre["core_radius"] < 1.0
    sub = np.arange(100, 900, dtype=np.int32)
    _centre_same(ps.densityCentre(6, members=sub), ref.density_centre(pos, got[2], sub))
    assert torch.equal(ps.d_particles_.acc_x, acc)
    ps.update(ps.getTimeStep())  # the force calculator goes on as before
