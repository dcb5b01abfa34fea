"""What the spatial-hash force kernels READ, word by word: the start array d_cell_lb of its three builders (cell_mark +
cell_gap by sorted position, the two-level search, the gallop of NBH_HASH_LB=cell), whole and clipped to a z-slab; what
nbody_hip_grid_export_layer writes; the work list of cell_units_kernel (units, counters, light list) -- and the forces on
grids one to three cells thick, where window_run clamps and drops rows.

One reference for the integer data: np.searchsorted on the sorted cell ids (tests/grid_ref.py, itself checked in
tests/test_grid_cpu.py); every such comparison is equality.  The forces are held to oracle.spatial_hash_forces_grid by
assert_hash_parity, unchanged.  NBH_HASH_LB, NBH_HASH_UNITS and NBH_HASH_SPECULATE are read when a grid is created, so
they are set (monkeypatch) before the constructor, and every case asserts the builder regime it was written for."""
import ctypes as C

import numpy as np
import pytest

import grid_ref as gr
import sort_ref as sr
from gpu_util import acc_of, assert_hash_parity, rel_err, to_device
from test_spatial_hash_gpu import KERNELS

pytestmark = pytest.mark.gpu

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    diff = got != want
    bad = np.flatnonzero(diff if diff.ndim == 1 else diff.any(axis=1))
    k = int(bad[0])
    pytest.fail(f"{what}: {bad.size} of {want.shape[0]} entries differ, first at {k}: got {got[k]}, want {want[k]}")


# ---- building and reading back ---------------------------------------------------------------------------------------------
def build(nb, grid, case, slab=None):
    """a packed build with the case's explicit bounds -> the device bodies, to be kept alive while the grid is read"""
    import torch
    lib = nb._lib.load()
    nb._lib.check(lib.nbody_hip_grid_set_slab(grid._h, *(slab if slab is not None else (0, 0))))
    posm = torch.from_numpy(case.posm).cuda()
    bounds = (C.c_float * 6)(*case.bounds)
    nb._lib.check(lib.nbody_hip_grid_build_packed(grid._h, posm.data_ptr(), case.n, bounds))
    return posm


def check_sort(nb, grid, case, tag):
    dims, total, _, _ = grid._info()
    assert tuple(dims) == case.dims and total == case.total, f"{tag}: grid {dims} against {case.dims}"
    _, _, pc, si = sr.grid_cell_data(nb, grid, case.n)
    same(pc, case.keys, f"{tag}: particle_cells against the intended keys")
    same(si, case.order, f"{tag}: sorted_indices against the stable argsort")


def check_start_array(grid, sorted_keys, n, cov, tag):
    """the exported start array against searchsorted; -> it (None: the build made none, as it should)"""
    got = grid.copyCellStartArray()
    if not gr.has_array(n, cov):
        assert got is None, f"{tag}: a start array where the build makes none"
        return None
    assert got is not None, f"{tag}: no start array"
    base, count, lb = got
    assert (base, count) == cov, f"{tag}: covers {(base, count)} against {cov}"
    same(lb, gr.start_array(sorted_keys, cov), f"{tag}: start array against searchsorted(left)")
    return lb


def export_layer(nb, grid, dims, z, room):
    """(rc, bodies words [room + 8, 4], lb [layer + 1 + 8]) with sentinel words behind both outputs"""
    import torch
    layer = dims[0] * dims[1]
    bodies = torch.full((room + 8, 4), -7.0, dtype=torch.float32, device="cuda")
    lb = torch.full((layer + 1 + 8,), -7, dtype=torch.int32, device="cuda")
    rc = nb._lib.load().nbody_hip_grid_export_layer(grid._h, z, bodies.data_ptr(), lb.data_ptr())
    torch.cuda.synchronize()
    return rc, bodies.cpu().numpy().view(np.uint32), lb.cpu().numpy()


def check_layers(nb, grid, case, cov, lb, tag):
    """every layer of the grid: the covered ones against the reference, the others ERR_VALIDATION"""
    sentinel = np.float32(-7.0).view(np.uint32)
    for z in range(-1, case.dims[2] + 1):
        want = gr.layer_export(lb, cov, case.dims, z, case.sorted_posm)
        room = 0 if want is None else want[0].shape[0]
        rc, bodies, lbz = export_layer(nb, grid, case.dims, z, room)
        if want is None:
            assert rc == nb._lib.ERR_VALIDATION, f"{tag}: layer {z} outside the slab gave {rc}"
            continue
        assert rc == 0, f"{tag}: layer {z}: {rc}"
        same(bodies[:room], want[0].view(np.uint32), f"{tag}: layer {z}: bodies_out against posm[order]")
        same(lbz[:-8], want[1], f"{tag}: layer {z}: lb_out against the start array rebased to 0")
        assert np.all(bodies[room:] == sentinel) and np.all(lbz[-8:] == -7), f"{tag}: layer {z}: words behind the outputs"


# ---- start array, 1-D grids -------------------------------------------------------------------------------------------------
LINES = gr.line_cases()


@pytest.mark.parametrize("name", sorted(LINES))
def test_start_array_on_a_line(nb, ctx, monkeypatch, name):
    """(a) runs of empty cells around kGapInline, between the keys and at both ends; (b) every body in one cell; (c) no
    empty cell (and, for the coarse level, every third cell); (d) random occupancy; (e) count = 2 n, 2 n + 1 and
    16 n + 4096 -- through the builder the case is written for, and the position cases through NBH_HASH_LB=cell as well"""
    hist, want = LINES[name]
    case = memo(("line", name), lambda: gr.Crafted((hist.size, 1, 1), hist, seed=11))
    cov = gr.covered(case.dims)
    for env in (None, "cell") if want == "position" else (None,):
        if env:
            monkeypatch.setenv("NBH_HASH_LB", env)
        else:
            monkeypatch.delenv("NBH_HASH_LB", raising=False)
        assert gr.builder(case.n, cov, env) == (env or want)
        grid = nb.SpatialHashGrid(case.n, 1.0)
        for k in range(2):   # (twice: the gap list's counters alternate)
            keep = build(nb, grid, case)
            tag = f"{name}, builder {env or want}, build {k}"
            check_sort(nb, grid, case, tag)
            check_start_array(grid, case.sorted_keys, case.n, cov, tag)
            del keep
        grid.close()


def test_start_array_with_more_long_runs_than_waves(nb, ctx):
    """(f) 3,015 runs of 65 empty cells in one build: cell_gap_kernel has 2,048 waves, so its stride loop runs"""
    hist = gr.hist_many_runs()
    case = memo(("many runs",), lambda: gr.Crafted((hist.size, 1, 1), hist, seed=12))
    cov = gr.covered(case.dims)
    assert gr.builder(case.n, cov) == "position" and gr.long_runs(case.sorted_keys, cov) > 512 * 4
    grid = nb.SpatialHashGrid(case.n, 1.0)
    for k in range(2):
        keep = build(nb, grid, case)
        check_sort(nb, grid, case, f"build {k}")
        check_start_array(grid, case.sorted_keys, case.n, cov, f"build {k}")
        del keep
    grid.close()


def test_no_start_array_one_cell_past_the_threshold(nb, oracle, ctx):
    """(e) 16 n + 4096 + 1 cells: the export says there is no array, the calls that need one say ERR_STATE, and the forces
    (the cell-run kernel) still match the oracle"""
    import torch
    hist = gr.hist_no_array()
    case = memo(("no array",), lambda: gr.Crafted((hist.size, 1, 1), hist, seed=13, jitter=gr.NO_ARRAY_JITTER))
    cov = gr.covered(case.dims)
    assert gr.builder(case.n, cov) is None and cov[1] == 16 * case.n + 4096 + 1
    lib = nb._lib.load()
    grid = nb.SpatialHashGrid(case.n, 1.0)
    keep = build(nb, grid, case)
    check_sort(nb, grid, case, "no array")
    assert check_start_array(grid, case.sorted_keys, case.n, cov, "no array") is None
    acc = torch.zeros((case.n, 4), device="cuda")
    out = torch.zeros((case.n + 8, 4), device="cuda")
    lbz = torch.zeros(cov[1] + 8, dtype=torch.int32, device="cuda")
    assert lib.nbody_hip_grid_forces_pair_packed(grid._h, grid._h, 0, 0, 1.0, 1.0, 0.05, acc.data_ptr(), 0) == nb._lib.ERR_STATE
    assert lib.nbody_hip_grid_export_layer(grid._h, 0, out.data_ptr(), lbz.data_ptr()) == nb._lib.ERR_STATE
    with pytest.raises(nb._lib.StateException):
        grid.unitList(0, cov[1], 128)
    # computeForces on this very build (the cell-run kernel: nothing else runs without a start array) against the oracle
    d, _ = to_device(nb, case.ic)
    ic = case.ic
    ref, _, kappa = oracle.spatial_hash_forces_grid_cond(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], case.n, 1.0,
                                                         float(np.float32(0.05) ** 2), 1.0, 1.0, case.bounds[:3], case.dims)
    grid.computeForces(d, 1.0, 1.0, 0.05)
    a = acc_of(d)
    nz = np.linalg.norm(ref, axis=1) > 0
    assert nz.mean() > 0.9 and np.all(a[~nz] == 0)
    assert_hash_parity("no start array", rel_err(a[nz], ref[nz]), kappa[nz], "oracle", 0)
    del keep
    grid.close()


# ---- start array and layer export, slabs -------------------------------------------------------------------------------------
# (an empty slab holds no bodies: only the case with bodies outside it exists)
SLAB_CASES = [(d, w, o) for d in gr.SLAB_GRIDS for w in range(7) for o in (False, True)
              if o or gr.covered(d, gr.slabs_of(d[2])[w]) is not None]


@pytest.mark.parametrize("dims,which,outside", SLAB_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_start_array_and_layers_of_a_slab(nb, ctx, dims, which, outside):
    """the whole grid, one layer at the bottom, three in the middle, one at the top, clipped at the top, clipped at the
    bottom, and an empty slab; bodies in the slab only / also below and above it (prev < first and cur > last in
    cell_mark_kernel).  Every covered layer is exported and compared, every other one is refused."""
    slab = gr.slabs_of(dims[2])[which]
    cov = gr.covered(dims, slab)
    case = memo(("slab", dims, which, outside), lambda: gr.Crafted(dims, gr.hist_slab(dims, slab, outside, 7), seed=14))
    tag = f"grid {dims} slab {slab}"
    grid = nb.SpatialHashGrid(case.n, 1.0)
    keep = build(nb, grid, case, slab)
    check_sort(nb, grid, case, tag)
    lb = check_start_array(grid, case.sorted_keys, case.n, cov, tag)
    if cov is None:
        rc, _, _ = export_layer(nb, grid, dims, 0, case.n)
        assert lb is None and rc == nb._lib.ERR_STATE
    else:
        assert gr.builder(case.n, cov) == "position"
        check_layers(nb, grid, case, cov, lb, tag)
    # the slab setting of the next build replaces this one: the whole grid again
    del keep
    keep = build(nb, grid, case)
    check_start_array(grid, case.sorted_keys, case.n, gr.covered(dims), tag + ", then the whole grid")
    grid.close()


def test_export_layer_empty_full_and_large(nb, ctx):
    """an empty layer beside one that holds every body; a layer of 131,769 cells, more than the 512 workgroups of
    layer_export_kernel cover in one pass"""
    h = np.zeros(5 * 3 * 3, np.int64)
    h[15:30] = np.arange(15) * 7 % 11
    small = memo(("layers small",), lambda: gr.Crafted((5, 3, 3), h, seed=15))
    big_dims = (363, 363, 2)
    total = big_dims[0] * big_dims[1] * 2
    big = memo(("layers big",), lambda: gr.Crafted(big_dims, np.bincount(np.random.default_rng(3).integers(0, total, 20000),
                                                                         minlength=total), seed=16))
    assert big_dims[0] * big_dims[1] + 1 > 512 * 256 and gr.builder(big.n, gr.covered(big_dims)) == "two-level"
    for case in (small, big):
        cov = gr.covered(case.dims)
        grid = nb.SpatialHashGrid(case.n, 1.0)
        keep = build(nb, grid, case)
        tag = f"grid {case.dims}"
        check_sort(nb, grid, case, tag)
        lb = check_start_array(grid, case.sorted_keys, case.n, cov, tag)
        check_layers(nb, grid, case, cov, lb, tag)
        del keep
        grid.close()
    lb = gr.start_array(small.sorted_keys, gr.covered(small.dims))
    assert lb[15] == 0 and lb[30] == small.n   # (layer 0 and 2 empty, layer 1 everything)


# ---- sequences of builds on one grid ---------------------------------------------------------------------------------------------
class LineBuild:
    """bodies on a line of cells along x, built from the bodies alone (grid.build: the key pass may be launched ahead of the
    grid record); geometry and keys as the oracle states them"""

    def __init__(self, oracle, hist, seed):
        c = gr.Crafted((len(hist), 1, 1), hist, seed=seed)
        self.ic, self.n = c.ic, c.n
        self.lo, self.dims = sr.grid_geometry(oracle, self.ic, 1.0)
        self.total = self.dims[0] * self.dims[1] * self.dims[2]
        self.keys = sr.grid_keys(oracle, self.ic, 1.0, self.lo, self.dims)
        self.order = sr.stable_order(self.keys)
        self.sorted_keys = self.keys[self.order]
        self.cov = (0, self.total)


def sequence(oracle):
    def every(G, step, m):
        h = np.zeros(G, np.int64)
        h[::step] = m
        return h
    return [(LineBuild(oracle, every(14, 1, 40), 1), "position", False),      # no run of 64 cells
            (LineBuild(oracle, every(600, 6, 1), 2), "two-level", None),      # overwrites the counters' scratch area; regrows
            (LineBuild(oracle, every(2000, 100, 250), 3), "position", True),  # long runs; regrows
            (LineBuild(oracle, every(2000, 80, 200), 4), "position", True),   # other runs, the other counter
            (LineBuild(oracle, every(2000, 70, 170), 7), "position", True),   # and the first counter again: zeroed two builds ago
            (LineBuild(oracle, every(6000, 1, 3), 5), "position", True),      # larger than lb_capacity again
            (LineBuild(oracle, every(10, 1, 30), 6), "position", False)]      # a small grid in the large allocation


@pytest.mark.parametrize("speculate", [None, "2"])
def test_sequences_of_builds_on_one_grid(nb, oracle, ctx, monkeypatch, speculate):
    steps = memo(("sequence",), lambda: sequence(oracle))
    cap = 0
    grows = []
    for b, want, runs in steps:   # (the regime and the growth of every step, before anything runs)
        assert gr.builder(b.n, b.cov) == want
        if runs is not None:
            assert (gr.long_runs(b.sorted_keys, b.cov) > 0) == runs
        grows.append(b.total + 1 > cap)
        if grows[-1]:
            cap = (b.total + 1) + (b.total + 1) // 2
    assert grows == [True, True, True, False, False, True, False]
    if speculate:
        monkeypatch.setenv("NBH_HASH_SPECULATE", speculate)
    grid = nb.SpatialHashGrid(max(b.n for b, _, _ in steps), 1.0)
    for k, (b, want, _) in enumerate(steps):
        d, _ = to_device(nb, b.ic)
        grid.build(d)
        tag = f"NBH_HASH_SPECULATE={speculate}, build {k} ({want})"
        dims, total, _, _ = grid._info()
        assert list(dims) == list(b.dims)
        _, _, pc, si = sr.grid_cell_data(nb, grid, b.n)
        same(pc, b.keys, f"{tag}: particle_cells")
        same(si, b.order, f"{tag}: sorted_indices")
        check_start_array(grid, b.sorted_keys, b.n, b.cov, tag)
    grid.close()


# ---- the work list ------------------------------------------------------------------------------------------------------------------
def check_units(got, want, tag):
    units, light, counts, cap = got
    same(counts, want["counts"], f"{tag}: the four counters")
    nh, no = int(counts[0]), int(counts[2])
    assert nh + no <= cap
    same(gr.unit_rows(units[:nh]), want["heavy"], f"{tag}: the units of the cells above 48 bodies, slots [0, {nh})")
    same(gr.unit_rows(units[cap - no:cap]), want["other"], f"{tag}: the other units, slots [{cap - no}, {cap})")
    same(np.sort(light.view(np.uint32)), want["light"], f"{tag}: the light list")


def unit_ranges(case, cov):
    """cell ranges of a case: the whole line, or every single layer the array covers"""
    layer = case.dims[0] * case.dims[1]
    if case.dims[2] == 1:
        return [(0, case.total)]
    return [(c, c + layer) for c in range(cov[0], cov[0] + cov[1], layer)]


UNIT_GRIDS = [((G, 1, 1), None) for G in gr.UNIT_LINES] + [(d, s) for d in gr.SLAB_GRIDS for s in (None, (2, 3))]


@pytest.mark.parametrize("setting", gr.UNIT_SETTINGS, ids=lambda s: f"chunk{s[0]}-min{s[1]}-mode{s[2]}")
@pytest.mark.parametrize("dims,slab", UNIT_GRIDS, ids=lambda v: str(v).replace(" ", ""))
def test_unit_list(nb, ctx, monkeypatch, dims, slab, setting):
    """lines of 2,047 / 2,048 / 2,049 / 4,097 cells (a workgroup takes 2,048) and single layers of the slab grids, whole
    (layer z starts at word 15 z: the clamped path, misaligned; at 32 z: the int4 path) and as the slab (2, 3).  The list is
    made twice in a row and once more after a force call that made lists of its own: the counters alternate."""
    import torch
    chunk, min_cnt, mode = setting
    total = dims[0] * dims[1] * dims[2]
    case = memo(("units", dims, setting), lambda: gr.Crafted(dims, gr.hist_units(total, chunk, min_cnt, 1), seed=17))
    cov = gr.covered(dims, slab)
    assert gr.builder(case.n, cov) == "position"
    if dims[2] > 1:   # which path the first thread of a layer takes
        layer = dims[0] * dims[1]
        aligned = [(c - cov[0]) % 4 == 0 for c, _ in unit_ranges(case, cov)]
        assert all(aligned) if layer % 4 == 0 else (any(aligned) and not all(aligned))
    monkeypatch.setenv("NBH_HASH_UNITS", "2")
    grid = nb.SpatialHashGrid(case.n, 1.0)
    keep = build(nb, grid, case, slab)
    tag = f"grid {dims} slab {slab} chunk {chunk} min_cnt {min_cnt} mode {mode}"
    check_sort(nb, grid, case, tag)
    lb = check_start_array(grid, case.sorted_keys, case.n, cov, tag)
    acc = torch.zeros((case.n, 4), device="cuda")
    for first, end in unit_ranges(case, cov):
        want = gr.unit_list(lb, cov, first, end, chunk, min_cnt, mode)
        for k in range(2):
            check_units(grid.unitList(first, end, chunk, min_cnt, mode), want, f"{tag}, cells [{first}, {end}), call {k}")
        grid.tuning(3)
        nb._lib.check(nb._lib.load().nbody_hip_grid_compute_forces_packed(grid._h, 1.0, 1.0, 0.05, acc.data_ptr()))
        grid.tuning(0)
        check_units(grid.unitList(first, end, chunk, min_cnt, mode), want, f"{tag}, cells [{first}, {end}), after forces")
    # ranges that are not inside the covered cells
    for first, end in ((cov[0] - 1, cov[0] + 1), (cov[0], cov[0] + cov[1] + 1), (cov[0] + 1, cov[0] + 1)):
        with pytest.raises(nb._lib.ValidationException):
            grid.unitList(first, end, chunk, min_cnt, mode)
    del keep
    grid.close()


# ---- forces at the rim of a thin grid -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.05, 0.0])
@pytest.mark.parametrize("cutoff", [1.0, 1.7])
@pytest.mark.parametrize("dims", gr.RIM_GRIDS, ids=str)
def test_forces_at_the_rim(nb, oracle, ctx, dims, cutoff, eps):
    """grids 1, 2 and 3 cells thick: window_run clamps c.x - 1 and c.x + 2 and drops the rows outside gy and gz in every
    cell.  Every force kernel and the automatic choice against the oracle on the same grid; the two-grid call over all
    layers gives the same bits as the one-grid call when the same kernel is forced."""
    import torch
    ic, bounds = memo(("rim", dims), lambda: gr.rim_bodies(dims))
    n, G = gr.RIM_N, 1.0
    eps2 = float(np.float32(eps) * np.float32(eps))
    ref, _, kappa = memo(("rim ref", dims, cutoff, eps), lambda: oracle.spatial_hash_forces_grid_cond(
        ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], n, G, eps2, 1.0, cutoff, bounds[:3], dims))
    nz = np.linalg.norm(ref, axis=1) > 0
    assert (~nz).mean() <= 0.10
    lib = nb._lib.load()
    posm = torch.from_numpy(sr.posm_of(ic)).cuda()
    grid = nb.SpatialHashGrid(n, 1.0)
    nb._lib.check(lib.nbody_hip_grid_build_packed(grid._h, posm.data_ptr(), n, (C.c_float * 6)(*bounds)))
    assert tuple(grid._info()[0]) == dims and grid.copyCellStartArray() is not None
    acc, pair = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 4), device="cuda")
    for kern in (0,) + KERNELS:
        tag = f"grid {dims} cutoff {cutoff} eps {eps} kernel {kern}"
        grid.tuning(kern)
        acc.fill_(7.0)
        nb._lib.check(lib.nbody_hip_grid_compute_forces_packed(grid._h, cutoff, G, eps, acc.data_ptr()))
        torch.cuda.synchronize()
        a = acc.cpu().numpy()
        assert np.all(a[:, 3] == 0) and np.all(a[~nz, :3] == 0), tag
        assert_hash_parity(tag, rel_err(a[nz, :3], ref[nz]), kappa[nz], "oracle", kern)
        if kern != 1:   # (the two-grid call has no cell-run kernel: it takes its automatic choice instead)
            pair.fill_(7.0)
            nb._lib.check(lib.nbody_hip_grid_forces_pair_packed(grid._h, grid._h, 0, 0, cutoff, G, eps, pair.data_ptr(), 0))
            torch.cuda.synchronize()
            same(pair.cpu().numpy().view(np.uint32), a.view(np.uint32), f"{tag}: forces_pair_packed(g, g) against compute_forces_packed")
    grid.tuning(0)
    grid.close()
