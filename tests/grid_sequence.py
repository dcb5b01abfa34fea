"""One reused spatial-hash grid driven through every branch of its host state machine (csrc/grid_plan.h: the three methods
of the start array and the grid without one, the regrown array and its scratch tail, the speculated key bits, the force
plan of every tuning, the work list and its statistics, the point workspace, a slab and the two-grid / layer entries, a
pending cell size), step by step.

sequence() yields one record per observable result; tests/test_grid_sequences_gpu.py compares each with a fresh grid that
was given only the settings in force at that step, tools/hash_digest.py digests them to compare two builds of the library
bit for bit."""
import ctypes as C

import numpy as np
import torch

from gpu_util import acc_of, packed, to_device

G = 1.0
N, CROWD, HALF = 4096, 300, 8.0
SCALES = (1.0, 1.6, 4.0)
DEFAULTS = {"scale": 1.0, "cell": 1.0, "tuning": 0}
TUNINGS = (1, 2, 3, 4, 6, 7, 8, 9, 10)


def prepare(nb):
    """{scale: (ic, device bodies, packed device bodies)}: 4,096 bodies in a box of half-width 8 plus 300 in one cell,
    positions times `scale`"""
    a = nb.ic.uniform_box(N, seed=7, lo=-HALF, hi=HALF, min_mass=0.5, max_mass=1.5)
    rng = np.random.default_rng(8)
    base = {k: np.concatenate([v, (rng.uniform(0.05, 0.95, CROWD) if k.startswith("pos") else
                                   np.full(CROWD, 1.0 if k == "mass" else 0.0)).astype(np.float32)]) for k, v in a.items()}
    data = {}
    for scale in SCALES:
        ic = {k: (v * np.float32(scale)).astype(np.float32) if k.startswith("pos") else v.copy() for k, v in base.items()}
        data[scale] = (ic, to_device(nb, ic)[0], packed(ic))
    return data


def points(m, scale):
    """m points around the box, some outside it, one not a number"""
    pts = np.random.default_rng(12).uniform(-1.25 * HALF * scale, 1.25 * HALF * scale, (m, 3)).astype(np.float32)
    pts[17 % m, 0] = np.nan
    return torch.from_numpy(pts).cuda()


def forces(grid, d, cutoff, eps):
    grid.computeForces(d, cutoff, G, eps)
    return {"acc": acc_of(d)}  # (the copy to the host synchronises)


def potential(grid, d, cutoff, eps):
    phi = torch.zeros(d.count, dtype=torch.float32, device="cuda")
    pe = grid.computePotential(d, cutoff, G, eps, phi)
    return {"phi": phi.cpu().numpy(), "pe": np.float64(pe)}


def field(grid, scale, cutoff, eps, m):
    return {"field": grid.computeField(points(m, scale), cutoff, G, eps).cpu().numpy()}


def start_array(grid):
    got = grid.copyCellStartArray()
    if got is None:
        return {"has": np.int64(0)}
    return {"has": np.int64(1), "base": np.int64(got[0]), "count": np.int64(got[1]), "lb": got[2]}


def cells(grid):
    return {"total": np.int64(grid.getTotalCells()), "dims": np.array(grid.getGridDims(), np.int64)}


def slab(nb, be, data, s, cutoff, eps):
    """a z-slab of the bodies on the box of them all, through the entry points of the sharded path: the bodies of layers
    [2, gz - 2) on grid "own" of the backend; one of its layers exported; the two-grid call over the slab and the layer
    call of the layer below the exported one, each overwriting and then accumulating"""
    from nbody_amd._lib import check
    lib = be.ctx._lib
    _, _, p = data[s["scale"]]
    bb = be.bbox(p).cpu().numpy()
    bounds = [float(v) for v in np.concatenate([bb[:3] - np.float32(0.001), bb[3:] + np.float32(0.001)])]
    dims = [int(np.ceil(np.float32(bounds[3 + a] - bounds[a]) / np.float32(s["cell"]))) + 1 for a in range(3)]
    gx, gy, gz = dims
    z0, nz = 2, gz - 4
    cz = be.cell_z(p, bounds[2], s["cell"], gz)
    mine = p[(cz >= z0) & (cz < z0 + nz)].contiguous()
    m = mine.shape[0]
    be.grid_build("own", mine, bounds, s["cell"], z0, nz)
    own = be._grids["own"][0]
    built, total = (C.c_int * 3)(), C.c_int()
    check(lib.nbody_hip_grid_info(own, C.byref(built), C.byref(total), C.byref((C.c_float * 3)()), C.byref((C.c_float * 3)())))
    assert list(built) == dims, (list(built), dims)
    check(lib.nbody_hip_grid_tuning(own, s["tuning"]))
    zs, zt = z0 + nz // 2, z0 + nz // 2 - 1
    layer_bodies = torch.zeros((m, 4), dtype=torch.float32, device="cuda")
    layer_lb = torch.zeros(gx * gy + 1, dtype=torch.int32, device="cuda")
    check(lib.nbody_hip_grid_export_layer(own, zs, layer_bodies.data_ptr(), layer_lb.data_ptr()))
    out = {"bodies": np.int64(m), "dims": np.array(dims, np.int64), "layer_bodies": layer_bodies.cpu().numpy(),
           "layer_lb": layer_lb.cpu().numpy()}
    acc = torch.full((m, 4), 7.0, device="cuda")
    for accumulate in (0, 1):
        assert be.grid_forces("own", "own", z0 - 1, nz + 5, cutoff, G, eps, acc, bool(accumulate))  # (clipped to the slab)
        out[f"pair{accumulate}"] = acc.cpu().numpy()
    for accumulate in (0, 1):
        check(lib.nbody_hip_grid_forces_layer_packed(own, zt, layer_bodies.data_ptr(), layer_lb.data_ptr(), zs, cutoff, G, eps,
                                                     acc.data_ptr(), accumulate))
        out[f"layer{accumulate}"] = acc.cpu().numpy()
    return out


def call(nb, ctx, grid, data, s, kind, args):
    """one observable result of `grid`, which stands at the settings `s`"""
    d = data[s["scale"]][1]
    if kind == "forces":
        return forces(grid, d, *args)
    if kind == "potential":
        return potential(grid, d, *args)
    if kind == "field":
        return field(grid, s["scale"], *args)
    if kind == "start":
        return start_array(grid)
    if kind == "cells":
        return cells(grid)
    raise ValueError(kind)


def sequence(nb, ctx, data):
    """yields (label, settings, kind, args, arrays): what a fresh grid with `settings` (scale of the bodies, cell size AS
    BUILT, tuning) must reproduce by `kind` with `args`"""
    from nbody_amd.distributed import HipBackend
    s = dict(DEFAULTS)
    grid = nb.SpatialHashGrid(N + CROWD, 1.0)

    def rec(label, kind, *args):
        return label, dict(s), kind, args, call(nb, ctx, grid, data, s, kind, args)

    def build(label, scale):
        grid.build(data[scale][1])
        s.update(scale=scale, cell=grid.getCellSize())
        yield rec(label + ": cells", "cells")
        yield rec(label + ": start array", "start")
        yield rec(label + ": forces", "forces", 1.0, 0.05)

    yield from build("1 scale 1", 1.0)
    yield from build("2 scale 1.6 (two-level search, regrown start array, other key bits)", 1.6)
    yield rec("2 scale 1.6: potential", "potential", 1.0, 0.05)
    yield from build("3 scale 1 again (dirty scratch counters, wrong speculation)", 1.0)
    yield from build("4 scale 4 (no start array)", 4.0)
    yield rec("4 scale 4: potential", "potential", 1.0, 0.05)
    yield rec("4 scale 4: field at 100 points", "field", 1.0, 0.05, 100)
    yield from build("5 scale 1 once more", 1.0)
    for k in range(10):
        yield rec(f"6 automatic, call {k + 1} of ten", "forces", 1.0, 0.05)
    grid.tuning(3)
    s["tuning"] = 3
    for k in range(10):  # (the first makes the list for its statistics, the second takes the unit form: a crowded cell)
        yield rec(f"6 tuning 3, call {k + 1} of ten", "forces", 1.0, 0.05)
    for tuning in TUNINGS:
        grid.tuning(tuning)
        s["tuning"] = tuning
        for eps in (0.05, 0.0):
            for cutoff in (1.0, 1.7):
                yield rec(f"7 tuning {tuning} eps {eps} cutoff {cutoff}", "forces", cutoff, eps)
    grid.tuning(0)
    s["tuning"] = 0
    yield rec("8 potential", "potential", 1.0, 0.05)
    yield rec("8 field at 100 points", "field", 1.0, 0.05, 100)
    yield rec("8 field at 10,000 points (the workspace grows)", "field", 1.0, 0.05, 10000)
    # a slab on a backend's handle that held the whole box before
    be = HipBackend(ctx)
    p = data[1.0][2]
    bb = be.bbox(p).cpu().numpy()
    be.grid_build("own", p, [float(v) for v in bb[:3] - 1] + [float(v) for v in bb[3:] + 1], 1.0, 0, 0)
    acc = torch.zeros((p.shape[0], 4), device="cuda")
    assert be.grid_forces("own", "own", 0, 0, 1.0, G, 0.05, acc, False)
    for tuning in (0, 3):
        yield f"9 slab, tuning {tuning}", dict(s, tuning=tuning), "slab", (1.0, 0.05), slab(nb, be, data, dict(s, tuning=tuning), 1.0, 0.05)
    be.close()
    # a pending cell size does not reach the grid as built
    before = []
    for tuning in (1, 0):
        grid.tuning(tuning)
        s["tuning"] = tuning
        before.append(rec(f"10 before setCellSize, tuning {tuning}: forces", "forces", 1.5, 0.05))
        before.append(rec(f"10 before setCellSize, tuning {tuning}: potential", "potential", 1.5, 0.05))
        before.append(rec(f"10 before setCellSize, tuning {tuning}: field", "field", 1.5, 0.05, 100))
    yield from before
    grid.setCellSize(2.0)
    for tuning in (1, 0):
        grid.tuning(tuning)
        s["tuning"] = tuning
        yield rec(f"10 after setCellSize without a build, tuning {tuning}: forces", "forces", 1.5, 0.05)
        yield rec(f"10 after setCellSize without a build, tuning {tuning}: potential", "potential", 1.5, 0.05)
        yield rec(f"10 after setCellSize without a build, tuning {tuning}: field", "field", 1.5, 0.05, 100)
    yield from build("11 build at cell 2", 1.0)
    grid.close()


def fresh(nb, ctx, data, s, kind, args):
    """the result of `kind` on a new grid given only the settings `s`: one build, one call"""
    if kind == "slab":
        from nbody_amd.distributed import HipBackend
        be = HipBackend(ctx)
        out = slab(nb, be, data, s, *args)
        be.close()
        return out
    grid = nb.SpatialHashGrid(N + CROWD, s["cell"])
    if s["tuning"]:
        grid.tuning(s["tuning"])
    grid.build(data[s["scale"]][1])
    out = call(nb, ctx, grid, data, s, kind, args)
    grid.close()
    return out
