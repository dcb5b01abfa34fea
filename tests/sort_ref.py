"""What tests/test_sort_edges_gpu.py (and the oracle pins of the 63-bit key) share: the sort keys of a body set as the
oracle states them, the one reference of every permutation -- np.argsort(key, kind="stable") --, and thin ctypes
readers of what a grid / a tree holds after a build.  Nothing here imports torch before a GPU helper is called."""
import ctypes as C

import numpy as np

import oracle_bind as ob

F = np.float32


# ---- keys -------------------------------------------------------------------------------------------------------------
def root_cube(oracle, x, y, z):
    """(lo[3], scale of the 10-bit keys, scale of the 21-bit keys) of the Barnes-Hut root cube, in float32 as
    root_from_bbox (csrc/barnes_hut.hip) forms them: lo = centre - half, 1024 / (2 half), then times 2048."""
    c, half = oracle.bh_root(x, y, z)
    half = F(half)
    lo = [F(F(c[a]) - half) for a in range(3)]
    s10 = F(F(1024.0) / F(F(2.0) * half))
    return lo, s10, F(s10 * F(2048.0))


def bh_keys_numpy(x, y, z, lo, scale, bits):
    """the key of oracle_bh_keys restated bit by bit: q = clamp((int)((p - lo) * scale), 0, 2^bits - 1) in float32, bit b
    of the x / y / z coordinate at key bit 3 b + 2 / + 1 / + 0"""
    top = (1 << bits) - 1
    key = np.zeros(x.size, np.uint64)
    for a, p in enumerate((x, y, z)):
        f = (p.astype(F) - F(lo[a])) * F(scale)
        assert f.dtype == F
        q = np.clip(f.astype(np.int64), 0, top).astype(np.uint64)   # (int) truncates towards zero, and so does astype
        for b in range(bits):
            key |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + (2 - a))
    return key


def tree_keys(oracle, ic, max_depth):
    """the bits a tree of max_depth > 10 sorts: the leading 3 max_depth of the 63 key bits"""
    x, y, z = ic["pos_x"], ic["pos_y"], ic["pos_z"]
    lo, _, s21 = root_cube(oracle, x, y, z)
    return oracle.bh_keys(x, y, z, lo, s21, bits=21) >> np.uint64(63 - 3 * max_depth)


def grid_geometry(oracle, ic, cell, bounds=None):
    """(lo[3], dims[3]) of the grid a build makes: the oracle's hash_grid (box of the bodies padded by 0.001), or the
    explicit (already padded) `bounds` = lo x, y, z, hi x, y, z of nbody_hip_grid_build_packed"""
    if bounds is None:
        lo, _, dims = oracle.hash_grid(ic["pos_x"], ic["pos_y"], ic["pos_z"], cell)
    else:
        lo = [float(F(v)) for v in bounds[:3]]
        dims = oracle.grid_dims(lo, [float(F(v)) for v in bounds[3:]], cell)
    return lo, dims


def grid_keys(oracle, ic, cell, lo, dims):
    n = ic["pos_x"].size
    cells = np.empty(n, np.int32)
    oracle.L.oracle_assign_cells(n, ic["pos_x"], ic["pos_y"], ic["pos_z"], ob._f3(*lo), cell, ob._i3(*dims), cells)
    return cells


def stable_order(key):
    """THE reference: sorted position -> input index"""
    return np.argsort(key, kind="stable").astype(np.int32)


def bits_for(total):
    """key bits of a grid of `total` cells (bits_for of csrc/grid_plan.h)"""
    b = 1
    while (1 << b) < total and b < 32:
        b += 1
    return b


# ---- bodies -----------------------------------------------------------------------------------------------------------
def bodies(x, y, z):
    """initial-condition dict of bodies at rest whose masses 1 + i 2^-17 are all different (exact in float32 below 2^17
    bodies): two bodies at one position are still two different float4 payloads"""
    n = len(x)
    assert n < (1 << 17)
    ic = {"pos_x": np.ascontiguousarray(x, F), "pos_y": np.ascontiguousarray(y, F), "pos_z": np.ascontiguousarray(z, F),
          "mass": (F(1.0) + np.arange(n, dtype=F) * F(2.0 ** -17)).astype(F)}
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k] = np.zeros(n, F)
    return ic


def take(ic, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in ic.items()}


def scaled(ic, s):
    return {k: ((v * F(s)).astype(F) if k.startswith("pos") else v) for k, v in ic.items()}


def posm_of(ic):
    return np.ascontiguousarray(np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"]], 1).astype(F))


# ---- what a grid / tree holds after a build (GPU) -----------------------------------------------------------------------
def sort_info(nb):
    """(driver_compiled, self_test, own_self_test, rocprim_version) of nbody_hip_sort_info"""
    v = [C.c_int(-1) for _ in range(4)]
    assert nb._lib.load().nbody_hip_sort_info(*[C.byref(c) for c in v]) == 0
    return tuple(c.value for c in v)


def grid_cell_data(nb, grid, n, total=None):
    """(cell_start, cell_end, particle_cells, sorted_indices) of the last build of n bodies; total = None: without the
    two per-cell arrays (NULL, which nbody_hip_grid_copy_cell_data allows)"""
    cs = ce = cs_ptr = ce_ptr = None
    if total is not None:
        cs, ce = np.empty(total, np.int32), np.empty(total, np.int32)
        cs_ptr, ce_ptr = cs.ctypes.data, ce.ctypes.data
    pc, si = np.empty(n, np.int32), np.empty(n, np.int32)
    nb._lib.check(nb._lib.load().nbody_hip_grid_copy_cell_data(grid._h, cs_ptr, ce_ptr, pc.ctypes.data, si.ctypes.data))
    return cs, ce, pc, si


def grid_sorted_bodies(nb, grid, n):
    """the n float4 bodies of the last build in cell order, as 32-bit words [n, 4]"""
    import torch
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    nb._lib.check(nb._lib.load().nbody_hip_grid_sorted_bodies(grid._h, 0, n, out.data_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def tree_order(nb, tree, n):
    """sorted position -> body index of the last build (nbody_hip_tree_copy_nodes without the nodes).  The C ABI does not
    hand out the tree's keys, so unlike the grid's particle_cells they are never held to the oracle's directly."""
    order = np.empty(n, np.int32)
    nb._lib.check(nb._lib.load().nbody_hip_tree_copy_nodes(tree._h, None, 0, order.ctypes.data))
    return order
