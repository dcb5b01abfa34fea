"""CPU restatement of the friends-of-friends groups (nbody_hip_grid_groups, include/nbody_hip_groups.h) for the tests.

  fof_labels   candidate pairs from scipy's kd-tree at b (1 + 1e-4); a pair is linked when fp32_dist2 of the fp32
               coordinate differences is < fl(b * b) (the kernels' fma chain, bit for bit) and the cell ids of the two
               bodies differ by at most 1 along every axis (cell_of = the grid's own ids, or field_ref.hash_cells; None: no
               cell restriction, plain friends-of-friends); connected components, each relabelled with its lowest index
  catalogue    (offsets, members) of the groups of at least min_members bodies: ascending by label, members ascending
  grid_of      the box and the dimensions a build gives the bodies (the box padded by 0.001, cells as grid_axis_cells
               counts them): what field_ref.hash_cells needs to restate the cell ids without a GPU
  union_find   the same labels from given links by a plain-Python union-find (the check of the restatement itself)
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from potential_ref import fp32_dist2


def linked_pairs(pos, b, cell_of=None, dims=None):
    """(i, j) arrays, i < j, of the linked pairs"""
    pos32 = np.ascontiguousarray(pos, np.float32)
    b32 = np.float32(b)
    b2 = np.float32(b32 * b32)
    pairs = cKDTree(pos32.astype(np.float64)).query_pairs(float(b32) * (1.0 + 1e-4), output_type="ndarray")
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    d = (pos32[j] - pos32[i]).astype(np.float32)
    ok = fp32_dist2(d[:, 0], d[:, 1], d[:, 2]) < b2
    if cell_of is not None:
        gx, gy, _ = (int(v) for v in dims)
        c = np.asarray(cell_of, np.int64)
        xyz = np.stack([c % gx, (c // gx) % gy, c // (gx * gy)], 1)
        ok &= (np.abs(xyz[i] - xyz[j]) <= 1).all(1)
    return i[ok], j[ok]


def labels_of(n, i, j):
    graph = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    lowest = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(lowest, comp, np.arange(n))
    return lowest[comp].astype(np.int32)


def fof_labels(pos, b, cell_of=None, dims=None):
    i, j = linked_pairs(pos, b, cell_of, dims)
    return labels_of(len(pos), i, j)


def catalogue(labels, min_members=1):
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    sizes = np.bincount(labels, minlength=n)
    order = np.argsort(labels, kind="stable")
    order = order[sizes[labels[order]] >= min_members]
    key = labels[order]
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(order) else np.zeros(0, np.int64)
    return np.r_[heads, len(order)].astype(np.int32), order.astype(np.int32)


def grid_of(pos, cell):
    """(bmin [3] fp32, dims [3]) of the grid a build makes of these bodies with this cell size"""
    f = np.float32
    pos32 = np.asarray(pos, f)
    lo = (pos32.min(0) - f(0.001)).astype(f)
    hi = (pos32.max(0) + f(0.001)).astype(f)
    cells = np.ceil(((hi - lo).astype(f) / f(cell)).astype(f))
    return lo, cells.astype(np.int64) + 1


def union_find(n, i, j):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(i, j):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], np.int32)


def uniform_box(n=20000, seed=7):
    """n bodies uniform in the unit box, and their mean spacing"""
    pos = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    return pos, 1.0 / n ** (1.0 / 3.0)
