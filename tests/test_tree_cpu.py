"""tests/tree_ref.py -- the reference octree the GPU build is held to in test_tree_gpu.py -- checked without a GPU: against
a deliberately naive second builder (recursive insertion by position: no keys, no sort), against the two numbers the
oracle's tree exposes, and on trees whose shape can be counted by hand."""
import math

import numpy as np
import pytest

import quadrupole_ref as qr
import sort_ref as sr
import tree_ref as tr

F = np.float32


def cloud(n, seed, half=1.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-half, half, (n, 3)).astype(F)
    ic = sr.bodies(p[:, 0], p[:, 1], p[:, 2])
    ic["mass"] = rng.uniform(0.5, 2.0, n).astype(F)
    return ic


def lattice(side, extra=()):
    """side^3 bodies at the cell centres of a side^3 lattice over [-1, 1]^3, then `extra` positions.  The root cube is
    the bounding box widened by 0.001 on every side, so each body stays well inside its lattice cell."""
    g = (np.arange(side) + 0.5) / side * 2.0 - 1.0
    x, y, z = (v.ravel() for v in np.meshgrid(g, g, g, indexing="ij"))
    pts = np.stack([x, y, z], 1)
    if len(extra):
        pts = np.concatenate([pts, np.asarray(extra, np.float64).reshape(-1, 3)])
    return sr.bodies(pts[:, 0], pts[:, 1], pts[:, 2])


# ---- the naive builder ---------------------------------------------------------------------------------------------------
def quantise(oracle, ic):
    """the integer position of every body on the 2^21 lattice of the root cube (morton_kernel's q, restated): the only
    thing the naive builder shares with the keys is this rounding of a position to a lattice cell"""
    x, y, z = ic["pos_x"], ic["pos_y"], ic["pos_z"]
    lo, _, s21 = sr.root_cube(oracle, x, y, z)
    q = np.empty((x.size, 3), np.int64)
    for a, p in enumerate((x, y, z)):
        q[:, a] = np.clip(((p.astype(F) - F(lo[a])) * F(s21)).astype(np.int64), 0, (1 << 21) - 1)
    return q


def naive_tree(q, max_depth, leaf_max):
    """breadth-first list of nodes {level, bodies (ascending index), children by octant, first}; a node is split while
    it holds more than leaf_max bodies and sits above max_depth, each body going to the octant its position lies in"""
    nodes = [dict(level=0, bodies=list(range(len(q))), cell=(0, 0, 0))]
    k = 0
    while k < len(nodes):
        nd = nodes[k]
        nd["children"] = [-1] * 8
        L = nd["level"]
        if len(nd["bodies"]) > leaf_max and L < max_depth:
            buckets = [[] for _ in range(8)]
            for b in nd["bodies"]:
                side = [(int(q[b, a]) >> (20 - L)) & 1 for a in range(3)]   # which half of the cell, per axis
                buckets[4 * side[0] + 2 * side[1] + side[2]].append(b)
            for o, bs in enumerate(buckets):
                if bs:
                    nd["children"][o] = len(nodes)
                    cell = tuple(2 * nd["cell"][a] + ((o >> (2 - a)) & 1) for a in range(3))
                    nodes.append(dict(level=L + 1, bodies=bs, cell=cell))
        k += 1
    # positions in the depth-first octant order = the Morton order of the leaves
    def number(i, first):
        nodes[i]["first"] = first
        for c in nodes[i]["children"]:
            if c >= 0:
                first = number(c, first)
        return nodes[i]["first"] + len(nodes[i]["bodies"])
    number(0, 0)
    # breadth-first order with children appended octant by octant IS level-major; inside a level the nodes of one
    # parent are in octant order and the parents in key order, so the level is key-ascending
    return nodes


@pytest.mark.parametrize("leaf_max", [1, 3, 8])
@pytest.mark.parametrize("max_depth", [1, 3, 10, 11, 21])
def test_reference_equals_recursive_insertion(oracle, max_depth, leaf_max):
    ic = cloud(300, seed=100 * max_depth + leaf_max)
    for k in ("pos_x", "pos_y", "pos_z"):
        ic[k][40:46] = ic[k][40]      # six coincident bodies: a chain to max_depth
        ic[k][7] = ic[k][8]
    ic["mass"][40:43] = 0.0
    t = tr.RefTree(oracle, ic, max_depth, leaf_max)
    nodes = naive_tree(quantise(oracle, ic), max_depth, leaf_max)
    assert t.node_count == len(nodes)
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1).astype(np.float64)
    m = ic["mass"].astype(np.float64)
    M, c, S = t.moments()
    half = F(t.root_half)
    for k, nd in enumerate(nodes):
        tag = f"node {k} (level {nd['level']})"
        assert t.level[k] == nd["level"], tag
        assert t.first[k] == nd["first"] and t.last[k] == nd["first"] + len(nd["bodies"]), tag
        assert sorted(t.order[t.first[k]:t.last[k]].tolist()) == nd["bodies"], tag
        assert t.children[k].tolist() == nd["children"], tag
        leaf = all(ch < 0 for ch in nd["children"])
        assert bool(t.is_leaf[k]) == leaf, tag
        if leaf and len(nd["bodies"]) == 1:
            assert t.particle_index[k] == nd["bodies"][0], tag
        elif leaf:
            assert t.particle_index[k] in nd["bodies"], tag
        else:
            assert t.particle_index[k] == -1, tag
        # geometry: the cell the recursion arrived at
        h = float(half) / 2 ** nd["level"]
        assert float(t.half_size[k]) == h
        want = [float(t.root_center[a]) - float(half) + (nd["cell"][a] + 0.5) * 2 * h for a in range(3)]
        assert np.allclose(t.center[k], want, rtol=0, atol=4 * np.spacing(F(abs(float(half)) + 1))), tag
        # moments: correctly rounded sums (math.fsum) of the exact products
        b = nd["bodies"]
        mass = math.fsum(m[b])
        assert abs(t.total_mass[k] - mass) <= np.spacing(mass), tag
        for a in range(3):
            com = math.fsum(m[b] * pos[b, a]) / mass if mass > 0 else 0.0
            assert abs(t.center_of_mass[k, a] - com) <= 2 * np.spacing(abs(com)), tag
        if mass > 0:
            M1, c1, S1 = qr.moments_of(pos[b], m[b])
            assert abs(M[k] - M1) <= 1e-14 * M1 and np.allclose(c[k], c1, rtol=0, atol=1e-14), tag
            assert np.allclose(S[k], S1, rtol=0, atol=1e-13 * (S1[:3].sum() + 1e-300)), tag
    # a one-body node is its body, bit for bit
    one = t.count == 1
    massive = one & (t.total_mass > 0)
    assert np.array_equal(t.center_of_mass[massive], t.pos_sorted[t.first[massive]].astype(np.float64))
    assert np.all(S[one] == 0)


@pytest.mark.parametrize("n,max_depth,leaf_max", [(1, 20, 1), (2, 20, 1), (300, 20, 1), (5000, 20, 1), (5000, 10, 8),
                                                  (4000, 3, 1), (6000, 21, 1), (6000, 16, 4)])
def test_reference_against_the_oracles_tree(oracle, n, max_depth, leaf_max):
    ic = cloud(n, seed=n + max_depth)
    for k in ("pos_x", "pos_y", "pos_z"):
        ic[k][: n // 50] = ic[k][0]          # coincident bodies
    t = tr.RefTree(oracle, ic, max_depth, leaf_max)
    *_, root_mass, nodes = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], np.arange(1), 1.0,
                                                    1e-4, 0.5, max_depth, leaf_max)
    assert t.node_count == nodes
    assert abs(t.total_mass[0] - root_mass) <= 1e-12 * root_mass   # (the oracle's root mass is a plain fp64 sum)
    assert t.total_mass[0] == math.fsum(ic["mass"].astype(np.float64))


# ---- trees whose shape can be counted by hand ----------------------------------------------------------------------------
def bases(counts, odd, max_depth):
    """level_base of both numberings from hand-counted nodes and odd sibling groups per level"""
    plain, aligned = [0], [0, 2]
    for L in range(max_depth + 1):
        plain.append(plain[-1] + counts[L])
        if L >= 1:
            aligned.append(aligned[-1] + counts[L] + odd[L])
    pad = lambda b: b + [b[-1]] * (tr.LEVELS - len(b))
    return pad(plain), pad(aligned)


def test_level_base_eight_corners(oracle):
    c = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    t = tr.RefTree(oracle, sr.bodies(c[:, 0], c[:, 1], c[:, 2]), 20, 1)
    # the root and its eight one-body children: one sibling group, of even size
    plain, aligned = bases([1, 8] + [0] * 19, [0] * 21, 20)
    assert t.level_base_plain == plain and t.level_base_aligned == aligned
    assert aligned[:3] == [0, 2, 10] and plain[:3] == [0, 1, 9]
    assert t.children[0].tolist() == list(range(1, 9))   # body (sx, sy, sz) in octant 4 [sx > 0] + 2 [sy > 0] + [sz > 0]
    assert t.particle_index[1:].tolist() == list(range(8))


def test_level_base_lattice(oracle):
    t = tr.RefTree(oracle, lattice(16), 20, 1)
    # 16^3 = 8^4 bodies, one per cell of level 4: every internal node has 8 children, no group is odd
    counts = [1, 8, 64, 512, 4096] + [0] * 16
    plain, aligned = bases(counts, [0] * 21, 20)
    assert t.level_counts == counts and t.odd_groups == [0] * 21
    assert t.level_base_plain == plain and t.level_base_aligned == aligned
    assert aligned[:6] == [0, 2, 10, 74, 586, 4682]
    assert np.all((t.children[t.level < 4] >= 0).sum(1) == 8) and t.is_leaf[t.level == 4].all()


def test_level_base_lattice_plus_one(oracle):
    # one more body in the cell of the lattice body nearest the centre, an eighth of a level-4 cell away from it on
    # every axis: the two share their level-5 cell's parent and part at level 6 (cells of 1/32: 1/64 apart puts them
    # in different level-6 cells) -> that level-4 leaf becomes a chain 4 -> 5 (one child: an odd group) -> 6 (two)
    d = 2.0 / 16 / 8
    base = 0.5 / 16 * 2.0
    t = tr.RefTree(oracle, lattice(16, extra=[(base + d, base + d, base + d)]), 20, 1)
    lv = [int(c) for c in t.level_counts]
    deep = [L for L in range(21) if lv[L]]
    assert lv[:5] == [1, 8, 64, 512, 4096]
    # below level 4: a chain of one-child levels, then the level where the two part (two leaves)
    chain = lv[5:deep[-1]]
    assert all(c == 1 for c in chain) and lv[deep[-1]] == 2
    odd = [0] * 21
    for L in range(5, deep[-1]):
        odd[L] = 1
    plain, aligned = bases(lv, odd, 20)
    assert t.odd_groups == odd
    assert t.level_base_plain == plain and t.level_base_aligned == aligned
    assert t.node_count == 4681 + len(chain) + 2
    assert aligned[tr.LEVELS - 1] == plain[tr.LEVELS - 1] + 1 + len(chain)   # the root's hole + one per chain level


@pytest.mark.parametrize("max_depth", [3, 10, 11, 21])
def test_level_base_two_coincident_bodies(oracle, max_depth):
    ic = sr.bodies([0.25, 0.25], [-0.5, -0.5], [0.125, 0.125])
    t = tr.RefTree(oracle, ic, max_depth, 1)
    # one node per level, each the only child of the one above (every sibling group is odd), the last one a leaf of two
    counts = [1] * (max_depth + 1)
    plain, aligned = bases(counts, [0] + [1] * max_depth, max_depth)
    assert t.level_base_plain == plain and t.level_base_aligned == aligned
    assert aligned[: max_depth + 2] == [2 * L for L in range(max_depth + 2)]
    assert t.node_count == max_depth + 1 and t.is_leaf.tolist() == [False] * max_depth + [True]
    assert t.count.tolist() == [2] * (max_depth + 1) and t.particle_index[-1] == 0
    assert np.array_equal(t.center_of_mass[-1], [0.25, -0.5, 0.125])


def test_massless_nodes_sit_at_the_origin(oracle):
    ic = cloud(64, seed=5)
    ic["mass"][:] = 0.0
    ic["mass"][3] = 2.0
    t = tr.RefTree(oracle, ic, 20, 1)
    zero = t.total_mass == 0
    assert zero.any() and np.all(t.center_of_mass[zero] == 0)
    assert np.array_equal(t.center_of_mass[0], [float(ic["pos_x"][3]), float(ic["pos_y"][3]), float(ic["pos_z"][3])])


def test_fp32_steps():
    a = np.array([1.0, 1.0, -1.0, 0.0, 1e-45], F)
    assert tr.fp32_steps(a, a.astype(np.float64)).tolist() == [0] * 5
    assert tr.fp32_steps(np.nextafter(a, F(np.inf)), a.astype(np.float64)).tolist() == [1] * 5
    assert tr.fp32_steps(np.array([0.0], F), np.array([-0.0])).tolist() == [0]
    assert tr.fp32_steps(np.array([1.0], F), np.array([1.0 + 3 * 2.0 ** -24])).tolist() == [2]
