"""A plain reference octree for the Barnes-Hut build (csrc/barnes_hut.hip), in numpy and fp64, without a GPU.

THE NODE RULE (the only statement of the topology in the suite that does not come from the build under test):
  * the bodies are taken in the order  sort_ref.stable_order(keys)  of their Morton keys on the root cube of
    oracle_bh_root (keys: oracle_bh_keys through sort_ref.tree_keys);
  * a node at level L is a run of sorted bodies that share the 3L-bit key prefix and whose PARENT run (the run of the
    3(L-1)-bit prefix that contains it) holds more than leaf_max bodies; the root is the run of all bodies;
  * a node is a leaf if it holds at most leaf_max bodies or sits at max_depth.
Nodes are numbered level by level, by ascending key inside a level (the order of BarnesHutTree.copyNodesToHost); the
children of a node are consecutive and sit in the slot of their octant (the three key bits of their level).

The sorted bits.  A tree of max_depth > 10 sorts the leading 3 max_depth bits of the 63-bit key (sort_ref.tree_keys);
a tree of max_depth <= 10 holds 30-bit keys and sorts ALL 30 of them, whatever its depth (tree_build_packed: first_bit
0, 30 key bits), so its order -- and with it the particle_index of a deepest leaf -- is that of the depth-10 keys.

Monopoles.  total_mass = sum m and center_of_mass = sum m x / sum m of the node's bodies, the products m x exact in
fp64 (24 x 24 bits), the sums in x87 extended precision (64-bit mantissa: a sum of c terms is within c 2^-64 of the
exact one relative to sum |m x|, 2^11 times closer than one fp64 rounding -- test_tree_cpu.py holds it to math.fsum),
the quotient in extended precision, rounded once to fp64.  A node whose mass sum is 0 has com (0, 0, 0).

WHAT A BUILD MAY DIFFER BY (the bounds test_tree_gpu.py asserts; nothing here is fitted to what the kernels give):
  * prefix path (n <= 1,572,864 bodies): the double-double prefix difference is exact to ~1e-30 and the quotient is one
    fp64 division, so the fp64 value the record is rounded from is the reference's up to 2^-53 relative: the record is
    the fp32 rounding of the reference or, at a rounding boundary, its fp32 neighbour (within_one_fp32_step).
  * bottom-up path (larger trees): every addition rounds once.  A leaf of c bodies adds c - 1 times (its products are
    exact); an internal node re-forms each child's sum m x as com x mass (the child's division + this product: 2
    roundings), adds up to 8 of them (7 additions) and divides (1): at most 10 roundings per level of height, on
    numerator and denominator alike.  With K = (largest leaf - 1) + 10 max_depth roundings on the longest path, to
    first order in u = 2^-53
        |com - ref| <= 2 K u  sum m |x| / sum m      (numerator and denominator, K each)
        |mass - ref| <= K u sum m
    before the record's rounding to fp32, which adds half an fp32 ulp of the value (bottom_up_bound).
"""
import math

import numpy as np

import quadrupole_ref as qr
import sort_ref as sr

F = np.float32
LD = np.longdouble
LEVELS = 24  # NBODY_HIP_TREE_LEVELS: level_base entries, the last one repeated
U64 = 2.0 ** -53
EXTENDED = np.finfo(LD).nmant >= 63


def sort_keys(oracle, ic, max_depth):
    """(keys the tree sorts, their width in bits)"""
    d = max(max_depth, 10)
    return sr.tree_keys(oracle, ic, d), 3 * d


def _deinterleave(prefix, level):
    """cell coordinates (x, y, z) of a 3 level-bit key prefix: bit b of x / y / z at key bit 3 b + 2 / + 1 / + 0"""
    q = [np.zeros(prefix.size, np.int64) for _ in range(3)]
    p = prefix.astype(np.uint64)
    for b in range(level):
        for a in range(3):
            q[a] |= (((p >> np.uint64(3 * b + (2 - a))) & np.uint64(1)) << np.uint64(b)).astype(np.int64)
    return q


def _segment_sums(values, first, last):
    """sums of values[first[k]:last[k]] (disjoint ascending ranges) in extended precision; values: (n,) fp64"""
    if not EXTENDED:  # no 80-bit long double on this machine: correctly rounded sums, one node at a time
        return np.array([math.fsum(values[a:b]) for a, b in zip(first, last)], LD)
    pad = np.concatenate([values.astype(LD), np.zeros(1, LD)])
    idx = np.stack([first, last], 1).ravel()
    return np.add.reduceat(pad, idx)[::2]


class RefTree:
    def __init__(self, oracle, ic, max_depth=20, leaf_max=1):
        x, y, z, m = (np.ascontiguousarray(ic[k], F) for k in ("pos_x", "pos_y", "pos_z", "mass"))
        n = x.size
        self.n, self.max_depth, self.leaf_max = n, max_depth, leaf_max
        keys, kbits = sort_keys(oracle, {"pos_x": x, "pos_y": y, "pos_z": z}, max_depth)
        self.order = sr.stable_order(keys)
        sk = keys[self.order]
        self.pos_sorted = np.stack([x, y, z], 1)[self.order]
        self.m_sorted = m[self.order]
        centre, half = oracle.bh_root(x, y, z)
        lo, _, _ = sr.root_cube(oracle, x, y, z)
        self.root_center, self.root_half = [F(c) for c in centre], F(half)

        firsts, lasts, prefixes, parents, odd = [], [], [], [], [0]
        big_above = None  # per body: the run of the level above that holds it has more than leaf_max bodies
        for L in range(max_depth + 1):
            pre = sk >> np.uint64(kbits - 3 * L) if L else np.zeros(n, np.uint64)
            head = np.ones(n, bool)
            head[1:] = pre[1:] != pre[:-1]
            starts = np.flatnonzero(head)
            size = np.diff(np.append(starts, n))
            rid = np.cumsum(head) - 1
            node_head = head & big_above if L else head
            f = np.flatnonzero(node_head)
            if f.size == 0:
                break
            firsts.append(f)
            lasts.append(f + size[rid[f]])
            prefixes.append(pre[f])
            if L:  # the parent of every node: the node of the level above whose range holds its first body
                par = np.searchsorted(firsts[L - 1], f, "right") - 1
                assert np.all(lasts[L - 1][par] >= lasts[L]) and np.all(lasts[L - 1][par] - firsts[L - 1][par] > leaf_max)
                parents.append(par)
                group = np.bincount(par, minlength=firsts[L - 1].size)
                odd.append(int((group & 1).sum()))  # sibling groups of level L of odd size
            big_above = (size > leaf_max)[rid]
        levels = len(firsts)
        counts = [f.size for f in firsts]
        self.level_counts = counts + [0] * (max_depth + 1 - levels)
        base = np.concatenate([[0], np.cumsum(self.level_counts)]).astype(np.int64)
        self.level = np.repeat(np.arange(levels), counts)
        self.first = np.concatenate(firsts)
        self.last = np.concatenate(lasts)
        self.count = self.last - self.first
        self.is_leaf = (self.count <= leaf_max) | (self.level == max_depth)
        nn = self.first.size
        self.children = np.full((nn, 8), -1, np.int64)
        for L in range(1, levels):
            child = base[L] + np.arange(counts[L])
            octant = (prefixes[L] & np.uint64(7)).astype(np.int64)
            self.children[base[L - 1] + parents[L - 1], octant] = child
        has_child = (self.children >= 0).any(1)
        assert np.array_equal(has_child, ~self.is_leaf)
        self.particle_index = np.where(self.is_leaf, self.order[self.first], -1)
        # the two numberings (tree_fill_kernel): plain = running node counts; even-aligned: the root's pair holds a
        # hole, then every level starts where the one above ends, each odd sibling group padded by one id
        self.odd_groups = odd + [0] * (max_depth + 1 - levels)
        self.level_base_plain = self._pad_levels(base)
        al = [0, 2]
        for L in range(1, max_depth + 1):
            al.append(al[L] + self.level_counts[L] + self.odd_groups[L])
        self.level_base_aligned = self._pad_levels(al)
        # geometry in fp32 as nbody_hip_tree_copy_nodes forms it: half = ldexp(root half, -level), centre = lo + (cell
        # + 0.5) (2 half)
        self.half_size = np.ldexp(self.root_half, -self.level).astype(F)
        self.center = np.empty((nn, 3), F)
        for L in range(levels):
            q = _deinterleave(prefixes[L], L)
            h2 = F(2.0) * self.half_size[base[L]]
            for a in range(3):
                self.center[base[L]:base[L + 1], a] = F(lo[a]) + (q[a].astype(F) + F(0.5)) * h2
        # monopoles
        m64 = self.m_sorted.astype(np.float64)
        p64 = self.pos_sorted.astype(np.float64)
        mass = np.empty(nn, LD)
        mx = np.empty((nn, 3), LD)
        self.abs_mx = np.empty((nn, 3))  # sum m |x|: the scale of the error bounds
        for L in range(levels):
            s = slice(base[L], base[L + 1])
            mass[s] = _segment_sums(m64, firsts[L], lasts[L])
            for a in range(3):
                prod = m64 * p64[:, a]  # exact
                mx[s, a] = _segment_sums(prod, firsts[L], lasts[L])
                self.abs_mx[s, a] = np.add.reduceat(np.append(np.abs(prod), 0.0), np.stack([firsts[L], lasts[L]], 1).ravel())[::2]
        self.total_mass = mass.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            com = mx / mass[:, None]
        self.center_of_mass = np.where((mass > 0)[:, None], com, LD(0)).astype(np.float64)
        self._moments = None

    def _pad_levels(self, base):
        b = [int(v) for v in base[: self.max_depth + 2]]
        return b + [b[-1]] * (LEVELS - len(b))

    @property
    def node_count(self):
        return self.first.size

    def level_base(self, aligned):
        return self.level_base_aligned if aligned else self.level_base_plain

    def moments(self):
        """fp64 (M, c, S[6]) of quadrupole_ref.node_moments over this tree's own ranges"""
        if self._moments is None:
            self._moments = qr.node_moments(self.first, self.last, self.pos_sorted, self.m_sorted)
        return self._moments

    def bottom_up_roundings(self):
        """K of the header: fp64 roundings on the longest path from a body to the root of a bottom-up build"""
        return int(self.count[self.is_leaf].max()) - 1 + 10 * self.max_depth

    def bottom_up_bound(self, got_com, got_mass):
        """(bound on |com - ref| (nodes, 3), bound on |mass - ref| (nodes,)) of the header for records got_*"""
        k = self.bottom_up_roundings()
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = np.where(self.total_mass[:, None] > 0, self.abs_mx / self.total_mass[:, None], 0.0)
        half_ulp = lambda got, ref: 0.5 * np.spacing(np.maximum(np.abs(got), np.abs(ref).astype(F)).astype(F)).astype(np.float64)
        return (2 * k * U64 * scale + half_ulp(got_com, self.center_of_mass),
                k * U64 * self.total_mass + half_ulp(got_mass, self.total_mass))


def fp32_steps(got, ref):
    """how many fp32 values lie between the record `got` (fp32) and the fp32 rounding of `ref` (fp64): 0 = it IS the
    rounding, 1 = its neighbour.  Works on the order-preserving integer image of the floats (+0 and -0 coincide)."""
    def image(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(image(got) - image(np.asarray(ref, np.float64).astype(F)))


def within_one_fp32_step(got, ref):
    return fp32_steps(got, ref) <= 1


# ---- an exported tree against the reference ------------------------------------------------------------------------------
def check_nodes(ref, nodes, bottom_up=False, tag=""):
    """BarnesHutTree.copyNodesToHost() (`nodes`, the OctreeNode records) against `ref`, node by node: counts, leaf flags,
    particle_index, the eight child slots and half_size exactly; center to the atol of test_tree_structure; total_mass and
    center_of_mass to the header's criterion of the monopole path the build took.  Returns what was measured:
    {"steps": fp32 values between a record and the rounded reference, worst over the nodes (prefix path),
     "margin": worst |record - ref| / bound (bottom-up path)}."""
    assert len(nodes) == ref.node_count, f"{tag}: {len(nodes)} nodes against the reference's {ref.node_count}"
    for name, want in (("particle_count", ref.count), ("is_leaf", ref.is_leaf), ("particle_index", ref.particle_index),
                       ("children", ref.children)):
        got = np.asarray(nodes[name])
        bad = np.flatnonzero((got != want).reshape(len(nodes), -1).any(1))
        assert bad.size == 0, (f"{tag}: {name} differs at {bad.size} nodes, first {bad[0]} (level {ref.level[bad[0]]}, bodies "
                               f"[{ref.first[bad[0]]}, {ref.last[bad[0]]})): {got[bad[0]]} against {want[bad[0]]}")
    assert np.array_equal(nodes["half_size"], ref.half_size), f"{tag}: half_size"
    assert np.allclose(nodes["center"], ref.center, atol=1e-6), f"{tag}: center"
    mass, com = np.asarray(nodes["total_mass"]), np.asarray(nodes["center_of_mass"])
    out = {"steps": 0, "margin": 0.0}
    if bottom_up:
        b_com, b_mass = ref.bottom_up_bound(com, mass)
        e_com, e_mass = np.abs(com - ref.center_of_mass), np.abs(mass - ref.total_mass)
        out["margin"] = float(max((e_com / b_com).max(), (e_mass / b_mass).max()))
        print(f"{tag}: bottom-up monopoles, K = {ref.bottom_up_roundings()} roundings, worst |record - ref| / bound = "
              f"{out['margin']:.3f}", flush=True)
        assert np.all(e_mass <= b_mass), f"{tag}: total_mass beyond the bottom-up bound at {np.flatnonzero(e_mass > b_mass)[:8]}"
        assert np.all(e_com <= b_com), f"{tag}: center_of_mass beyond the bottom-up bound at {np.flatnonzero((e_com > b_com).any(1))[:8]}"
    else:
        s_mass, s_com = fp32_steps(mass, ref.total_mass), fp32_steps(com, ref.center_of_mass)
        out["steps"] = int(max(s_mass.max(), s_com.max()))
        out["neighbours"] = int((s_mass > 0).sum() + (s_com > 0).sum())
        print(f"{tag}: prefix monopoles, {len(nodes)} nodes, worst distance to the rounded reference {out['steps']} fp32 "
              f"step(s), {out['neighbours']} of {4 * len(nodes)} values not the rounding itself", flush=True)
        assert np.all(s_mass <= 1), f"{tag}: total_mass not the rounded reference at {np.flatnonzero(s_mass > 1)[:8]}"
        assert np.all(s_com <= 1), f"{tag}: center_of_mass not the rounded reference at {np.flatnonzero((s_com > 1).any(1))[:8]}"
    return out


def check_moments(ref, mom, tag=""):
    """BarnesHutTree.copyMomentsToHost() against the reference's second moments, under the criterion of
    test_moments_against_bodies (err <= 4e-7 tr S + 1e-30); the moments of a one-body node are exactly 0"""
    mom = np.asarray(mom, np.float64)
    _, _, S = ref.moments()
    assert mom.shape == S.shape, f"{tag}: {mom.shape} moments against {S.shape}"
    trace = S[:, :3].sum(1)
    err = np.abs(mom - S).max(1)
    worst = float((err / np.maximum(trace, 1e-300))[trace > 0].max()) if (trace > 0).any() else 0.0
    print(f"{tag}: second moments, worst |S - S_ref| / tr S = {worst:.3e}", flush=True)
    assert np.all(err <= 4e-7 * trace + 1e-30), f"{tag}: moments off at {np.flatnonzero(err > 4e-7 * trace + 1e-30)[:8]}"
    assert np.all(mom[ref.count == 1] == 0.0), f"{tag}: one-body nodes with non-zero moments"
    return worst
