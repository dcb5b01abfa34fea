"""The opening decision of the Barnes-Hut walks (csrc/barnes_hut.hip: bh_traverse_kernel, bh_traverse_pair_kernel,
bh_field_kernel) stated exactly, and the search for the cases that sit on its edge.

THE DECISION, in fp32, every operation rounded once:
    dx, dy, dz = fl(com - p)                       (per axis)
    d2         = fma(dz, dz, fma(dy, dy, fl(dx dx)))
    dist2      = fl(d2 + eps2),  eps2 = fl(eps eps)
    theta2     = fl(theta theta)
    size2      = fl(fl(2 h) fl(2 h))
    far  <=>  size2 < fl(theta2 dist2)
The scalar routines (fma_exact, dist2_exact, decide) form every fma as a fractions.Fraction and round it ONCE
(round32); the vectorised fma32 goes through fp64, where the product is exact and the sum is repaired wherever its
rounding to fp64 landed on a tie of fp32 (the only place a second rounding can differ from a single one);
test_walk_edges_cpu.py holds fma32 to fma_exact on planted double-rounding inputs.

EdgeRestatement is quadrupole_ref.Restatement with that distance, and walk_detail() adds per target the internal
nodes tested and accepted, the leaf bodies used, the scale of its sums, and per wave (64 consecutive sorted positions
counted from the start of the walked range) the children of every sibling group popped, + 1 for the root: what
stats()["nodes_visited"] and the visit histogram of the kernels count.

THE POPULATION (population): about 600 bodies in 12 clumps on the binary lattice Z / 64, so that every coordinate
difference is exact; THE CASES (theta_cases): for every (children of the parent 1..8, rank among them) with an internal
child, a node and a target outside it, and the two neighbouring fp32 values of theta between which that one decision
-- and no other of the target -- changes; point_cases: points at which the field walk meets fl(theta2 dist2) == size2.
All cases are found on an EXPORTED node table (BarnesHutTree.copyNodesToHost, or node_table() of tree_ref.RefTree
without a GPU), never on positions alone: a record may be the fp32 neighbour of the reference centre of mass.
"""
from fractions import Fraction

import numpy as np

import quadrupole_ref as qr

F = np.float32
SEED = 1
CLUMPS, PER_CLUMP, WIDTHS = 12, 50, (4, 16, 64, 200)
MARGIN = 1e-3           # what a case's two decisions change of its target's force and phi, at least (100 x TOL)
CANCEL = 16.0           # a sum with sum |terms| > CANCEL |sum| is measured on sum |terms| / CANCEL
UNIT_REPLICAS = 16      # case nodes of at most n / 16 bodies (a unit of the split walk at 16 replicas) come first
GOOD = 3e-3             # the search for a combination stops at a case with this margin
COMBOS = [(c, r) for c in range(1, 9) for r in range(c)]


# ---- exact fp32 arithmetic ------------------------------------------------------------------------------------------
def round32(x):
    """the fp32 nearest to the Fraction x, ties to even: ONE rounding (normal and subnormal range, no overflow)"""
    x = Fraction(x)
    if x == 0:
        return F(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                      # 2^e <= a < 2^(e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)          # the spacing of fp32 there
    k = round(a / q)                                # Fraction.__round__: half to even
    v = float(k * q)                                # exact: k <= 2^24
    assert v < 3.5e38
    return F(-v if x < 0 else v)


def fma_exact(a, b, c):
    """fp32 fma(a, b, c): the exact value, rounded once"""
    return round32(Fraction(float(F(a))) * Fraction(float(F(b))) + Fraction(float(F(c))))


def fma32(a, b, c):
    """fma_exact on arrays.  a b is exact in fp64 (48 bits); s = fl64(a b + c) and its error e (TwoSum) are exact.  The
    fp32 rounding of s is that of a b + c unless s is a tie of fp32 (low 29 bits 0x10000000) that the exact sum misses
    (e != 0): there s moves one fp64 step towards the exact sum, off the tie."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    tie = (np.atleast_1d(s).view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)
    tie = tie.reshape(np.shape(s)) & (e != 0)
    s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def dist2_fma32(dx, dy, dz):
    dx, dy, dz = (np.asarray(v, F) for v in (dx, dy, dz))
    return fma32(dz, dz, fma32(dy, dy, (dx * dx).astype(F)))


def dist2_exact(com, p, eps):
    """(d2, dist2) of the header for one centre of mass and one point, through Fractions"""
    d = [round32(Fraction(float(F(c))) - Fraction(float(F(x)))) for c, x in zip(com, p)]
    d2 = fma_exact(d[2], d[2], fma_exact(d[1], d[1], round32(Fraction(float(d[0])) ** 2)))
    eps2 = round32(Fraction(float(F(eps))) ** 2)
    return d2, round32(Fraction(float(d2)) + Fraction(float(eps2)))


def size2_of(half):
    s = round32(2 * Fraction(float(F(half))))
    return round32(Fraction(float(s)) ** 2)


def threshold(theta, dist2):
    theta2 = round32(Fraction(float(F(theta))) ** 2)
    return round32(Fraction(float(theta2)) * Fraction(float(dist2)))


def decide(com, half, p, theta, eps):
    """far (accepted) <=> size2 < fl(theta2 dist2)"""
    return bool(size2_of(half) < threshold(theta, dist2_exact(com, p, eps)[1]))


def next32(v, up=True):
    return np.nextafter(F(v), F(np.inf) if up else F(-np.inf))


def theta_edge(size2, dist2):
    """(largest fp32 theta in (0, 2] at which size2 < fl(theta2 dist2) is false, its successor at which it is true), or
    None when the decision does not change inside (0, 2].  The test is monotonic in theta: bisection over the bit
    patterns of the positive fp32 values."""
    far = lambda bits: bool(size2 < threshold(np.array([bits], np.uint32).view(F)[0], dist2))
    lo, hi = 1, int(np.array([2.0], F).view(np.uint32)[0])      # the smallest positive fp32, 2.0
    if far(lo) or not far(hi):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if far(mid) else (mid, hi)
    return tuple(np.array([lo, hi], np.uint32).view(F))


# ---- the population and a node table without a GPU ---------------------------------------------------------------------
def population(seed=SEED):
    rng = np.random.default_rng(seed)
    centres = rng.integers(-512, 512, (CLUMPS, 3))
    pts = []
    for k in range(CLUMPS):
        w = WIDTHS[k % len(WIDTHS)]
        pts.append(centres[k] + rng.integers(-w, w + 1, (PER_CLUMP, 3)))
    pts = np.unique(np.concatenate(pts), axis=0)
    pts = pts[rng.permutation(len(pts))]
    pos = (pts / 64.0).astype(F)
    assert np.array_equal(pos.astype(np.float64) * 64.0, pts)
    ic = {"pos_x": pos[:, 0].copy(), "pos_y": pos[:, 1].copy(), "pos_z": pos[:, 2].copy(),
          "mass": (2.0 ** rng.integers(-3, 1, len(pos))).astype(F)}
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k] = np.zeros(len(pos), F)
    return ic


def positions(ic):
    return np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)


NODE_DTYPE = np.dtype([("center_of_mass", F, 3), ("half_size", F), ("total_mass", F), ("children", np.int32, 8),
                       ("is_leaf", bool), ("particle_count", np.int32)])


def node_table(ref):
    """the fields of copyNodesToHost the walk reads, from tree_ref.RefTree, the centre of mass rounded to fp32"""
    t = np.zeros(ref.node_count, NODE_DTYPE)
    t["center_of_mass"] = ref.center_of_mass.astype(F)
    t["half_size"] = ref.half_size
    t["total_mass"] = ref.total_mass.astype(F)
    t["children"] = ref.children
    t["is_leaf"] = ref.is_leaf
    t["particle_count"] = ref.count
    return t


# ---- the restatement with the exact distance and the new outputs ------------------------------------------------------------
class Detail:
    """what walk_detail returns; per target (in the order of `targets`): acc, phi, tested, accepted, leaf_bodies,
    scale_acc, scale_phi; pairs = (slot, node, accepted) of every test; visited = the kernels' nodes_visited"""


class EdgeRestatement(qr.Restatement):
    def __init__(self, nodes, sorted_indices, pos, mass):
        super().__init__(nodes, sorted_indices, pos, mass)
        self.n = len(self.order)
        valid = self.children >= 0
        self.nchild = valid.sum(1)
        self.parent = np.full(len(nodes), -1, np.int64)
        self.sibrank = np.zeros(len(nodes), np.int64)
        rows, cols = np.nonzero(valid)
        self.parent[self.children[rows, cols]] = rows
        self.sibrank[self.children[rows, cols]] = (np.cumsum(valid, 1) - 1)[rows, cols]
        self.count = self.last - self.first
        many = self.leaf & (self.count > 1)
        pm = np.zeros(len(nodes), np.int64)         # leaves of several bodies among a node's children
        np.add.at(pm, self.parent[many & (self.parent >= 0)], 1)
        self.many_sibling = np.where(self.parent >= 0, pm[np.maximum(self.parent, 0)] - many, 0) > 0

    def dist2(self, dx, dy, dz):
        return dist2_fma32(dx, dy, dz)

    def at_points(self, points):
        """the same tree with `points` (k, 3) as further targets, indices n .. n + k - 1: no body is one of them, so
        nothing is skipped by index (the field walk)"""
        r = object.__new__(EdgeRestatement)
        r.__dict__.update(self.__dict__)
        r.pos32 = np.concatenate([self.pos32, np.asarray(points, F).reshape(-1, 3)])
        return r

    def record_centred(self):
        """the same walk with every accepted node evaluated at the centre its fp32 RECORD holds, not at the fp64 centre
        of its bodies: what a kernel that reads the record can be held to at full tolerance.  (A centre at |c| ~ 10
        seen from |d| ~ 0.05 loses 2^-24 |c| / |d| ~ 1e-5 of the term to that rounding, whatever the kernel does.)"""
        r = object.__new__(EdgeRestatement)
        r.__dict__.update(self.__dict__)
        r.c = self.com32.astype(np.float64)
        return r

    def walk_detail(self, targets, theta, G, eps, order, first=None):
        """Detail of the bodies `targets`; first: the sorted position the walked range starts at (waves are counted
        from there; None: no wave count, e.g. for points)"""
        targets = np.asarray(targets, np.int64)
        det = {}
        out = Detail()
        out.acc, out.phi = self.walk(targets, theta, G, eps, order, detail=det)
        slot, node, far = det["tested"]
        k = len(targets)
        out.pairs = det["tested"]
        out.tested = np.bincount(slot, minlength=k)
        out.accepted = np.bincount(slot[far], minlength=k)
        assert np.array_equal(out.accepted, det["counts"][:, 0])
        out.leaf_bodies = det["counts"][:, 1]
        out.scale_acc = np.maximum(np.linalg.norm(out.acc, axis=1), abs(G) * det["abs_acc"] / CANCEL)
        out.scale_phi = np.maximum(np.abs(out.phi), abs(G) * det["abs_phi"] / CANCEL)
        out.visited = None
        if first is not None:
            assert not self.leaf[0]
            wave = (self.rank[targets] - first) // 64
            assert wave.min() >= 0
            opened = np.unique(np.stack([wave[slot[~far]], node[~far]], 1), axis=0)
            out.visited = int(self.nchild[opened[:, 1]].sum()) + len(np.unique(wave))
        return out

    def decisions_of(self, detail, slot):
        """{node: accepted} of one target of a Detail"""
        s, nd, far = detail.pairs
        m = s == slot
        return dict(zip(nd[m].tolist(), far[m].tolist()))


# ---- theta edges --------------------------------------------------------------------------------------------------------
class Case:
    """node, target (original index), combo = (children of the parent, rank), eps, theta_open, theta_accept, equality
    (fl(theta_open^2 dist2) == size2), margin (what the flip changes, order 1, on the scale Detail.scale_acc / scale_phi), many_sibling"""

    def __repr__(self):
        return (f"Case(node {self.node} x{self.count}, combo {self.combo}, target {self.target}, eps {self.eps}, theta "
                f"{float(self.theta_open)!r} | {float(self.theta_accept)!r}, eq {self.equality}, margin {self.margin:.2e})")


def _estimates(r, eps, G=1.0):
    """fp64 estimate, for every (target, node), of what accepting the node instead of summing its bodies changes of the
    target's force and phi, relative to the direct sums (scale: max(|sum|, sum |terms| / CANCEL))"""
    n = r.n
    pos = r.pos32.astype(np.float64)[:n]
    ps, ms = pos[r.order], r.m[r.order]
    e2 = float(F(F(eps) * F(eps)))
    d = ps[None, :, :] - pos[:, None, :]
    h = (d * d).sum(-1) + e2
    ok = (d * d).sum(-1) > 0
    inv = np.where(ok, 1.0 / np.sqrt(np.where(ok, h, 1.0)), 0.0)
    A = (ms[None, :] * inv ** 3)[:, :, None] * d
    P = ms[None, :] * inv
    CA = np.concatenate([np.zeros((n, 1, 3)), np.cumsum(A, 1)], 1)
    CP = np.concatenate([np.zeros((n, 1)), np.cumsum(P, 1)], 1)
    mag = (ms[None, :] * inv ** 2).sum(1)
    sa = np.maximum(np.linalg.norm(CA[:, n], axis=1), mag / CANCEL)
    sp = CP[:, n]
    dn = r.c[None, :, :] - pos[:, None, :]
    hn = (dn * dn).sum(-1) + e2
    invn = 1.0 / np.sqrt(np.maximum(hn, 1e-30))
    mono_a = (r.M[None, :] * invn ** 3)[:, :, None] * dn
    mono_p = r.M[None, :] * invn
    da = np.linalg.norm(mono_a - (CA[:, r.last] - CA[:, r.first]), axis=2) / sa[:, None]
    dp = np.abs(mono_p - (CP[:, r.last] - CP[:, r.first])) / sp[:, None]
    est = np.minimum(da, dp)
    theta = np.sqrt(r.size2.astype(np.float64)[None, :] / np.maximum(hn, 1e-30))
    inside = (r.rank[:n, None] >= r.first[None, :]) & (r.rank[:n, None] < r.last[None, :])
    est[inside | (theta > 1.9) | (theta < 0.05)] = -1.0
    return est


def verify_case(r, node, target, eps, t_open, t_acc, G=1.0):
    """the reference's own statement of a case: the node is tested at both thetas, opened at one and accepted at the
    other; every other decision the two walks share is the same, and the tests only the opening walk takes are all
    below the node.  Returns the margin (order 1) or None."""
    a = r.walk_detail([target], t_open, G, eps, 1)
    b = r.walk_detail([target], t_acc, G, eps, 1)
    da, db = r.decisions_of(a, 0), r.decisions_of(b, 0)
    if da.get(node) is not False or db.get(node) is not True:
        return None
    if not set(db) <= set(da) or any(da[k] != db[k] for k in db if k != node):
        return None
    below = [k for k in da if k not in db]
    if not all(r.first[node] <= r.first[k] and r.last[k] <= r.last[node] and k != node for k in below):
        return None
    ma = np.linalg.norm(a.acc[0] - b.acc[0]) / max(a.scale_acc[0], b.scale_acc[0])
    mp = abs(a.phi[0] - b.phi[0]) / max(a.scale_phi[0], b.scale_phi[0])
    return float(min(ma, mp))


def theta_cases(r, eps, prefer_many=False, tries=8):
    """{combo: Case} on the tree of r for softening eps: per combination the (node, target) with the largest estimated
    margin that the reference confirms (verify_case) with a margin of at least MARGIN"""
    est = _estimates(r, eps)
    internal = np.flatnonzero(~r.leaf & (r.parent >= 0) & (r.count <= r.n // 2))
    found = {}
    for combo, small in [(c, s) for s in (True, False) for c in COMBOS]:
        if combo in found:
            continue
        cand = internal[(r.nchild[r.parent[internal]] == combo[0]) & (r.sibrank[internal] == combo[1])]
        if small:
            cand = cand[r.count[cand] <= r.n // UNIT_REPLICAS]
        if prefer_many and r.many_sibling[cand].any():
            cand = cand[r.many_sibling[cand]]
        if cand.size == 0:
            continue
        sub = est[:, cand]
        flat = np.argsort(-sub, axis=None, kind="stable")[:tries]
        for f in flat:
            t, k = np.unravel_index(f, sub.shape)
            if sub[t, k] < MARGIN:
                break
            node, target = int(cand[k]), int(t)
            com, half = r.com32[node], r.nodes["half_size"][node]
            d2, dist2 = dist2_exact(com, r.pos32[target], eps)
            edge = theta_edge(size2_of(half), dist2)
            if edge is None:
                continue
            margin = verify_case(r, node, target, eps, edge[0], edge[1])
            if margin is None or margin < MARGIN:
                continue
            c = Case()
            c.node, c.target, c.combo, c.eps, c.count = node, target, combo, eps, int(r.count[node])
            c.theta_open, c.theta_accept = edge
            c.dist2, c.size2 = dist2, size2_of(half)
            c.equality = bool(threshold(edge[0], dist2) == c.size2)
            c.margin, c.many_sibling = margin, bool(r.many_sibling[node])
            # the vectorised walk took these two decisions (verify_case); the Fraction routine must agree
            assert decide(com, half, r.pos32[target], edge[0], eps) is False
            assert decide(com, half, r.pos32[target], edge[1], eps) is True
            if combo not in found or c.margin > found[combo].margin:
                found[combo] = c
            if c.margin >= GOOD:
                break
    return found


def check_theta_cases(deep, cut):
    """the conditions on the cases of the two trees (deep: {eps: {combo: Case}} of the (20, 1) tree; cut: of the (4, 1)
    tree); returns (all cases, share of exact equalities)"""
    cases = [c for by_eps in (deep, cut) for found in by_eps.values() for c in found.values()]
    for c in cases:
        assert 0.0 < c.theta_open < c.theta_accept <= 2.0, c
        assert c.theta_accept == next32(c.theta_open), c
        assert c.margin >= MARGIN, c
    for eps, found in deep.items():
        assert sorted(found) == COMBOS, (eps, sorted(set(COMBOS) - set(found)))
    equal = sum(c.equality for c in cases)
    assert 4 * equal >= len(cases), (equal, len(cases))
    many = sum(c.many_sibling for found in cut.values() for c in found.values())
    assert many >= 8, many
    return cases, equal / len(cases)


# ---- point edges ----------------------------------------------------------------------------------------------------------
class PointCase:
    """node, axis, sign, theta, points (3, 3): the edge point and its two fp32 neighbours along the axis"""


def point_cases(r, theta, want=12):
    """points at which the field walk (eps = 0) finds fl(theta2 dist2) == size2 exactly: theta = 1: com -+ 2h along one
    axis, theta = 0.5: com -+ 4h, where fl(com - p) is that distance exactly; the node must be tested there, and
    accepting it instead must change the field at the point by MARGIN at least"""
    mult = {1.0: 2, 0.5: 4}[float(theta)]
    out = []
    for node in np.flatnonzero(~r.leaf & (r.parent >= 0)):
        com, half = r.com32[node], F(r.nodes["half_size"][node])
        dist = F(mult) * half
        for axis in range(3):
            for sign in (-1, 1):
                p = com.copy()
                p[axis] = F(com[axis] + F(sign) * dist)
                if F(com[axis] - p[axis]) != F(-sign) * dist:
                    continue
                d2, dist2 = dist2_exact(com, p, 0.0)
                if threshold(theta, dist2) != size2_of(half):
                    continue
                pts = np.stack([p, p, p])
                pts[1, axis], pts[2, axis] = next32(p[axis], False), next32(p[axis], True)
                rp = r.at_points(pts)
                det = rp.walk_detail(r.n + np.arange(3), theta, 1.0, 0.0, 1)
                if rp.decisions_of(det, 0).get(int(node)) is not False:
                    continue
                # what the decision is worth at the point: at the next theta the node, and it alone, is accepted
                margin = verify_case(rp, int(node), r.n, 0.0, F(theta), next32(theta))
                if margin is None or margin < MARGIN:
                    continue
                c = PointCase()
                c.margin = margin
                c.node, c.axis, c.sign, c.theta, c.points = int(node), axis, sign, float(theta), pts
                c.decisions = [rp.decisions_of(det, k).get(int(node)) for k in range(3)]
                out.append(c)
                break
            if out and out[-1].node == int(node):
                break
        if len(out) >= want:
            break
    return out


def check_point_case(nodes, c):
    """the equality of a point case, from the record alone"""
    com, half = np.asarray(nodes["center_of_mass"][c.node], F), F(nodes["half_size"][c.node])
    d2, dist2 = dist2_exact(com, c.points[0], 0.0)
    assert threshold(c.theta, dist2) == size2_of(half), (c.node, c.theta)
    assert decide(com, half, c.points[0], c.theta, 0.0) is False
