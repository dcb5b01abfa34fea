"""fp64 restatement of the Barnes-Hut walk at multipole order 1 and 2 (nbody_hip_tree_set_multipole_order) for the tests.

It walks the EXPORTED tree (BarnesHutTree.copyNodesToHost + sorted_indices_) and takes every opening decision in fp32
exactly as the kernel forms it: dx = fl(com - x) from the node's fp32 record, d^2 = fma(dz, dz, fma(dy, dy, dx dx))
(potential_ref.fp32_dist2), h = fl(d^2 + eps^2), accept  fl((2 half)^2) < fl(theta^2 h).  Leaves interact body by body
(the body itself skipped; with eps^2 < 1e-12 coincident bodies too).  An accepted internal node is evaluated in fp64
with its mass M, centre c and second moment S computed FROM ITS BODIES (node_moments), not from the exported moments,
so a comparison checks the build and the walk together:
  a   = G [ M d h^-3/2 - 3 S d h^-5/2 - 3/2 tr(S) d h^-5/2 + 15/2 (d^T S d) d h^-7/2 ]      (order 2; order 1: M d h^-3/2)
  phi = -G [ M h^-1/2 + 3/2 (d^T S d) h^-5/2 - 1/2 tr(S) h^-3/2 ]
with d = c - x, h = |d|^2 + eps^2 (fp64).  The walk is a vectorised frontier over batches of targets.
"""
import numpy as np

from potential_ref import fp32_dist2


def node_ranges(nodes):
    """[first, last) of every exported node in the Morton order (children in octant order = key order)"""
    n_nodes = len(nodes)
    cnt = nodes["particle_count"].astype(np.int64)
    ch = nodes["children"].astype(np.int64)
    first = np.zeros(n_nodes, np.int64)
    frontier = np.array([0], np.int64)
    while frontier.size:
        c = ch[frontier]
        valid = c >= 0
        cc = np.where(valid, cnt[np.maximum(c, 0)], 0)
        off = np.cumsum(cc, axis=1) - cc
        f = first[frontier][:, None] + off
        first[c[valid]] = f[valid]
        frontier = c[valid]
    return first, first + cnt


def node_moments(first, last, pos_sorted, m_sorted, chunk=1 << 22):
    """fp64 (M, c[3], S[6] = xx yy zz xy xz yz) of every node from its bodies (two passes: centre, then S)"""
    pos = np.asarray(pos_sorted, np.float64)
    m = np.asarray(m_sorted, np.float64)
    n_nodes = len(first)
    M = np.zeros(n_nodes)
    c = np.zeros((n_nodes, 3))
    S = np.zeros((n_nodes, 6))
    cnt = last - first
    k0 = 0
    while k0 < n_nodes:  # chunks of nodes holding about `chunk` body entries
        csum = np.cumsum(cnt[k0:])
        k1 = k0 + max(1, int(np.searchsorted(csum, chunk)))
        k1 = min(k1, n_nodes)
        lens = cnt[k0:k1]
        starts = np.cumsum(lens) - lens
        idx = np.arange(lens.sum()) - np.repeat(starts, lens) + np.repeat(first[k0:k1], lens)
        seg = starts
        mb = m[idx]
        Mk = np.add.reduceat(mb, seg)
        with np.errstate(invalid="ignore", divide="ignore"):
            ck = np.stack([np.add.reduceat(mb * pos[idx, a], seg) for a in range(3)], 1) / Mk[:, None]
        ck = np.where(Mk[:, None] > 0, ck, 0.0)
        dev = pos[idx] - np.repeat(ck, lens, axis=0)
        pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
        Sk = np.stack([np.add.reduceat(mb * dev[:, a] * dev[:, b], seg) for a, b in pairs], 1)
        M[k0:k1], c[k0:k1], S[k0:k1] = Mk, ck, Sk
        k0 = k1
    return M, c, S


def node_eval(d, h, M, S, order):
    """(acceleration / G, phi / -G) of accepted nodes: d (k, 3), h (k,), M (k,), S (k, 6); fp64"""
    inv = 1.0 / np.sqrt(h)
    i3 = inv ** 3
    a = (M * i3)[:, None] * d
    phi = M * inv
    if order == 2:
        Sd = np.stack([S[:, 0] * d[:, 0] + S[:, 3] * d[:, 1] + S[:, 4] * d[:, 2],
                       S[:, 3] * d[:, 0] + S[:, 1] * d[:, 1] + S[:, 5] * d[:, 2],
                       S[:, 4] * d[:, 0] + S[:, 5] * d[:, 1] + S[:, 2] * d[:, 2]], 1)
        dsd = (d * Sd).sum(1)
        tr = S[:, 0] + S[:, 1] + S[:, 2]
        i5, i7 = i3 * inv * inv, i3 * inv ** 4
        a = a - 3.0 * i5[:, None] * Sd + (7.5 * dsd * i7 - 1.5 * tr * i5)[:, None] * d
        phi = phi + 1.5 * dsd * i5 - 0.5 * tr * i3
    return a, phi


class Restatement:
    """the walk over one exported tree: Restatement(tree, ic).walk(targets, theta, G, eps, order)"""

    def __init__(self, nodes, sorted_indices, pos, mass):
        self.nodes = nodes
        self.order = np.asarray(sorted_indices, np.int64)
        self.pos32 = np.asarray(pos, np.float32)
        self.m = np.asarray(mass, np.float64)
        self.first, self.last = node_ranges(nodes)
        self.pos_sorted = self.pos32[self.order]
        self.M, self.c, self.S = node_moments(self.first, self.last, self.pos_sorted, self.m[self.order])
        self.rank = np.empty(len(self.order), np.int64)
        self.rank[self.order] = np.arange(len(self.order))
        self.com32 = np.asarray(nodes["center_of_mass"], np.float32)
        h = np.asarray(nodes["half_size"], np.float32)
        size = (np.float32(2) * h).astype(np.float32)
        self.size2 = (size * size).astype(np.float32)
        self.leaf = np.asarray(nodes["is_leaf"], bool)
        self.children = nodes["children"].astype(np.int64)

    def interaction_counts(self, targets, theta, eps):
        return self.walk(targets, theta, 1.0, eps, 1, counts=True)

    def dist2(self, dx, dy, dz):
        """the fp32 |d|^2 every decision is taken on (a subclass may state it more strictly: walk_edge_ref.py)"""
        return fp32_dist2(dx, dy, dz)

    def walk(self, targets, theta, G, eps, order, batch=2048, counts=False, detail=None):
        """(acc (k, 3), phi (k,)) of the bodies `targets` (original indices); counts=True: per target, the number of
        accepted internal nodes and of leaf bodies it interacts with (its interaction list's size).  detail: a dict
        that receives "tested" = (target slot, internal node, accepted) of every opening test taken, "counts", and
        "abs_acc" / "abs_phi" = sum of |term| / G per target (the scale of a sum whose terms cancel)"""
        targets = np.asarray(targets, np.int64)
        theta2 = np.float32(np.float32(theta) * np.float32(theta))
        eps2 = np.float32(np.float32(eps) * np.float32(eps))
        guard = float(eps2) < 1e-12
        acc = np.zeros((len(targets), 3))
        phi = np.zeros(len(targets))
        cnt = np.zeros((len(targets), 2), np.int64)
        mag = np.zeros((len(targets), 2))
        tested = []
        for b0 in range(0, len(targets), batch):
            tb = np.arange(b0, min(b0 + batch, len(targets)))
            ti = np.zeros(len(tb), np.int64) + tb  # target slot
            nd = np.zeros(len(tb), np.int64)       # node (the root)
            while ti.size:
                x32 = self.pos32[targets[ti]]
                leaf = self.leaf[nd]
                # leaves: body by body
                li, ln = ti[leaf], nd[leaf]
                if li.size:
                    lens = self.last[ln] - self.first[ln]
                    rep_t = np.repeat(li, lens)
                    starts = np.cumsum(lens) - lens
                    q = np.arange(lens.sum()) - np.repeat(starts, lens) + np.repeat(self.first[ln], lens)
                    body = self.order[q]
                    ok = body != targets[rep_t]
                    d32 = (self.pos32[body] - self.pos32[targets[rep_t]]).astype(np.float32)
                    r2 = self.dist2(d32[:, 0], d32[:, 1], d32[:, 2]).astype(np.float64)
                    if guard:
                        ok &= r2 > 0
                    d = d32.astype(np.float64)
                    h = r2 + float(eps2)
                    with np.errstate(divide="ignore"):
                        inv = np.where(ok, 1.0 / np.sqrt(np.where(ok, h, 1.0)), 0.0)
                    f = self.m[body] * inv ** 3
                    for a in range(3):
                        acc[:, a] += np.bincount(rep_t, f * d[:, a], minlength=len(targets))
                    phi += np.bincount(rep_t, self.m[body] * inv, minlength=len(targets))
                    cnt[:, 1] += np.bincount(rep_t[ok], minlength=len(targets))
                    if detail is not None:
                        mag[:, 0] += np.bincount(rep_t, np.abs(f) * np.sqrt((d * d).sum(1)), minlength=len(targets))
                        mag[:, 1] += np.bincount(rep_t, self.m[body] * inv, minlength=len(targets))
                ti, nd, x32 = ti[~leaf], nd[~leaf], x32[~leaf]
                if not ti.size:
                    break
                d32 = (self.com32[nd] - x32).astype(np.float32)
                d2 = self.dist2(d32[:, 0], d32[:, 1], d32[:, 2])
                dist2 = (d2 + eps2).astype(np.float32)
                far = self.size2[nd] < (theta2 * dist2).astype(np.float32)
                if detail is not None:
                    tested.append((ti, nd, far))
                ai, an = ti[far], nd[far]
                if ai.size:
                    d = self.c[an] - self.pos32[targets[ai]].astype(np.float64)
                    h = (d * d).sum(1) + float(eps2)
                    a_n, p_n = node_eval(d, h, self.M[an], self.S[an], order)
                    for a in range(3):
                        acc[:, a] += np.bincount(ai, a_n[:, a], minlength=len(targets))
                    phi += np.bincount(ai, p_n, minlength=len(targets))
                    cnt[:, 0] += np.bincount(ai, minlength=len(targets))
                    if detail is not None:
                        mag[:, 0] += np.bincount(ai, np.sqrt((a_n * a_n).sum(1)), minlength=len(targets))
                        mag[:, 1] += np.bincount(ai, np.abs(p_n), minlength=len(targets))
                oi, on = ti[~far], nd[~far]
                ch = self.children[on]
                valid = ch >= 0
                ti = np.repeat(oi, valid.sum(1))
                nd = ch[valid]
        if detail is not None:
            cat = lambda k, t: np.concatenate([e[k] for e in tested]).astype(t) if tested else np.zeros(0, t)
            detail.update(tested=(cat(0, np.int64), cat(1, np.int64), cat(2, bool)), counts=cnt, abs_acc=mag[:, 0],
                          abs_phi=mag[:, 1])
        if counts:
            return cnt
        return G * acc, -G * phi


def single_node(d, eps, M, S, order):
    """a_node and phi_node of ONE node (fp64): d (k, 3) = c - x, S (6,) -- the header's formulas"""
    d = np.atleast_2d(np.asarray(d, np.float64))
    h = (d * d).sum(1) + eps * eps
    a, p = node_eval(d, h, np.full(len(d), float(M)), np.tile(np.asarray(S, np.float64), (len(d), 1)), order)
    return a, -p


def moments_of(pos, m):
    """fp64 (M, c, S[6]) of one set of bodies"""
    pos = np.asarray(pos, np.float64)
    m = np.asarray(m, np.float64)
    M = m.sum()
    c = (m[:, None] * pos).sum(0) / M
    e = pos - c
    S = np.array([(m * e[:, a] * e[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))])
    return M, c, S
