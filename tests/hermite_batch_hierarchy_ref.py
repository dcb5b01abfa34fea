"""The restatement of the ensemble HIERARCHIES (include/nbody_hip.h "ensemble HIERARCHIES") for
the tests; not a test file.

ONE program text, `_decompose`, runs the model operation by operation in the model's order on three kinds of number:

  evaluate   numpy fp64 scalars: every + - * / sqrt rounds once, nothing is fused, sums of three terms go left to right --
             what csrc/hermite_batch_hierarchy_common.h does on the device;
  bounded    pairs (value, absolute bound): the same fp64 value and, carried through every operation with u = 2^-53, a
             bound on |value - what exact arithmetic gives on the same inputs|.  For z = x op y rounded:
               +, -   bound_x + bound_y + u |z|
               *      |x| bound_y + |y| bound_x + bound_x bound_y + u |z|
               /      (bound_x + |z| bound_y) / (|y| - bound_y) + u |z|
               sqrt   sqrt(x + bound_x) - sqrt(max(x - bound_x, 0)) + 2 u sqrt(x + bound_x)
             Mechanical, valid at any depth of the tree, and fitted on nothing;
  exact      fractions.Fraction, the square roots taken to 2^-200.

The bound holds only while exact arithmetic takes the same decisions, so every decision of the bounded run is recorded
with its margin and its bound, and `clear` wants margin > CLEAR bound (CLEAR = 1e6), or a bound of 0 (an exact value),
for:  eps < 0 of every pair looked at;  the chosen a against every other candidate's, unless the two are bitwise equal,
where the index tie-break decides;  the four criteria of the resolved test (a resolved system: all four of every top
pair; an unresolved one with K >= 2: at least one criterion of one pair clearly missed).

The cases of the GPU tests are at the end."""
import math
import os
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
CLEAR = 1.0e6
NONE = 0xFFFFFFFF
MAX_N = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hermite_batch_hierarchy_states.npz")


# ---- the three kinds of number -------------------------------------------------------------------------------------------
class Bd:
    """(value, absolute bound)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = np.float64(v), float(e)

    def __add__(self, o):
        z = self.v + o.v
        return Bd(z, self.e + o.e + U * abs(float(z)))

    def __sub__(self, o):
        z = self.v - o.v
        return Bd(z, self.e + o.e + U * abs(float(z)))

    def __mul__(self, o):
        z = self.v * o.v
        return Bd(z, abs(float(self.v)) * o.e + abs(float(o.v)) * self.e + self.e * o.e + U * abs(float(z)))

    def __truediv__(self, o):
        z = self.v / o.v
        den = abs(float(o.v)) - o.e
        return Bd(z, (self.e + abs(float(z)) * o.e) / den + U * abs(float(z)) if den > 0 and np.isfinite(z) else math.inf)


def _bd_sqrt(x):
    v = max(float(x.v), 0.0) if x.v == x.v else math.nan
    hi = v + x.e
    return Bd(np.sqrt(np.float64(v)), math.sqrt(hi) - math.sqrt(max(v - x.e, 0.0)) + 2 * U * math.sqrt(hi) if hi == hi else math.inf)


def _fsqrt(q, bits=200):
    """sqrt of a non-negative Fraction to 2^-bits relative, as a Fraction"""
    if q == 0:
        return Fraction(0)
    shift = max(0, 2 * bits - (q.numerator.bit_length() - q.denominator.bit_length()) + 2)
    shift += shift & 1
    return Fraction(math.isqrt((q.numerator << shift) // q.denominator), 1 << (shift // 2))


class _Kit:
    def __init__(self, lift, sqrt, val, err):
        self.lift, self.sqrt, self.val, self.err = lift, sqrt, val, err


FLOAT = _Kit(np.float64, np.sqrt, float, lambda x: 0.0)
BOUNDED = _Kit(Bd, _bd_sqrt, lambda x: float(x.v), lambda x: x.e)
EXACT = _Kit(lambda x: Fraction(float(x)), _fsqrt, lambda x: x, lambda x: 0.0)


# ---- the model -----------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("m", "x", "v", "left", "right", "parent", "bodies", "a", "e", "r", "energy")


class Pair:
    __slots__ = ("M", "r", "eps", "dw", "a", "candidate", "d", "w")


class Result:
    """nodes (Node list, node_count of them), top (ids), resolved, min_sep, min_p, min_q, largest, decisions
    [(what, margin, bound, holds)], pairs: the top pairs' (p, q, Pair, criteria)"""

    @property
    def top_count(self):
        return len(self.top)

    @property
    def node_count(self):
        return len(self.nodes)


def _pair(P, Q, G, k):
    d = [Q.x[c] - P.x[c] for c in range(3)]
    w = [Q.v[c] - P.v[c] for c in range(3)]
    o = Pair()
    o.d, o.w = d, w
    o.M = P.m + Q.m
    o.r = k.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    v2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    o.dw = d[0] * w[0] + d[1] * w[1] + d[2] * w[2]
    if k.val(o.r) == 0:  # (the model: -inf or NaN, every comparison false; exact arithmetic cannot divide)
        o.eps, o.a, o.candidate = None, None, False
        return o
    o.eps = k.lift(0.5) * v2 - (G * o.M) / o.r
    o.candidate = bool(k.val(o.M) > 0 and k.val(o.r) > 0 and k.val(o.eps) < 0)
    o.a = (G * o.M) / (k.lift(-2.0) * o.eps) if o.candidate else None
    return o


def _ecc(o, G, k):
    d, w = o.d, o.w
    h = [d[1] * w[2] - d[2] * w[1], d[2] * w[0] - d[0] * w[2], d[0] * w[1] - d[1] * w[0]]
    h2 = h[0] * h[0] + h[1] * h[1] + h[2] * h[2]
    gm = G * o.M
    t = k.lift(1.0) + ((k.lift(2.0) * o.eps) * h2) / (gm * gm)
    return k.sqrt(t if k.val(t) > 0 else (Bd(0.0, max(t.e + float(t.v), 0.0)) if k is BOUNDED else k.lift(0.0)))


def _decompose(X, V, m, G, r_sep, kappa, k):
    n = len(m)
    assert 2 <= n <= MAX_N
    Gk, rs, kp = k.lift(np.float32(G)), k.lift(np.float32(r_sep)), k.lift(np.float32(kappa))
    zero = k.lift(0.0)
    nodes, dec = [], []
    for i in range(n):
        b = Node()
        b.m, b.x, b.v = k.lift(m[i]), [k.lift(c) for c in X[i]], [k.lift(c) for c in V[i]]
        b.left = b.right = b.parent = NONE
        b.bodies, b.a, b.e, b.r, b.energy = 1, zero, zero, zero, zero
        nodes.append(b)
    top, cache = list(range(n)), {}

    def pair(p, q):
        if (p, q) not in cache:
            cache[(p, q)] = _pair(nodes[p], nodes[q], Gk, k)
        return cache[(p, q)]

    for _ in range(n - 1):
        cands = []
        for i, p in enumerate(top):
            for q in top[i + 1:]:
                o = pair(p, q)
                if o.eps is not None and k.val(o.M) > 0:
                    dec.append(("eps < 0", abs(k.val(o.eps)), k.err(o.eps), o.candidate))
                if o.candidate:
                    cands.append((k.val(o.a), p, q))
        if not cands:
            break
        _, p, q = min(cands)
        o = pair(p, q)
        for a2, p2, q2 in cands:
            if (p2, q2) != (p, q) and a2 != k.val(o.a):
                dec.append(("smallest a", a2 - k.val(o.a), k.err(o.a) + k.err(pair(p2, q2).a), True))
        c = Node()
        P, Q = nodes[p], nodes[q]
        c.m = o.M
        c.x = [(P.m * P.x[j] + Q.m * Q.x[j]) / o.M for j in range(3)]
        c.v = [(P.m * P.v[j] + Q.m * Q.v[j]) / o.M for j in range(3)]
        c.left, c.right, c.parent, c.bodies = p, q, NONE, P.bodies + Q.bodies
        c.a, c.r, c.energy, c.e = o.a, o.r, o.eps, _ecc(o, Gk, k)
        P.parent = Q.parent = len(nodes)
        top = [t for t in top if t not in (p, q)] + [len(nodes)]
        nodes.append(c)
    res = Result()
    res.nodes, res.top, res.decisions, res.pairs = nodes, top, dec, []
    res.largest = max(nodes[t].bodies for t in top)
    res.min_sep, res.min_p, res.min_q = None, NONE, NONE
    failed, best = 0, None
    one = k.lift(1.0)
    for i, p in enumerate(top):
        for q in top[i + 1:]:
            o = pair(p, q)
            if o.eps is None:  # (r = 0: no criterion holds, exactly)
                crit, holds = [(-1.0, 0.0)] * 4, [False] * 4
            else:
                lim = kp * (nodes[p].a * (one + nodes[p].e) + nodes[q].a * (one + nodes[q].e))
                # (margin, bound) of r > r_sep, d.w > 0, eps > 0, r > kappa (apo_p + apo_q)
                crit = [(k.val(o.r) - k.val(rs), k.err(o.r)), (k.val(o.dw), k.err(o.dw)), (k.val(o.eps), k.err(o.eps)),
                        (k.val(o.r) - k.val(lim), k.err(o.r) + k.err(lim))]
                holds = [bool(k.val(o.r) > k.val(rs)), bool(k.val(o.dw) > 0), bool(k.val(o.eps) > 0),
                         bool(k.val(o.r) > k.val(lim))]
            failed += not all(holds)
            res.pairs.append((p, q, o, crit, holds))
            key = (k.val(o.r), p, q)
            if key[0] == key[0] and (best is None or key < best):
                best, res.min_sep, res.min_p, res.min_q = key, o.r, p, q
    res.resolved = int(len(top) >= 2 and failed == 0)
    return res


def _state(X, V, m):
    return np.asarray(X, np.float64), np.asarray(V, np.float64), np.asarray(m, np.float64)


def evaluate(X, V, m, G, r_sep, kappa):
    with np.errstate(all="ignore"):
        return _decompose(*_state(X, V, m), G, r_sep, kappa, FLOAT)


def bounded(X, V, m, G, r_sep, kappa):
    with np.errstate(all="ignore"):
        return _decompose(*_state(X, V, m), G, r_sep, kappa, BOUNDED)


def exact(X, V, m, G, r_sep, kappa):
    return _decompose(*_state(X, V, m), G, r_sep, kappa, EXACT)


def _ok(margin, bound):
    return bound == 0.0 or abs(margin) > CLEAR * bound


def clear(b):
    """-> (True, "") or (False, the first decision of the bounded run that is not clear)"""
    for what, margin, bound, _ in b.decisions:
        if not _ok(margin, bound):
            return False, f"{what}: margin {margin:.3g} against bound {bound:.3g}"
    if len(b.top) >= 2:
        if b.resolved:
            for p, q, _, crit, _ in b.pairs:
                for c, (margin, bound) in enumerate(crit):
                    if not _ok(margin, bound):
                        return False, f"criterion {c} of the pair ({p}, {q}): margin {margin:.3g} against bound {bound:.3g}"
        elif not any(not h and _ok(margin, bound) for _, _, _, crit, holds in b.pairs for (margin, bound), h in zip(crit, holds)):
            return False, "unresolved, but no criterion is clearly missed"
    return True, ""


def forest(res):
    """the canonical string (the rule of nbody_amd.hierarchy_string), straight from the nodes"""
    n = sum(1 for b in res.nodes if b.left == NONE)

    def walk(i):
        if i < n:
            return i, str(i)
        a, b = sorted((walk(res.nodes[i].left), walk(res.nodes[i].right)))
        return a[0], f"[{a[1]} {b[1]}]"
    return " ".join(t for _, t in sorted(walk(t) for t in res.top))


VALUES = ("mass", "a", "e", "r", "energy")


def node_values(res, kit):
    """[node][5] floats of mass, a, e, r, energy, and (BOUNDED) their bounds"""
    rows = [[b.m, b.a, b.e, b.r, b.energy] for b in res.nodes]
    return (np.array([[float(kit.val(c)) for c in r] for r in rows], np.float64),
            np.array([[kit.err(c) for c in r] for r in rows], np.float64))


def check_table(tag, rec, table, n, ev, bd, macro=None):
    """a record and a table of the engine against the restatement: the structure exactly, the values within the bound"""
    assert (int(rec["resolved"]), int(rec["top_count"]), int(rec["node_count"]), int(rec["largest"])) == \
        (ev.resolved, ev.top_count, ev.node_count, ev.largest), (tag, rec)
    assert macro is None or int(rec["macro"]) == macro, (tag, rec["macro"], macro)
    assert (rec["reserved"] == 0).all() and table.shape[0] == 2 * n
    vals, _ = node_values(ev, FLOAT)
    _, tol = node_values(bd, BOUNDED)
    worst = 0.0
    for i, b in enumerate(ev.nodes):
        t = table[i]
        assert (int(t["left"]), int(t["right"]), int(t["parent"]), int(t["bodies"])) == (b.left, b.right, b.parent, b.bodies), (tag, i, t)
        assert t["reserved"] == 0.0
        for c, name in enumerate(VALUES):
            diff = abs(float(t[name]) - vals[i, c])
            assert diff <= tol[i, c], (tag, i, name, float(t[name]), vals[i, c], tol[i, c])
            worst = max(worst, diff)
    assert not np.frombuffer(np.ascontiguousarray(table[ev.node_count:]).tobytes(), np.uint8).any(), (tag, "slots above node_count")
    if ev.min_sep is None:
        assert np.isposinf(rec["min_sep"]) and rec["min_p"] == NONE and rec["min_q"] == NONE, (tag, rec)
    else:
        assert (int(rec["min_p"]), int(rec["min_q"])) == (ev.min_p, ev.min_q), (tag, rec)
        assert abs(float(rec["min_sep"]) - float(ev.min_sep)) <= bd.min_sep.e, (tag, rec["min_sep"], ev.min_sep)
        worst = max(worst, abs(float(rec["min_sep"]) - float(ev.min_sep)))
    return worst


def is_none(rec):
    return (rec["resolved"] == 0 and rec["top_count"] == 0 and rec["macro"] == 0 and rec["node_count"] == 0 and rec["largest"] == 0
            and np.isposinf(rec["min_sep"]) and rec["min_p"] == NONE and rec["min_q"] == NONE and (rec["reserved"] == 0).all())


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------
def _ic(rows):
    a = np.asarray(rows, np.float64)
    keys = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")
    return {k: a[:, c].astype(np.float32) for c, k in enumerate(keys)}


def state_of(ic):
    X = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1).astype(np.float64)
    V = np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1).astype(np.float64)
    return X, V, np.asarray(ic["mass"], np.float64)


# a circular binary of two masses 2 at distance 1 (G = 1: w = 2, eps = -2, a = 1, h = 2, e = 0, all exact)
BIN = [[-0.5, 0, 0, 0, -1, 0, 2], [0.5, 0, 0, 0, 1, 0, 2]]


def _graded():
    """16 circular binaries of separations 0.01 1.033^k on a spiral of radius 10 to 25 and a single, on the outward flow
    v = x / 2: 33 bodies, 528 pairs"""
    rows = []
    for k in range(16):
        s, th, R = 0.01 * 1.033 ** k, 2 * math.pi * k / 16, 10.0 + k
        c = np.array([R * math.cos(th), R * math.sin(th), 0.0])
        u = 0.5 * math.sqrt(2.0 / s)  # each member of two masses 1: half the relative circular speed
        for sign in (-1, 1):
            rows.append([c[0] + sign * 0.5 * s, c[1], c[2], 0.5 * c[0], 0.5 * c[1] + sign * u, 0.0, 1.0])
    rows.append([0, 0, 30.0, 0, 0, 15.0, 1.0])
    return rows


def snapshot_cases():
    """{name: dict(ic, r_sep, kappa, forest, K, nodes, resolved)}; G = 1, eps = 0"""
    out = {
        "binary and a receding single": dict(rows=BIN + [[100, 0, 0, 5, 0, 0, 1]], r_sep=10, kappa=5, forest="[0 1] 2", K=2, nodes=4, resolved=1),
        "the single approaching": dict(rows=BIN + [[100, 0, 0, -5, 0, 0, 1]], r_sep=10, kappa=5, forest="[0 1] 2", K=2, nodes=4, resolved=0),
        "the single inside r_sep": dict(rows=BIN + [[100, 0, 0, 5, 0, 0, 1]], r_sep=150, kappa=5, forest="[0 1] 2", K=2, nodes=4, resolved=0),
        "not isolated": dict(rows=BIN + [[100, 0, 0, 5, 0, 0, 1]], r_sep=10, kappa=200, forest="[0 1] 2", K=2, nodes=4, resolved=0),
        "permuted": dict(rows=[BIN[0], [100, 0, 0, 5, 0, 0, 1], BIN[1]], r_sep=10, kappa=5, forest="[0 2] 1", K=2, nodes=4, resolved=1),
        "hierarchical triple": dict(rows=BIN + [[20, 0, 0, 0, 0.3, 0, 1]], r_sep=10, kappa=0, forest="[[0 1] 2]", K=1, nodes=5, resolved=0),
        "mirrored 2+2": dict(rows=[[-10.5, 0, 0, -3, -1, 0, 2], [-9.5, 0, 0, -3, 1, 0, 2], [9.5, 0, 0, 3, -1, 0, 2], [10.5, 0, 0, 3, 1, 0, 2]],
                             r_sep=5, kappa=2, forest="[0 1] [2 3]", K=2, nodes=6, resolved=1),
        "three singles": dict(rows=[[-10, 0, 0, -4, 0, 0, 1], [10, 0, 0, 4, 0, 0, 1], [0, 10, 0, 0, 4, 0, 1]], r_sep=5, kappa=3,
                              forest="0 1 2", K=3, nodes=3, resolved=1),
        "n = 2 bound": dict(rows=BIN, r_sep=10, kappa=0, forest="[0 1]", K=1, nodes=3, resolved=0),
        "n = 2 unbound": dict(rows=[[-1, 0, 0, -3, 0, 0, 1], [1, 0, 0, 3, 0, 0, 1]], r_sep=1, kappa=0, forest="0 1", K=2, nodes=2, resolved=1),
        "massless bound to massive": dict(rows=[[0, 0, 0, 0, 0, 0, 4], [1, 0, 0, 0, 2, 0, 0]], r_sep=1, kappa=0, forest="[0 1]", K=1, nodes=3, resolved=0),
        "two massless": dict(rows=[[0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 0, 0]], r_sep=0.5, kappa=0, forest="0 1", K=2, nodes=2, resolved=1),
        "33 bodies": dict(rows=_graded(), r_sep=1, kappa=2, forest=" ".join(f"[{2 * k} {2 * k + 1}]" for k in range(16)) + " 32", K=17, nodes=49, resolved=1),
        "cold chain of 64": dict(rows=[[3.0 ** i, 0, 0, 0, 0, 0, 1] for i in range(64)], r_sep=1, kappa=0, forest=None, K=1, nodes=127, resolved=0),
    }
    for c in out.values():
        c["ic"] = _ic(c.pop("rows"))
    return out


SMALL = [k for k in snapshot_cases() if k not in ("33 bodies", "cold chain of 64")]  # (the cases of the recorded states)


def two_plus_two_ic():
    """two circular binaries of masses 0.5 and separations 0.5 and 0.4 (so their a differ by a quarter: a mirror-symmetric
    encounter would leave the order of the two composites to the last bits) approaching along x at relative speed 8 with an
    offset of 3 in y: a distant 2+2 fly-by that ends as two receding binaries -- no single body ever leaves, so the escape
    test cannot call it"""
    v, u = 0.5 * math.sqrt(1.0 / 0.5), 0.5 * math.sqrt(1.0 / 0.4)
    return _ic([[-3 + 0.25, 1.5, 0, 4, v, 0, 0.5], [-3 - 0.25, 1.5, 0, 4, -v, 0, 0.5],
                [3 + 0.2, -1.5, 0, -4, u, 0, 0.5], [3 - 0.2, -1.5, 0, -4, -u, 0, 0.5]])


# the walk: the fly-by of the outcomes tests and the 2+2 encounter as one ensemble
WALK = dict(dt=1.0 / 8, macros=10, r_sep=[2.0, 3.5], kappa=2.0)

# the eight fly-bys of the outcomes tests (hermite_batch_outcomes_ref.flyby_ic): their dt_max with these separation radii
FLY_DT = [1.0 / 2, 1.0 / 4, 1.0 / 6, 1.0 / 8, 1.0 / 10, 1.0 / 12, 1.0 / 8, 1.0 / 8]
FLY_RSEP = [1.5, 1.5, 1.5, 1.5, 2.5, 2.5, 0.0, 50.0]
FLY = dict(G=1.0, eps=0.0, L=10, precision="extended", macros=9, kappa=2.0)


def first_resolved(Xs, Vs, m, G, r_sep, kappa, want_clear=True):
    """the boundaries the engine examines, in turn, up to the first resolved one: -> (macro index or 0, [evaluate per
    examined boundary], [bounded ...])"""
    evs, bds = [], []
    for k in range(len(Xs)):
        ev, bd = evaluate(Xs[k], Vs[k], m, G, r_sep, kappa), bounded(Xs[k], Vs[k], m, G, r_sep, kappa)
        if want_clear:
            ok, why = clear(bd)
            assert ok, (k + 1, why)
        evs.append(ev)
        bds.append(bd)
        if ev.resolved:
            return k + 1, evs, bds
    return 0, evs, bds


def recorded(key):
    with np.load(GOLDEN) as z:
        return z[key + "_X"], z[key + "_V"], z[key + "_m"]
