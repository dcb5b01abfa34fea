"""The ensemble OUTCOMES (include/nbody_hip.h "ensemble OUTCOMES") restated: not a test file.

`evaluate` is the model in numpy fp64, operation by operation in the model's order (numpy rounds every elementwise
operation once and fuses nothing, which is what csrc/hermite_batch_outcomes_common.h asks of the compilers).  `exact`
evaluates the same quantities from the same float state in rational arithmetic (fractions.Fraction), with the one square
root taken last (to 2^-200 relative).

The tolerance of r, vr and e against the engine, derived from the model's operation count and NOT fitted on the GPU.
u = 2^-53.  Each of the seven sums passes every term through at most
    K = ceil(n / 512) + 6 + 7
additions (the thread's chain, six lane distances, seven joins of waves), and the term m X itself is rounded once, so to
first order |dS| <= (K + 1) u sum |t_k|.  Write A0 = sum m, A1 = sum |m X_c|, A2 = sum |m V_c| (per component c).  The
per-body chain then propagates absolute errors; every cancelling step (S1 - m X, X - R, 1/2 w^2 - G S0 / r) enters through
the absolute error of its operands, which is the same as multiplying the relative error by that step's condition number
(|a| + |b|) / |a - b| -- `Bounds.kappa` reports the three condition numbers of the worst body:
    M  = S0 - m          dM  = (K + 1) u A0 + u |M|
    N  = S1 - m X        dN  = (K + 1) u A1 + u |m X| + u |N|          (one rounding of m X, one of the difference)
    R  = N / M           dR  = dN / M + |R| dM / M + u |R|
    d  = X - R           dd  = dR + u |d|                              (the same for U and w from S2 and V)
    r2 = dx dx + ..      dr2 = sum 2 |d_c| dd_c + 3 u r2               (three products, two additions: each <= u r2)
    r  = sqrt(r2)        dr  = dr2 / (2 r) + u r
    dw = dx wx + ..      ddw = sum (|d_c| dw_c + |w_c| dd_c) + 3 u sum |d_c w_c|
    vr = dw / r          dvr = ddw / r + |vr| dr / r + u |vr|
    h  = 0.5 (w . w)     dh  = sum |w_c| dw_c + 1.5 u w2
    p  = (G S0) / r      dp  = p ((K + 1) u A0 / S0 + dr / r + 2 u)    (G S0 rounded, the quotient rounded)
    e  = h - p           de  = dh + dp + u |e|
Those are the terms of first order.  What they leave out are products of two errors.  Take every error relative to the
quantity it multiplies or divides further down -- dM / M, dd_c / r, dw_c / |w|, dr / r, (K + 1) u for the sums -- and call
the largest `Bounds.rel` (per body; about 1e-15 here).  A product of two errors is then at most rel times a term of first
order, or, where that term vanishes with a component (dd_c^2 in r2 when d_c = 0), rel^2 r2 against the 3 u r2 that is
always there.  The tests assert rel < REL_MAX = 1e-12 for every body whose values they compare, so rel^2 < 2^-20 u and the
terms of second order are below 2^-20 of the bound: each bound is multiplied by SECOND = 1 + 2^-20 for them, and by
nothing else.
The engine evaluates the same chain on the same state -- the same correctly rounded, unfused fp64 operations in the same
order -- so the GPU tests hold |engine - restatement| to this bound itself for r, vr and e, and to dM for rest_mass;
nothing in it is fitted on the GPU.  tests/test_hermite_batch_outcomes_cpu.py holds the restatement to the same bound against exact arithmetic for every
case below, at its initial state and at the states the engine recorded (tests/golden/hermite_batch_outcomes_states.npz).

Decisions.  A body is CLEAR at a boundary when its verdict cannot depend on those errors: an escaping body has all three
margins |r - r_esc|, |d.w|, |e| above 1e6 times their bounds (dr, ddw, de); a body that does not escape has at least one
criterion that fails by more than 1e6 times its bound.  A body whose rest has no mass is clear when M is exactly 0."""
import math
import os
from fractions import Fraction

import numpy as np

# the states the engine reached: X and V (hi + lo as fp64) after every macro step of every case below and of the eight
# fly-bys, recorded on an MI355X by tests/golden/make_hermite_batch_outcomes_states.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hermite_batch_outcomes_states.npz")
U53 = 2.0 ** -53
CLEAR = 1.0e6
SECOND = 1.0 + 2.0 ** -20  # the terms of second order (module docstring)
REL_MAX = 1.0e-12
THREADS, WAVE = 512, 64
NONE = 0xFFFFFFFF


def sum_ops(n):
    """K: the additions on the longest path of a sum over n bodies"""
    return -(-n // THREADS) + 6 + 7


def model_sum(t):
    """sum of the terms t [n, ...] in the model's order: thread, lane distances 32 .. 1, waves in rising order"""
    t = np.asarray(t, np.float64)
    n = t.shape[0]
    acc = np.zeros((THREADS,) + t.shape[1:])
    for k in range(-(-n // THREADS)):
        part = t[k * THREADS:(k + 1) * THREADS]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    a = acc.reshape((THREADS // WAVE, WAVE) + t.shape[1:]).copy()
    off = WAVE // 2
    while off:
        a[:, :off] = a[:, :off] + a[:, off:2 * off]
        off //= 2
    total = a[0, 0].copy()
    for w in range(1, THREADS // WAVE):
        total = total + a[w, 0]
    return total


class Bodies:
    """what the model gives for every body of one system at one boundary"""

    def __init__(self, r, vr, e, rest, dw, escapes):
        self.r, self.vr, self.e, self.rest, self.dw, self.escapes = r, vr, e, rest, dw, escapes

    @property
    def count(self):
        return int(self.escapes.sum())

    @property
    def lowest(self):
        idx = np.flatnonzero(self.escapes)
        return int(idx[0]) if idx.size else NONE


def evaluate(X, V, m, G, r_esc):
    """the model in fp64, in its order.  X, V [n, 3] fp64 (hi + lo), m [n] (float32 values), G and r_esc float32 values"""
    X, V, m = np.asarray(X, np.float64), np.asarray(V, np.float64), np.asarray(m, np.float64)
    n = m.size
    G, r_esc = float(np.float32(G)), float(np.float32(r_esc))
    zero = np.zeros(n)
    if n < 2 or not r_esc > 0.0:
        return Bodies(zero, zero, zero, zero, zero, np.zeros(n, bool))
    S0 = model_sum(m)
    S1 = model_sum(m[:, None] * X)
    S2 = model_sum(m[:, None] * V)
    M = S0 - m
    ok = M > 0.0
    with np.errstate(all="ignore"):
        Ms = np.where(ok, M, 1.0)[:, None]
        R = (S1[None, :] - m[:, None] * X) / Ms
        Uc = (S2[None, :] - m[:, None] * V) / Ms
        d, w = X - R, V - Uc
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        dw = d[:, 0] * w[:, 0] + d[:, 1] * w[:, 1] + d[:, 2] * w[:, 2]
        vr = dw / r
        e = 0.5 * (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]) - (G * S0) / r
        esc = ok & (r > r_esc) & (dw > 0.0) & (e > 0.0)
    f = lambda a: np.where(ok, a, 0.0)  # noqa: E731
    return Bodies(f(r), f(vr), f(e), f(M), f(dw), esc)


class Bounds:
    def __init__(self, dr, dvr, de, ddw, dM, kappa, rel):
        self.dr, self.dvr, self.de, self.ddw, self.dM, self.kappa, self.rel = dr, dvr, de, ddw, dM, kappa, rel


def _kappa(operands, result):
    """the condition number (|a| + |b|) / |a - b| of a difference; 1 where both operands are 0, inf where it cancels to 0"""
    with np.errstate(all="ignore"):
        return np.where(result > 0, operands / np.where(result > 0, result, 1.0), np.where(operands > 0, np.inf, 1.0))


def bounds(X, V, m, G):
    """the per-body error bounds of the module docstring, evaluated with the restatement's own values"""
    X, V, m = np.asarray(X, np.float64), np.asarray(V, np.float64), np.asarray(m, np.float64)
    n, u, G = m.size, U53, float(np.float32(G))
    K1 = sum_ops(n) + 1
    S0, A0 = m.sum(), np.abs(m).sum()
    S1, S2 = (m[:, None] * X).sum(0), (m[:, None] * V).sum(0)
    A1, A2 = np.abs(m[:, None] * X).sum(0), np.abs(m[:, None] * V).sum(0)
    M = S0 - m
    ok = M > 0.0
    Ms = np.where(ok, M, 1.0)
    dM = K1 * u * A0 + u * np.abs(M)

    def chain(S, A, Y):
        N = S[None, :] - m[:, None] * Y
        dN = K1 * u * A[None, :] + u * np.abs(m[:, None] * Y) + u * np.abs(N)
        Rc = N / Ms[:, None]
        dR = dN / Ms[:, None] + np.abs(Rc) * (dM / Ms)[:, None] + u * np.abs(Rc)
        dd = Y - Rc
        kap = np.maximum(_kappa(np.abs(S)[None, :] + np.abs(m[:, None] * Y), np.abs(N)), _kappa(np.abs(Y) + np.abs(Rc), np.abs(dd)))
        return dd, dR + u * np.abs(dd), kap

    d, dd, kd = chain(S1, A1, X)
    w, dwv, kw = chain(S2, A2, V)
    r2 = (d * d).sum(1)
    r = np.sqrt(r2)
    rs = np.maximum(r, 1e-300)
    dr2 = (2 * np.abs(d) * dd).sum(1) + 3 * u * r2
    dr = dr2 / (2 * rs) + u * r
    dwd = (d * w).sum(1)
    ddw = (np.abs(d) * dwv + np.abs(w) * dd).sum(1) + 3 * u * np.abs(d * w).sum(1)
    vr = dwd / rs
    dvr = ddw / rs + np.abs(vr) * dr / rs + u * np.abs(vr)
    w2 = (w * w).sum(1)
    dh = (np.abs(w) * dwv).sum(1) + 1.5 * u * w2
    p = G * S0 / rs
    dp = np.abs(p) * (K1 * u * A0 / max(abs(S0), 1e-300) + dr / rs + 2 * u)
    e = 0.5 * w2 - p
    de = dh + dp + u * np.abs(e)
    ke = _kappa(0.5 * w2 + np.abs(p), np.abs(e))
    z = lambda a: np.where(ok, SECOND * a, 0.0)  # noqa: E731
    worst = int(np.argmax(np.where(ok, de, -1.0))) if ok.any() else 0
    kappa = (float(kd[worst].max()), float(kw[worst].max()), float(ke[worst]))
    ws = np.maximum(np.sqrt(w2), 1e-300)
    rel = np.maximum.reduce([dM / Ms, dd.max(1) / rs, dwv.max(1) / ws, dr / rs, np.full(n, K1 * u)])  # (module docstring)
    return Bounds(z(dr), z(dvr), z(de), z(ddw), z(dM), kappa, rel)


def _fsqrt(q, bits=200):
    """sqrt of a non-negative Fraction to 2^-bits relative, as a Fraction"""
    if q == 0:
        return Fraction(0)
    shift = max(0, 2 * bits - (q.numerator.bit_length() - q.denominator.bit_length()) + 2)
    shift += shift & 1
    return Fraction(math.isqrt((q.numerator << shift) // q.denominator), 1 << (shift // 2))


def exact(X, V, m, G, bodies=None):
    """{i: (r, vr, e, rest, dw)} as floats rounded from exact rational arithmetic on the float state (bodies: which; all)"""
    n = len(m)
    Xf = [[Fraction(float(c)) for c in row] for row in np.asarray(X, np.float64)]
    Vf = [[Fraction(float(c)) for c in row] for row in np.asarray(V, np.float64)]
    mf = [Fraction(float(c)) for c in np.asarray(m, np.float64)]
    Gf = Fraction(float(np.float32(G)))
    S0 = sum(mf)
    S1 = [sum(mf[i] * Xf[i][c] for i in range(n)) for c in range(3)]
    S2 = [sum(mf[i] * Vf[i][c] for i in range(n)) for c in range(3)]
    out = {}
    for i in (range(n) if bodies is None else bodies):
        M = S0 - mf[i]
        if M <= 0:
            out[i] = (0.0, 0.0, 0.0, 0.0, 0.0)
            continue
        d = [Xf[i][c] - (S1[c] - mf[i] * Xf[i][c]) / M for c in range(3)]
        w = [Vf[i][c] - (S2[c] - mf[i] * Vf[i][c]) / M for c in range(3)]
        r = _fsqrt(sum(c * c for c in d))
        dw = sum(a * b for a, b in zip(d, w))
        if r == 0:
            out[i] = (0.0, float("nan"), float("nan"), float(M), float(dw))
            continue
        out[i] = (float(r), float(dw / r), float(sum(c * c for c in w) / 2 - Gf * S0 / r), float(M), float(dw))
    return out


def clear(b, bd, r_esc):
    """per body: the verdict cannot depend on the rounding errors (module docstring)"""
    r_esc = float(np.float32(r_esc))
    mr, mw, me = np.abs(b.r - r_esc) > CLEAR * bd.dr, np.abs(b.dw) > CLEAR * bd.ddw, np.abs(b.e) > CLEAR * bd.de
    fails_clearly = ((b.r <= r_esc) & mr) | ((b.dw <= 0.0) & mw) | ((b.e <= 0.0) & me)
    massless_rest = b.rest == 0.0  # (M = S0 - m is 0 exactly only when the rest has no mass: never an escape)
    return np.where(b.escapes, mr & mw & me, fails_clearly | massless_rest)


# ---- the cases of the tests: {name: dict(ic=..., G, eps, dt, L, r_esc, macros, precision, expect=(count, lowest) or None)} ----
def _ic(rows):
    a = np.asarray(rows, np.float64)
    keys = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")
    return {k: a[:, c].astype(np.float32) for c, k in enumerate(keys)}


def flyby_ic():
    """an equal-mass circular binary of separation 0.5 around the origin and a light intruder that starts beyond every
    escape radius used with it, APPROACHING at speed 8 with impact parameter 1, and leaves on the far side"""
    v = 0.5 * math.sqrt(1.0 / 0.5)  # each member: half the relative circular speed sqrt(G M / a)
    return _ic([[0.25, 0, 0, 0, v, 0, 0.5], [-0.25, 0, 0, 0, -v, 0, 0.5], [-3, 1, 0, 8, 0, 0, 0.0625]])


# eight copies of the fly-by: the intruder starts at x = -3 with speed 8 and impact parameter 1; with dt_max[s] it stands
# near x = -3 + 8 k dt_max[s] after k macro steps and escapes at the first boundary beyond r_esc on the far side
FLY_DT = [1.0 / 2, 1.0 / 4, 1.0 / 6, 1.0 / 8, 1.0 / 10, 1.0 / 12, 1.0 / 8, 1.0 / 8]
FLY_RESC = [1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 0.0, 50.0]
FLY_MACRO = [1, 2, 3, 4, 5, 6, 0, 0]  # the macro index of the first escape, 0: never
FLY = dict(G=1.0, eps=0.0, L=10, precision="extended", macros=7)


def kicked_plummer(nb, n, index, seed):
    """a Plummer sphere (all inside r = 10.6) with body `index` put at (12, 0, 0) and sent outward at speed 4"""
    ic = {k: np.array(v, np.float32) for k, v in nb.ic.plummer(n, seed=seed).items()}
    for k, val in (("pos_x", 12.0), ("pos_y", 0.0), ("pos_z", 0.0), ("vel_x", 4.0), ("vel_y", 0.0), ("vel_z", 0.0)):
        ic[k][index] = val
    return ic


def cases(nb):
    e9 = math.sqrt(0.1 / 1.9)  # speed at the apocentre 1.9 of a = 1, e = 0.9, G M = 1
    out = {
        # both members leave: count 2, the lower index 0
        "unbound pair": dict(ic=_ic([[0.5, 0, 0, 1, 0.25, 0, 0.5], [-0.5, 0, 0, -1, -0.25, 0, 0.5]]), r_esc=1.5, macros=8,
                             precision="extended", expect=(2, 0)),
        # a = 1, e = 0.9 from the apocentre 1.9 > r_esc: beyond the radius, but bound and falling back: never
        "bound e = 0.9 pair": dict(ic=_ic([[0.95, 0, 0, 0, 0.5 * e9, 0, 0.5], [-0.95, 0, 0, 0, -0.5 * e9, 0, 0.5]]), r_esc=1.5,
                                   macros=5, precision="fp32", expect=None),
        "fly-by": dict(ic=flyby_ic(), r_esc=2.0, macros=8, dt=1.0 / 8, precision="extended", expect=(1, 2)),
        # the second body of thread 3, in the first wave; the third body of thread 0
        "plummer 600, body 515": dict(ic=kicked_plummer(nb, 600, 515, 31), r_esc=12.5, macros=4, precision="fp32",
                                      eps=0.05, expect=(1, 515)),
        "plummer 1025, body 1024": dict(ic=kicked_plummer(nb, 1025, 1024, 32), r_esc=12.5, macros=4, precision="extended",
                                        eps=0.05, expect=(1, 1024)),
        # a massless body leaves a binary
        "massless escaper": dict(ic=_ic([[0.25, 0, 0, 0, 0.5 * math.sqrt(2.0), 0, 0.5], [-0.25, 0, 0, 0, -0.5 * math.sqrt(2.0), 0, 0.5],
                                         [0, 1, 0, 0.5, 3, 0, 0.0]]), r_esc=1.5, macros=5, precision="fp32", expect=(1, 2)),
        # the whole mass in body 0 (M_r = 0: never), the massless body 1 leaves
        "whole mass in one body": dict(ic=_ic([[0, 0, 0, 0, 0, 0, 1.0], [1, 0, 0, 3, 0.5, 0, 0.0]]), r_esc=1.5, macros=5,
                                       precision="fp32", expect=(1, 1)),
        "n = 1": dict(ic=_ic([[5, 0, 0, 3, 0, 0, 1.0]]), r_esc=1.0, macros=2, precision="fp32", expect=None),
    }
    for c in out.values():
        c.setdefault("G", 1.0)
        c.setdefault("eps", 0.0)
        c.setdefault("dt", 1.0 / 16)
        c.setdefault("L", 10)
    return out


def recorded(key):
    """(X [macros, n, 3], V, m) of GOLDEN: key = the case's place in cases(), or "fly" for the eight fly-bys"""
    pre = "fly" if key == "fly" else f"c{key}"
    with np.load(GOLDEN) as z:
        return z[pre + "_X"], z[pre + "_V"], z[pre + "_m"]


def state_of(ic):
    """(X, V, m) of an initial-condition dict: the float32 values widened"""
    X = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1).astype(np.float64)
    V = np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1).astype(np.float64)
    return X, V, np.asarray(ic["mass"], np.float64)
