"""The ensemble mergers (include/nbody_hip.h, "ensemble MERGERS") restated in numpy for the tests
(tests/test_hermite_batch_mergers_*.py): the slots, the merged body and what is stored of it, the radius rule, the
compaction with the ids, the energy deltas with the sum over the others in the model's order, and the same in exact
rational arithmetic.  numpy only.

Every operation below is one IEEE operation on np.float64 / np.float32 scalars, in the order the model writes them, so
the restatement equals csrc/hermite_batch_mergers_common.h bit for bit where that file forbids contraction (the merged
body, the stored values, delta_ke); np.cbrt and the pair terms (the diagnostics' diag_pair, which the device may contract)
are compared within a stated bound.  The restatement's own error against exact arithmetic:
  merged X, V before the rounding to what is stored: two products, a sum and a quotient -> 3 u64 (|ma Xa| + |mb Xb|) / M
      with u64 = 2^-53, far below the 2^-24 |X| (fp32) or 2^-46 |X| (hi + lo) of the stored value;
  delta_ke: 3 terms of 6 operations each -> 8 u64 (KE + KEa + KEb);
  delta_pe: 3 (n - 2) + 1 terms t of at most 8 operations each, summed in a tree of depth <= ceil(n / 256) + 6 + 3 ->
      (8 + ceil(n / 256) + 10) u64 G sum |t|."""
import math
from fractions import Fraction

import numpy as np

import hermite_batch_events_cases as ec

NONE = 0xFFFFFFFF
U64 = 2.0 ** -53
f64, f32 = np.float64, np.float32


# the arithmetic cases of the GPU test (and of the CPU test, at their initial states): name, n, the pair's slots.  n = 2 -> 1;
# n = 3 at every pair (move / no move of the last slot); n = 5 at an offset; n = 257 and 1,025 with the last body at slot 256
# resp. 1,024, so that the move crosses the 256-source tile and the 1,024-source block
CASES = [("pair", 2, (0, 1)), ("triple01", 3, (0, 1)), ("triple02", 3, (0, 2)), ("triple12", 3, (1, 2)), ("five", 5, (1, 3)),
         ("tile", 257, (3, 255)), ("block", 1025, (3, 255))]
CASE_SEP = 0.01  # the pair's separation; both get the radius CASE_SEP, everyone else none: the only contact


def case_ic(nb, n, pair):
    """a Plummer sphere of n bodies with the pair brought to CASE_SEP of each other, at rest relative to each other.  The
    pair is made light (1e-3 and 2e-3): unsoftened (eps = 0: the GUARD forms), two bodies of mass 1/2 at rest 0.01 apart
    would be thrown through each other and out of contact by the first predictor step, before any pair is looked at;
    G m / d^2 <= 34 moves these by less than 0.5 * 34 / 64^2 = 0.004 each in the longest step (dt_max = 1/64), so the
    first block step sees them closer than the sum of their radii, 0.02"""
    ic = {k: v[:n].copy() for k, v in dict(nb.ic.plummer(max(n, 2), seed=300 + n)).items()}
    ic = ec.with_close_pair(ic, pair[0], pair[1], CASE_SEP)
    ic["mass"][pair[0]], ic["mass"][pair[1]] = np.float32(1e-3), np.float32(2e-3)
    return ic


def case_radii(n, pair):
    r = np.zeros(n, np.float32)
    r[list(pair)] = CASE_SEP
    return r


def slots(ci, cj, n):
    """-> None (the record is refused) or (lo, hi, moved_from, dead)"""
    ci, cj, n = int(ci), int(cj), int(n)
    if ci == cj or ci >= n or cj >= n:
        return None
    lo, hi, dead = min(ci, cj), max(ci, cj), n - 1
    return lo, hi, (NONE if hi == dead else dead), dead


def concerned(stopped, status):
    return int(stopped) == 1 and int(status) == 0


def radius(ra, rb):
    a, b = f64(f32(ra)), f64(f32(rb))
    return f32(np.cbrt(a * a * a + b * b * b))


def split(v, ext):
    hi = f32(v)
    return hi, (f32(f64(v) - f64(hi)) if ext else f32(0.0))


class System:
    """one system's state as the engine holds it: pos, vel [n, 3] fp32 with their residuals (zeros in fp32 mode), mass,
    radii fp32, ids uint32; n is the live count, the arrays keep the slots of the layout"""

    def __init__(self, pos, vel, mass, radii, pos_lo=None, vel_lo=None, ids=None, ext=False):
        self.pos, self.vel = np.array(pos, f32), np.array(vel, f32)
        self.pos_lo = np.zeros_like(self.pos) if pos_lo is None else np.array(pos_lo, f32)
        self.vel_lo = np.zeros_like(self.vel) if vel_lo is None else np.array(vel_lo, f32)
        self.mass, self.radii = np.array(mass, f32), np.array(radii, f32)
        self.ids = np.arange(len(self.mass), dtype=np.uint32) if ids is None else np.array(ids, np.uint32)
        self.n, self.ext, self.log = len(self.mass), bool(ext), []

    @classmethod
    def from_f64(cls, X, V, mass, radii, ext):
        X, V = np.asarray(X, f64), np.asarray(V, f64)
        p, v = X.astype(f32), V.astype(f32)
        return cls(p, v, mass, radii, (X - p).astype(f32), (V - v).astype(f32), ext=ext)

    def X(self):
        return self.pos.astype(f64) + self.pos_lo.astype(f64)

    def V(self):
        return self.vel.astype(f64) + self.vel_lo.astype(f64)


def pair_term(ma, Xa, mb, Xb, eps2):
    """the diagnostics' t(a, b) = ma mb / sqrt(|Xb - Xa|^2 + eps2), 0 when the radicand is 0"""
    d = Xb - Xa
    h = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + eps2
    return f64(0.0) if h == 0.0 else ma * mb / np.sqrt(h)


def kinetic(m, V):
    return f64(0.5) * (m * (V[0] * V[0] + V[1] * V[1] + V[2] * V[2]))


def model_sum(terms, keep, lanes=256, wave=64):
    """the sum of terms[k] over the k with keep[k] in the model's order: lane t adds k = t, t + lanes, ...; inside each
    wave lane l takes lane l + off for off = wave / 2 .. 1; the waves' sums in rising order"""
    acc = [f64(0.0)] * lanes
    for k in range(len(terms)):
        if keep[k]:
            acc[k % lanes] = acc[k % lanes] + terms[k]
    for w0 in range(0, lanes, wave):
        off = wave // 2
        while off:
            for lane in range(off):
                acc[w0 + lane] = acc[w0 + lane] + acc[w0 + lane + off]
            off //= 2
    total = acc[0]
    for w0 in range(wave, lanes, wave):
        total = total + acc[w0]
    return total


def merge(sys, ci, cj, G, eps, contact=(np.inf, 0, 0), stored=None):
    """One pass on one system, in place: -> the log entry (a dict), or None when the record is refused.  eps: the fp32
    softening (eps2 is its fp32 square, as the handle's); contact: (d2, tick, macro) of the event record.  stored:
    (mass, pos hi, pos lo, vel hi, vel lo) of the merged body as an engine stored them -- the deltas are defined on the
    stored values, so a test that has checked those against this restatement's (entry["own"]) passes them in."""
    s = slots(ci, cj, sys.n)
    if s is None:
        return None
    lo, hi, moved, dead = s
    X, V, m = sys.X(), sys.V(), sys.mass.astype(f64)
    eps2 = f64(f32(eps) * f32(eps))
    ma, mb = m[lo], m[hi]
    M = ma + mb
    if M == 0.0:
        Xm, Vm = f64(0.5) * (X[lo] + X[hi]), f64(0.5) * (V[lo] + V[hi])
    else:
        Xm, Vm = (ma * X[lo] + mb * X[hi]) / M, (ma * V[lo] + mb * V[hi]) / M
    m32 = f32(M)
    ph, pl = zip(*(split(c, sys.ext) for c in Xm))
    vh, vl = zip(*(split(c, sys.ext) for c in Vm))
    own_stored = (m32, np.array(ph, f32), np.array(pl, f32), np.array(vh, f32), np.array(vl, f32))
    if stored is not None:
        m32, ph, pl, vh, vl = (f32(stored[0]),) + tuple(tuple(np.asarray(a, f32)) for a in stored[1:])
    Xs = np.array(ph, f64) + np.array(pl, f64)   # the merged body as stored
    Vs = np.array(vh, f64) + np.array(vl, f64)
    Ms = f64(m32)
    dke = (kinetic(Ms, Vs) - kinetic(ma, V[lo])) - kinetic(mb, V[hi])
    live = range(sys.n)
    terms = [f64(0.0) if k in (lo, hi) else
             (pair_term(Ms, Xs, m[k], X[k], eps2) - pair_term(ma, X[lo], m[k], X[k], eps2)) - pair_term(mb, X[hi], m[k], X[k], eps2)
             for k in live]
    others = model_sum(terms, [k not in (lo, hi) for k in live])
    own = pair_term(ma, X[lo], mb, X[hi], eps2)
    dpe = -f64(G) * (others - own)
    mags = sum(abs(pair_term(Ms, Xs, m[k], X[k], eps2)) + abs(pair_term(ma, X[lo], m[k], X[k], eps2)) +
               abs(pair_term(mb, X[hi], m[k], X[k], eps2)) for k in live if k not in (lo, hi)) + abs(own)
    r = radius(sys.radii[lo], sys.radii[hi])
    entry = dict(slot_a=lo, slot_b=hi, id_a=int(sys.ids[lo]), id_b=int(sys.ids[hi]), moved_from=moved,
                 contact_d2=f32(contact[0]), contact_tick=int(contact[1]), contact_macro=int(contact[2]), mass=M,
                 radius=r, delta_ke=dke, delta_pe=dpe, others=others, pe_terms=float(mags),
                 ke_terms=float(kinetic(Ms, Vs) + kinetic(ma, V[lo]) + kinetic(mb, V[hi])), n=sys.n, own=own_stored,
                 momentum_terms=np.abs(ma * V[lo]) + np.abs(mb * V[hi]))
    # the stores
    sys.pos[lo], sys.pos_lo[lo], sys.vel[lo], sys.vel_lo[lo] = ph, pl, vh, vl
    sys.mass[lo], sys.radii[lo] = m32, r
    if moved != NONE:
        for a in (sys.pos, sys.pos_lo, sys.vel, sys.vel_lo, sys.mass, sys.radii, sys.ids):
            a[hi] = a[dead]
    sys.vel[dead] = sys.vel_lo[dead] = sys.pos_lo[dead] = 0.0
    sys.mass[dead] = sys.radii[dead] = 0.0
    sys.ids[dead] = NONE
    sys.n -= 1
    sys.log.append(entry)
    return entry


def pe_bound(entry, G):
    """the fp64 rounding of delta_pe as a formula in n and the sum of |terms| (module docstring); it covers the engine's
    evaluation too, whose pair terms may contract |d|^2 into fused operations (never more roundings than counted)"""
    return (8 + math.ceil(entry["n"] / 256) + 10) * U64 * abs(G) * entry["pe_terms"]


def ke_bound(entry):
    return 8 * U64 * entry["ke_terms"]


def exact(X, V, m, lo, hi):
    """M and the merged X, V before any rounding, in rational arithmetic"""
    Fx = lambda a: [Fraction(float(c)) for c in a]  # noqa: E731
    ma, mb = Fraction(float(m[lo])), Fraction(float(m[hi]))
    M = ma + mb
    if M == 0:
        Xm = [(a + b) / 2 for a, b in zip(Fx(X[lo]), Fx(X[hi]))]
        Vm = [(a + b) / 2 for a, b in zip(Fx(V[lo]), Fx(V[hi]))]
    else:
        Xm = [(ma * a + mb * b) / M for a, b in zip(Fx(X[lo]), Fx(X[hi]))]
        Vm = [(ma * a + mb * b) / M for a, b in zip(Fx(V[lo]), Fx(V[hi]))]
    return M, Xm, Vm


def exact_deltas(Ms, Xs, Vs, X, V, m, n, lo, hi, G, eps2):
    """delta_ke exactly and delta_pe with exact radicands (the stored merged body Ms, Xs, Vs given in fp64)"""
    F = lambda c: Fraction(float(c))  # noqa: E731
    ke = lambda mm, v: F(mm) * sum(F(c) * F(c) for c in v) / 2  # noqa: E731

    def t(m1, x1, m2, x2):
        h = sum((F(b) - F(a)) ** 2 for a, b in zip(x1, x2)) + F(eps2)
        return Fraction(0) if h == 0 else F(m1) * F(m2) / Fraction(math.sqrt(h))  # (sqrt of the rounded radicand: 2 u64)

    dke = ke(Ms, Vs) - ke(m[lo], V[lo]) - ke(m[hi], V[hi])
    s = sum((t(Ms, Xs, m[k], X[k]) - t(m[lo], X[lo], m[k], X[k]) - t(m[hi], X[hi], m[k], X[k])
             for k in range(n) if k not in (lo, hi)), Fraction(0))
    return dke, -F(G) * (s - t(m[lo], X[lo], m[hi], X[hi]))


def parse_check_output(text):
    """the "case" / "body" / "out" lines of csrc/hermite_batch_mergers_check.cpp -> a list of dicts"""
    cases, cur = [], None
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            cur = dict(name=w[1], n=int(w[3]), ext=int(w[5]), i=int(w[7]), j=int(w[9]), G=float.fromhex(w[11]),
                       eps=float.fromhex(w[13]), bodies=[], out=None)
            cases.append(cur)
        elif w[0] == "body":
            cur["bodies"].append([float.fromhex(v) for v in w[3::2]])
        elif w[0] == "out":
            cur["out"] = dict(lo=int(w[2]), hi=int(w[4]), moved=int(w[6]), dead=int(w[8]),
                              values=[float.fromhex(v) for v in w[10::2]])
    return cases
