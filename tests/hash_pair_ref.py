"""The cutoff decision of the spatial hash, pair by pair, restated without a grid -- and the lattice populations that put
pairs exactly ON the decision's edge (tests/test_hash_pairs_cpu.py checks this file, tests/test_hash_pairs_gpu.py holds
the kernels to it).

Lattice bodies: every coordinate is an integer (|.| < 2^24) times a unit that is a power of two, so positions and their
differences are exact in float32 and everything the decision depends on is integer arithmetic here:
  dist2_fp32(i, j, k)  hash_dist2 of csrc/spatial_hash.hip on integers: fl(i i), fl(j j + that), fl(k k + that), each
                       rounded to 24 significant bits, nearest even (one product, two fused multiply-adds);
  the decision         d2 < cutoff2 with cutoff2 = fl(cutoff cutoff), as HashParams::set forms it;
  reference()          the fp64 sum of m_j d h^-3/2 over exactly the pairs that pass, h = the float32 value of d2 + eps2
                       (the "gold" kind of tests/gpu_util.py), with kappa = sum |t| / |a| and the decided pairs.  A
                       coincident pair (d = 0) passes the decision and contributes exactly 0.  No grid takes part.

Populations (fixed seeds, at most 2,500 bodies, explicit bounds for nbody_hip_grid_build_packed):
  ties(...)     a 16^3 lattice of unit spacing, half occupied, a tenth of the bodies duplicated; cutoff 5 (30 lattice
                vectors at exactly 25, 24 at 24, 72 at 26) or 4 (cutoff2 = 16, a power of two: 6 vectors at 16, 48 at 17,
                none at 15, 48 at 14); cell 6 with the bounds on lattice planes (bodies exactly on cell faces) or 5.05 with
                the bounds off the lattice.  About 80 bodies per occupied cell, windows of up to all ~2,250 bodies:
                several LDS batches.  (The issue asked for about 12^3 sites; 16^3 is what gives windows of thousands of entries.)
                sparse: ~3 % occupancy for the light-cell forms -- groups of four: a random site, a site at the largest
                lattice distance below the cutoff from it, and for each of the two a site at exactly the cutoff, so
                that every body has a tie.
  one_ulp(c)    "stars" on a fine lattice (unit 2^-11, half of q = 2^-10: the half-unit coordinates reach float32 values
                that no sum of three integer squares does): a centre in the middle of a cell, ONE boundary satellite
                whose d2 is the float 2, 1 or 0 ulps below / above cutoff2, and fillers beyond the cutoff that put the
                satellite at a chosen place of the centre's window.  Stars are four cells apart.
  Population.scaled(k)   everything times 2^k (masses 4^k): the accelerations keep their magnitude.
"""
import itertools
import math
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "n-body_amd", "csrc", "spatial_hash.hip")
EPS_FRACTION = 0.05          # eps = 0.05 cutoff for the ordinary instantiations, 0 for GUARD
ONE_ULP_UNIT = 2.0 ** -11    # half of q = 2^-10


def limits():
    """(lowest cutoff2, highest cutoff2 of the compare-free decision; eps2 below which GUARD runs), float32, read from
    cut_const_ok and HashParams::guard of csrc/spatial_hash.hip"""
    with open(SOURCE) as f:
        s = f.read()
    m = re.search(r"cut_const_ok\(float cutoff2\) \{ return cutoff2 >= ([0-9.e+-]+)f && cutoff2 <= ([0-9.e+-]+)f; \}", s)
    g = re.search(r"bool guard\(bool compare_free = true\) const \{ return eps2 < ([0-9.e+-]+)f \|\|", s)
    assert m and g, "cut_const_ok / HashParams::guard of csrc/spatial_hash.hip no longer read as this file expects"
    return F(m.group(1)), F(m.group(2)), F(g.group(1))


# ---- float32 arithmetic on integers ---------------------------------------------------------------------------------------
def round24(v):
    """non-negative integers (below 2^53) rounded to 24 significant bits, ties to even: float32's rounding"""
    v = np.asarray(v, np.int64)
    _, ex = np.frexp(v.astype(np.float64))            # v = m 2^ex, 0.5 <= m < 1: ex = bit length
    sh = np.maximum(ex.astype(np.int64) - 24, 0)
    r = v >> sh
    rem = v - (r << sh)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), np.int64(0))
    up = (sh > 0) & ((rem > half) | ((rem == half) & ((r & 1) == 1)))
    return (r + up) << sh


def dist2_fp32(i, j, k):
    """hash_dist2(dx, dy, dz) = fma(dz, dz, fma(dy, dy, dx * dx)) for dx, dy, dz = i, j, k units: the integer d2 / unit^2"""
    i, j, k = (np.asarray(v, np.int64) for v in (i, j, k))
    return round24(k * k + round24(j * j + round24(i * i)))


def neighbour(v, ulps):
    """the float32 value `ulps` floats above (below: negative) the float32 value v"""
    v = F(v)
    for _ in range(abs(int(ulps))):
        v = np.nextafter(v, F(np.inf) if ulps > 0 else F(-np.inf))
    return v


# ---- populations -----------------------------------------------------------------------------------------------------------
class Population:
    """ints [n, 3] lattice coordinates, mass [n] float32, unit (a power of two), cutoff = cutoff_units unit, the grid's cell
    size and bounds (float32 values), planted = [(centre, satellite, intended ulps)] of the one-ulp populations"""

    def __init__(self, name, ints, mass, unit, cutoff_units, cell, bounds, planted=(), k=0, base=None):
        self.name, self.k, self.base = name, k, base
        self.ints = np.ascontiguousarray(ints, np.int64)
        assert np.abs(self.ints).max() < (1 << 24)
        self.mass = np.ascontiguousarray(mass, F)
        self.n = self.ints.shape[0]
        assert self.n <= 2500
        self.unit = float(unit)
        assert math.frexp(self.unit)[0] == 0.5, "the unit is a power of two"
        self.cutoff_units = int(cutoff_units)
        self.cutoff = F(self.cutoff_units * self.unit)
        self.c2_units = int(round24(self.cutoff_units ** 2))      # cutoff2 / unit^2 = fl(cutoff cutoff) / unit^2
        self.cell = F(cell)
        self.bounds = tuple(F(b) for b in bounds)
        self.planted = list(planted)

    @property
    def cutoff2(self):
        return F(self.cutoff * self.cutoff)

    def eps(self, fraction):
        """eps = fraction x cutoff as a float32 (scales with the population: rounding commutes with a power of two)"""
        return F(np.float64(fraction) * np.float64(self.cutoff))

    def pos(self):
        return (self.ints.astype(np.float64) * self.unit).astype(F)

    @property
    def posm(self):
        p = np.empty((self.n, 4), F)
        p[:, :3] = self.pos()
        p[:, 3] = self.mass
        return p

    def ic(self):
        p = self.pos()
        return {"pos_x": np.ascontiguousarray(p[:, 0]), "pos_y": np.ascontiguousarray(p[:, 1]),
                "pos_z": np.ascontiguousarray(p[:, 2]), "mass": self.mass}

    def dims(self):
        """ceilf(fl(fl(hi - lo) / cell)) + 1 per axis, as the build forms them"""
        lo, hi = np.array(self.bounds[:3], F), np.array(self.bounds[3:], F)
        return tuple(int(v) + 1 for v in np.ceil(((hi - lo).astype(F) / self.cell).astype(F)))

    def cells_xyz(self, pos=None):
        """cell coordinates [n, 3]: min(max(int(floorf(fl(fl(p - lo) / cell))), 0), dim - 1)"""
        p = self.pos() if pos is None else np.asarray(pos, F)
        lo = np.array(self.bounds[:3], F)
        q = np.floor(((p - lo[None, :]).astype(F) / self.cell).astype(F)).astype(np.int64)
        return np.clip(q, 0, np.array(self.dims(), np.int64)[None, :] - 1)

    def cells(self, pos=None):
        c, d = self.cells_xyz(pos), self.dims()
        return (c[:, 0] + d[0] * (c[:, 1] + d[1] * c[:, 2])).astype(np.int32)

    def scaled(self, k):
        """positions, cell, bounds, cutoff (and eps, through eps()) times 2^k, masses times 4^k"""
        s = Population(f"{self.name} x 2^{k}", self.ints, np.ldexp(self.mass, 2 * k).astype(F), math.ldexp(self.unit, k),
                       self.cutoff_units, np.ldexp(self.cell, k), [np.ldexp(b, k) for b in self.bounds], self.planted, k,
                       self)
        assert np.all(np.isfinite(s.posm)) and np.all(s.mass > 0) and np.isfinite(s.cutoff2) and s.cutoff2 > 0
        return s


def scale_exponents(pop):
    """(largest k whose cutoff2 still passes cut_const_ok, the smallest k whose cutoff2 does not, the negative k nearest 0
    that takes eps2 = (0.05 cutoff)^2 below the GUARD threshold) -- from the limits in csrc/spatial_hash.hip"""
    _, hi, guard = limits()

    def c2(k):
        with np.errstate(over="ignore"):
            c = np.ldexp(pop.cutoff, k)
            return F(c * c)

    def e2(k):
        e = np.ldexp(pop.eps(EPS_FRACTION), k)
        return F(e * e)
    k_in = max(k for k in range(0, 64) if c2(k) <= hi)
    k_neg = max(k for k in range(-64, 0) if e2(k) < guard)
    assert c2(k_in + 1) > hi and e2(k_neg + 1) >= guard
    return k_in, k_in + 1, k_neg


def lattice_vectors(s, reach=6):
    """integer vectors of squared length s"""
    r = range(-reach, reach + 1)
    return np.array([v for v in itertools.product(r, r, r) if v[0] * v[0] + v[1] * v[1] + v[2] * v[2] == s], np.int64)


def below_lattice(s):
    """the largest squared length of an integer vector below s"""
    return max(t for t in range(s) if len(lattice_vectors(t)))


TIES_L = 16
TIES_CELLS = {"faces": (6.0, (0.0, 0.0, 0.0, 15.0, 15.0, 15.0)),                 # bodies at 6 and 12 lie ON cell faces
              "off": (5.05, (-0.37, -1.21, -0.83, 15.4, 15.9, 15.2))}            # bounds off the lattice


def ties(cutoff_units, cells, sparse=False):
    assert cutoff_units in (4, 5) and cells in TIES_CELLS
    L = TIES_L
    rng = np.random.default_rng(1000 * cutoff_units + 10 * sorted(TIES_CELLS).index(cells) + int(sparse))
    sites = np.array(list(itertools.product(range(L), range(L), range(L))), np.int64)
    if not sparse:
        pts = sites[rng.random(L ** 3) < 0.5]
    else:
        c2 = cutoff_units ** 2
        at, under = lattice_vectors(c2), lattice_vectors(below_lattice(c2))
        chosen = set()
        def step(s, vs):
            ok = vs[np.all((s + vs >= 0) & (s + vs < L), axis=1)]
            return s + ok[rng.integers(len(ok))]
        for s in sites[rng.random(L ** 3) < 0.0075]:
            b = step(s, under)
            chosen.update(tuple(v) for v in (s, step(s, at), b, step(b, at)))
        pts = np.array(sorted(chosen), np.int64)
    pts = np.concatenate([pts, pts[rng.choice(len(pts), len(pts) // 10, replace=False)]])   # coincident pairs
    pts = pts[rng.permutation(len(pts))]
    mass = rng.uniform(0.5, 1.5, len(pts)).astype(F)   # (random: the tie vectors of a body do not cancel)
    cell, bounds = TIES_CELLS[cells]
    return Population(f"ties cutoff {cutoff_units} cell {cell}{' sparse' if sparse else ''}", pts, mass, 1.0, cutoff_units,
                      cell, bounds)


# ---- the one-ulp stars ------------------------------------------------------------------------------------------------------
def search_offset(cutoff_units, ulps):
    """the first offset (i >= j >= k >= 0, j <= cutoff / 8; largest i, then smallest j, then smallest k) whose float32 d2 is
    the float `ulps` from cutoff2"""
    target = int(neighbour(F(int(round24(cutoff_units ** 2))), ulps))
    jmax = cutoff_units // 8
    j, k = np.meshgrid(np.arange(jmax + 1), np.arange(jmax + 1), indexing="ij")
    for i in range(math.isqrt(target) + 2, math.isqrt(target) - 256, -1):
        hit = (dist2_fp32(i, j, k) == target) & (k <= j)
        if hit.any():
            jj, kk = np.argwhere(hit)[0]
            return int(i), int(jj), int(kk)
    raise AssertionError(f"no offset {ulps} ulps from the cutoff {cutoff_units}")


# cutoff in units of 2^-11 (3001 q, 4095 q, 2897 q -- just above 2^23 q^2 -- and 4096 q, a power-of-two cutoff2):
# {ulps from cutoff2: offset}.  The even offsets are twice the integer offsets in q (exact sums of squares below 2^24 q^2);
# the others come from search_offset (tests/test_hash_pairs_cpu.py derives them again): M - 2 q^2 is 7 mod 8 for 3001 q,
# and so is the float below 2^24 q^2, so only a ROUNDED sum lands there; (8192, 2, 2) rounds to 2^26 itself.
ONE_ULP = {
    6002: {-2: (5996, 259, 70), -1: (5992, 344, 40), 0: (6002, 0, 0), 1: (6002, 2, 0), 2: (6002, 2, 2)},
    8190: {-1: (8064, 1408, 256), 0: (8190, 0, 0)},
    5794: {-1: (5792, 152, 8), 0: (5794, 0, 0)},
    8192: {-1: (8191, 91, 90), 0: (8192, 0, 0), 1: (8192, 3, 0)},
}
ONE_ULP_SEARCHED = ((6002, -2), (8192, -1), (8192, 1))


def signed_permutations(v):
    out = set()
    for p in itertools.permutations(v):
        for s in itertools.product((1, -1), repeat=3):
            out.add(tuple(int(a * b) for a, b in zip(p, s)))
    return sorted(out)


def one_ulp(cutoff_units):
    """the star population of one cutoff.  A star, in input order: n fillers in the cell at x - 1 of the satellite's row
    (beyond the cutoff from the centre), on every fifth star a body 0.4 cutoff from the centre in the centre's cell, the
    centre, the satellite, and -- where that makes fewer than three -- one more body in the last cell of the window."""
    c = cutoff_units
    cu = 2 * ((101 * c + 199) // 200) + 2            # the cell in units: even, >= 1.01 cutoff
    assert cu >= 1.01 * c and cu % 2 == 0
    stars = []
    for u, off in sorted(ONE_ULP[c].items()):
        perms = signed_permutations(off)
        stars += [(u, sp) for sp in perms * -(-12 // len(perms))]     # at least twelve stars of every class
    side = math.ceil(len(stars) ** (1.0 / 3.0) - 1e-9)
    rng = np.random.default_rng(c)
    pts, planted = [], []
    long_runs, short_runs = {}, {}
    for s, (u, sp) in enumerate(stars):
        g = (s % side, (s // side) % side, s // (side * side))
        ctr = np.array([(4 * gi + 1) * cu + cu // 2 for gi in g], np.int64)      # the middle of cell 4 g + 1
        r = [int(np.sign(a)) if abs(a) > cu // 2 else 0 for a in sp]              # the satellite's cell, relative
        assert sum(abs(a) for a in r) == 1
        # the place of the satellite in its run: 0 .. 7, and for two stars of every class whose satellite lies at + x the
        # last place of a run of 33 and of 65 entries
        if r[0] == 1 and long_runs.get(u, 0) < 2:
            want = (32, 64)[long_runs.get(u, 0)]
            long_runs[u] = long_runs.get(u, 0) + 1
        else:
            want = short_runs.get(u, 0) % 8
            short_runs[u] = short_runs.get(u, 0) + 1
        near = s % 5 == 3
        n_pre = max(want - (1 + int(near) if r[0] == 1 else 0), 0)
        star = [ctr + np.array([-(145 * c) // 100, r[1] * (9 * c) // 10 + (i + 1) * (c // 256),
                                r[2] * (9 * c) // 10 - (i + 1) * (c // 300)]) for i in range(n_pre)]
        if near:
            star.append(ctr + np.array([(2 * c) // 5, 0, 0]))
        planted.append((len(pts) + len(star), len(pts) + len(star) + 1, u))
        star += [ctr, ctr + np.array(sp)]
        if len(star) < 3:
            star.append(ctr + np.array([(145 * c) // 100, (9 * c) // 10, (9 * c) // 10]))
        pts += star
    pts = np.array(pts, np.int64)
    hi = 4 * side * cu * ONE_ULP_UNIT
    return Population(f"one ulp cutoff {c}", pts, rng.uniform(0.5, 1.5, len(pts)).astype(F), ONE_ULP_UNIT, c,
                      cu * ONE_ULP_UNIT, (0.0, 0.0, 0.0, hi, hi, hi), planted)


def planted_ulps(pop):
    """per planted pair: how many floats its d2 lies from cutoff2 (negative: below) -- a permutation of a searched offset
    sums in another order and may round to another float than the intended one"""
    out = []
    for ctr, sat, _ in pop.planted:
        d = pop.ints[sat] - pop.ints[ctr]
        d2 = F(int(dist2_fp32(*d)))
        c2 = F(pop.c2_units)
        u, v = 0, c2
        while v != d2:
            u += 1 if d2 > c2 else -1
            v = np.nextafter(v, F(np.inf) if d2 > c2 else F(-np.inf))
            assert abs(u) <= 64, "a planted pair far from the cutoff"
        out.append(u)
    return np.array(out)


def window_places(pop):
    """per planted pair (place of the satellite in its run of the centre's window, length of that run, place in the whole
    window, length of the window): the nine runs are the cells x - 1 .. x + 1 of the rows y - 1 .. y + 1, z - 1 .. z + 1 in
    cell order, a cell's bodies in input order (the stable sort)"""
    xyz, keys, dims = pop.cells_xyz(), pop.cells().astype(np.int64), pop.dims()
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    out = []
    for ctr, sat, _ in pop.planted:
        cx, cy, cz = xyz[ctr]
        before, found = 0, None
        for r in range(9):
            yy, zz = cy + r % 3 - 1, cz + r // 3 - 1
            if not (0 <= yy < dims[1] and 0 <= zz < dims[2]):
                continue
            base = (zz * dims[1] + yy) * dims[0]
            k0 = np.searchsorted(sk, base + max(cx - 1, 0))
            k1 = np.searchsorted(sk, base + min(cx + 2, dims[0]))
            run = order[k0:k1]
            at = np.flatnonzero(run == sat)
            if at.size:
                found = (int(at[0]), len(run), before + int(at[0]))
            before += len(run)
        assert found is not None, "a satellite outside its centre's window"
        out.append(found + (before,))
    return np.array(out)


# ---- the populations of the tests, built once ----------------------------------------------------------------------------------
TIES = (("ties", 5, "faces", False), ("ties", 5, "off", False), ("ties", 4, "faces", False), ("ties", 4, "off", False))
SPARSE = (("ties", 5, "faces", True), ("ties", 4, "off", True))
STARS = tuple(("one_ulp", c) for c in sorted(ONE_ULP))
KEYS = TIES + SPARSE + STARS
SCALED = (("ties", 5, "faces", False), ("one_ulp", 6002))     # the populations that are also run scaled
FIELD = (("ties", 5, "faces", False), ("ties", 4, "off", False))   # ... cut into two slabs, and whose field is taken


def field_sites():
    """the points of the field test: every site of the ties lattice, occupied or not"""
    return np.array(list(itertools.product(range(TIES_L), range(TIES_L), range(TIES_L))), np.int64)
_memo = {}


def population(key, k=0):
    if (key, k) not in _memo:
        _memo[key, k] = population(key).scaled(k) if k else (ties(*key[1:]) if key[0] == "ties" else one_ulp(key[1]))
    return _memo[key, k]


def reference_of(key, fraction, k=0, **kw):
    """reference() of a population at eps = fraction x cutoff, kept"""
    tag = ("ref", key, k, fraction, tuple(sorted(kw.items())))
    if tag not in _memo:
        pop = population(key, k)
        _memo[tag] = reference(pop, pop.eps(fraction), **kw)
    return _memo[tag]


# ---- the reference ---------------------------------------------------------------------------------------------------------
def reference(pop, eps, targets=None, le=False, shift_ulps=0, exact_h=False, G=1.0, block=128):
    """fp64 sums over the pairs that pass `d2 < cutoff2` (le: <=; shift_ulps: cutoff2 replaced by the float that many floats
    away -- the mutants of the sharpness test).  targets None: the bodies on each other, a body never on itself;
    else lattice points [m, 3] (a point on a body: a coincident pair).  exact_h: h = |d|^2 + eps2 without any rounding,
    as the oracle's fp64 sum takes it (the decision stays on the float32 d2).
    -> dict: acc [m, 3], kappa [m], sabs [m], count [m] (pairs that passed), pairs (i [p], j [p]) int32, phi [m] and
    phi_scale [m] (the shifted potential -m_j (h^-1/2 - shift) of the field kernel and sum m_j h^-1/2; a coincident pair
    counts unless eps2 is below the GUARD threshold)"""
    src = pop.ints
    tgt = src if targets is None else np.asarray(targets, np.int64)
    m_t = tgt.shape[0]
    eps2 = F(F(eps) * F(eps))
    c2 = F(pop.c2_units)
    thr = float(neighbour(c2, shift_ulps))
    u2 = F(pop.unit * pop.unit)
    guard = eps2 < limits()[2]
    cutoff2 = F(c2 * u2)
    assert cutoff2 == pop.cutoff2
    shift = 1.0 / math.sqrt(float(cutoff2) + float(eps2))
    mass = pop.mass.astype(np.float64)
    acc, sabs = np.zeros((m_t, 3)), np.zeros(m_t)
    count = np.zeros(m_t, np.int64)
    phi, phis = np.zeros(m_t), np.zeros(m_t)
    pi, pj = [], []
    for b0 in range(0, m_t, block):
        rows = np.arange(b0, min(b0 + block, m_t))
        d = src[None, :, :] - tgt[rows, None, :]
        d2 = dist2_fp32(d[..., 0], d[..., 1], d[..., 2])
        d2f = d2.astype(np.float64)
        ok = (d2f <= thr) if le else (d2f < thr)
        if targets is None:
            ok[np.arange(rows.size), rows] = False
        ii, jj = np.nonzero(ok)                                             # everything below: the accepted pairs only
        dd, dd2 = d[ii, jj], d2[ii, jj]
        if exact_h:
            h = (dd * dd).sum(1).astype(np.float64) * float(u2) + float(eps2)
        else:
            h = ((dd2.astype(np.float64) * float(u2)).astype(F) + eps2).astype(np.float64)   # the float32 value of d2 + eps2
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(dd2 > 0, mass[jj] * h ** -1.5, 0.0)
            p = np.where((dd2 > 0) | (not guard), mass[jj] * h ** -0.5, 0.0)
        t = w[:, None] * (dd.astype(np.float64) * pop.unit)
        nr = rows.size
        for a in range(3):
            acc[rows, a] = G * np.bincount(ii, t[:, a], nr)
        sabs[rows] = G * np.bincount(ii, np.linalg.norm(t, axis=1), nr)
        count[rows] = np.bincount(ii, minlength=nr)
        phis[rows] = G * np.bincount(ii, p, nr)
        phi[rows] = -G * np.bincount(ii, p - np.where(p > 0, mass[jj] * shift, 0.0), nr)
        pi.append((rows[ii]).astype(np.int32))
        pj.append(jj.astype(np.int32))
    norm = np.linalg.norm(acc, axis=1)
    kappa = np.where(norm > 0, sabs / np.where(norm > 0, norm, 1.0), 0.0)
    return {"acc": acc, "kappa": kappa, "sabs": sabs, "count": count, "pairs": (np.concatenate(pi), np.concatenate(pj)),
            "phi": phi, "phi_scale": phis}


def pair_d2(pop, pairs):
    """the integer d2 / unit^2 of the listed pairs"""
    d = pop.ints[pairs[1]] - pop.ints[pairs[0]]
    return dist2_fp32(d[:, 0], d[:, 1], d[:, 2])


# ---- cut_const and the clamped FMA, restated --------------------------------------------------------------------------------
def cut_const(cutoff2):
    """(-1 / h, K) of cut_const(cutoff2): the bit manipulation and the float32 product and sum of the source"""
    cm = np.array([cutoff2], F).view(np.uint32)[0] - np.uint32(1)
    e = (int(cm) >> 23) & 255
    big = np.array([(277 - e) << 23], np.uint32).view(F)[0]
    cmf = np.array([cm], np.uint32).view(F)[0]
    return F(-big), F(F(cmf * big) + F(1.0))


def clamped_fma(d2, nbig, k):
    """clamp(fma(d2, nbig, k)) to [0, 1] in float32 with one rounding: the exact value as a fraction, rounded once"""
    from fractions import Fraction
    d2 = F(d2)
    if np.isinf(d2):
        return F(0.0)                                                  # fma(inf, -big, K) = -inf
    x = Fraction(float(d2)) * Fraction(float(nbig)) + Fraction(float(k))
    if x <= 0:
        return F(0.0)
    if x >= 1:
        return F(1.0)
    # (0, 1): round once to float32 -- through the nearest double, which is exact enough only away from float32's ties;
    # the caller's claim is that this branch is never taken
    return F(float(x))
