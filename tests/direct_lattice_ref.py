"""The exact tier of the Direct N^2 kernels: bodies on an integer lattice, integers all the way down (DESIGN.md 4.1,
"Testing every kernel form pair by pair").  Plain numpy, no GPU.

Construction.  Positions are distinct sites of a 32 x 32 x 20 integer lattice, centred: x, y in [-16, 15], z in
[-10, 9] (20,480 sites).  Masses are small integers, G = 1, eps^2 = 2^40 (eps = 2^20).  Every pair then has
d^2 <= 31^2 + 31^2 + 19^2 = 2,283 < 2^16 = half an ulp of 2^40, so fma(dx, dx, fma(dy, dy, fma(dz, dz, eps2))) IS 2^40,
rsq gives 2^-20, the common factor is 2^-60 for every pair, and a contribution is 2^-60 m_j (p_j - p_i): 2^-60 times an
integer.  Every partial sum of every kernel form is 2^-60 times an integer below 2^24, so fp32 FMAs, fp32 slot planes,
fp64 atomics, fp64 folds and the final rounding to fp32 lose nothing, in any order.  In units of G 2^-60:

    u_i = (sum_j m_j p_j) - (sum_j m_j) p_i                      (O(N), int64)

A pair (i, j) left out, counted twice or credited to another body moves u_i by +- m_j (p_j - p_i), a non-zero integer
vector (sites are distinct): at least one whole unit, whatever N is."""
from dataclasses import dataclass

import numpy as np

LX, LY, LZ = 32, 32, 20
NSITES = LX * LY * LZ                # 20,480
EPS = float(2.0 ** 20)               # the SoA entry points take eps
EPS2 = float(2.0 ** 40)
G = 1.0
UNIT = 2.0 ** -60                    # a = u G UNIT
PHI_UNIT = 2.0 ** -20                # phi = -G PHI_UNIT sum m_j
D2_MAX = 31 * 31 + 31 * 31 + 19 * 19
ASSIGNMENTS = ("index", "permuted")
EQUAL_MASSES = ("ones", "threes")
GENERAL_MASSES = ("g123", "g0123")
MASSES = EQUAL_MASSES + GENERAL_MASSES
PERM_SEED = 20480


def all_sites():
    """site k -> (k % 32 - 16, (k // 32) % 32 - 16, k // 1024 - 10), int64 [NSITES, 3]"""
    k = np.arange(NSITES, dtype=np.int64)
    return np.stack([k % LX - LX // 2, (k // LX) % LY - LY // 2, k // (LX * LY) - LZ // 2], 1)


def mass_pattern(n, masses):
    """int64 [n].  ones / threes: the equal-mass instantiation; g123: values in {1, 2, 3}; g0123: the same with a zero
    on every 97th body (bodies 96, 193, ...: at most n / 97 of them).  The general patterns start 1, 2, ... so that no
    n >= 2 happens to be uniform."""
    if isinstance(masses, np.ndarray):
        assert masses.shape == (n,)
        return masses.astype(np.int64)
    if masses == "ones":
        return np.full(n, 1, np.int64)
    if masses == "threes":
        return np.full(n, 3, np.int64)
    if masses in GENERAL_MASSES:
        m = np.random.default_rng(123 if masses == "g123" else 1230).integers(1, 4, NSITES).astype(np.int64)
        m[0], m[1] = 1, 2
        if masses == "g0123":
            m[96::97] = 0
        return m[:n].copy()
    raise ValueError(masses)


@dataclass
class Lattice:
    p: np.ndarray        # int64 [n, 3] sites
    m: np.ndarray        # int64 [n] masses

    @property
    def n(self):
        return self.p.shape[0]

    @property
    def packed(self):
        """float32 [n, 4] {x, y, z, m}: what the packed entry points take"""
        return np.ascontiguousarray(np.concatenate([self.p, self.m[:, None]], 1).astype(np.float32))

    def cut(self, lo, hi):
        return Lattice(self.p[lo:hi].copy(), self.m[lo:hi].copy())

    def decode(self, i, delta, R, src=None):
        return decode(self, i, delta, R, src)


def lattice(n, assignment="index", masses="ones", nonzero=False):
    """n bodies on distinct sites.  assignment: 'index' = body i on site i, 'permuted' = a fixed seeded permutation of
    the sites.  nonzero: only sites without a zero coordinate (a body there does not move under a displacement far below
    its ulp: the integrator test)."""
    s = all_sites()
    if nonzero:
        s = s[np.all(s != 0, axis=1)]
    assert 0 < n <= s.shape[0], (n, s.shape[0])
    if assignment == "permuted":
        s = s[np.random.default_rng(PERM_SEED).permutation(s.shape[0])]
    elif assignment != "index":
        raise ValueError(assignment)
    return Lattice(s[:n].copy(), mass_pattern(n, masses))


# ---- the O(N) int64 expectation -------------------------------------------------------------------------------------
def expect_all_pairs(lat):
    """u [n, 3] int64: every body against all the others (the self pair contributes 0)"""
    return (lat.m[:, None] * lat.p).sum(0)[None, :] - lat.m.sum() * lat.p


def expect_two_sets(a, b):
    """(u on A from B, u on B from A), int64"""
    ua = (b.m[:, None] * b.p).sum(0)[None, :] - b.m.sum() * a.p
    ub = (a.m[:, None] * a.p).sum(0)[None, :] - a.m.sum() * b.p
    return ua, ub


def expect_points(pts2, src):
    """Arbitrary target points given as TWICE their coordinates (int64 [M, 3]: lattice sites are even, half-integer points
    odd).  Returns (u2 [M, 3] int64 = 2 u, msum): a = u2 G UNIT / 2, phi = -G PHI_UNIT msum for every point.  A point
    that coincides with a source gets d = 0 from it in the force and its m_j in the potential (direct_field_kernel)."""
    pts2 = np.asarray(pts2, np.int64)
    u2 = 2 * (src.m[:, None] * src.p).sum(0)[None, :] - src.m.sum() * pts2
    return u2, int(src.m.sum())


def acc_rows(u, scale=UNIT, prefill=None):
    """float32 [n, 4] rows {a, 0} of the integers u (exactly: asserts that nothing is rounded); prefill: int64 [n, 3] in the
    same unit, added (the accumulate forms)"""
    u = np.asarray(u, np.int64)
    if prefill is not None:
        u = u + np.asarray(prefill, np.int64)
    assert np.abs(u).max(initial=0) < 2 ** 24
    out = np.zeros((u.shape[0], 4), np.float32)
    out[:, :3] = (u.astype(np.float64) * scale).astype(np.float32)
    assert np.array_equal(out[:, :3].astype(np.float64) / scale, u)
    return out


def units(a, scale=UNIT):
    """back to units: float64 [n, 3] (integers when all is well) of float32 accelerations"""
    return np.asarray(a, np.float64)[:, :3] / scale


# ---- brute force, for the CPU tests -----------------------------------------------------------------------------------
def brute_points(pts2, src):
    """O(N M) int64 double loop of expect_points"""
    pts2 = np.asarray(pts2, np.int64)
    u2 = np.zeros(pts2.shape, np.int64)
    for i in range(pts2.shape[0]):
        for j in range(src.n):
            u2[i] += src.m[j] * (2 * src.p[j] - pts2[i])
    return u2, int(sum(int(x) for x in src.m))


# ---- fp32 emulation of the pair arithmetic, scalar form (direct.hip: interact) -----------------------------------------
def fma32(a, b, c):
    """fmaf for operands whose product and sum are exact in float64 (integers below 2^16 and 2^40): one rounding"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def pair_r2(d):
    """r2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, eps2))) of float32 differences d [..., 3]"""
    e2 = np.float32(EPS2)
    return fma32(d[..., 0], d[..., 0], fma32(d[..., 1], d[..., 1], fma32(d[..., 2], d[..., 2], np.broadcast_to(e2, d.shape[:-1]))))


def pair_terms(lat, i):
    """the fp32 terms f d of body i against every source, [n, 3] float32, with f = (m inv) (inv inv), inv = 1 / sqrt(r2)"""
    p32 = lat.p.astype(np.float32)
    d = p32 - p32[i]
    inv = (np.float32(1.0) / np.sqrt(pair_r2(d))).astype(np.float32)
    f = (lat.m.astype(np.float32) * inv) * (inv * inv)
    return (f[:, None] * d).astype(np.float32)


def running_sum32(terms, order):
    """one fp32 accumulator over terms[order], left to right"""
    return np.add.accumulate(terms[order].astype(np.float32), axis=0, dtype=np.float32)[-1]


# ---- failure messages --------------------------------------------------------------------------------------------------
def where(j, R):
    """(superblock, 64-body chunk of it, lane) of body j at R bodies per lane (superblocks of 256 R bodies)"""
    S = 256 * R
    return j // S, (j % S) // 64, j % 64


def decode(lat, i, delta, R, src=None):
    """Which partner explains delta = u_i - ref_i?  Every j with delta = s k m_j (p_j - p_i), s = +-1, k in {1, 2}, as
    dicts {i, j, sign, k, superblock, chunk, lane, d}: j's place at R bodies per lane and the ring offset d from i's
    superblock to j's (the kernel visits the pair from the I side at offset d when d <= NB / 2, from j's side at NB - d
    otherwise).  src: the partners are the bodies of ANOTHER set (two sets, points against bodies; d is then j's superblock
    itself, as the two-set kernel addresses it).  Sorted by k, then by distance.  The list may hold a few: a pair left out
    looks like the pair with the mirror image of j in p_i counted twice, and with general masses a lighter body twice as
    far explains the same vector.  The true partner is always among them."""
    delta = np.asarray(np.rint(delta), np.int64)
    S = 256 * R
    own = src is None
    src = lat if own else src
    NB = (src.n + S - 1) // S
    out = []
    rel = src.m[:, None] * (src.p - lat.p[i])
    for k in (1, 2):
        for s in (1, -1):
            hit = np.all(s * k * rel == delta[None, :], axis=1) & (src.m > 0)
            if own:
                hit[i] = False
            for j in np.nonzero(hit)[0]:
                sb, chunk, lane = where(int(j), R)
                out.append({"i": int(i), "j": int(j), "sign": s, "k": k, "superblock": sb, "chunk": chunk, "lane": lane,
                            "d": (sb - i // S) % NB if own else sb, "dist2": int(((src.p[j] - lat.p[i]) ** 2).sum())})
    out.sort(key=lambda c: (c["k"], c["dist2"]))
    return out


def describe(lat, u, ref, R, src=None, limit=4):
    """the first few failing bodies of u [n, 3] against ref, decoded (src: see decode)"""
    u = np.asarray(u, np.float64)
    ref = np.asarray(ref, np.float64)
    bad = np.nonzero(np.any(u != ref, axis=1))[0]
    S = 256 * R
    lines = [f"{bad.size} of {lat.n} bodies differ (R = {R}, superblocks of {S})"]
    for i in bad[:limit]:
        dl = u[i] - ref[i]
        if not np.all(np.isfinite(dl)) or np.any(dl != np.rint(dl)) or np.abs(dl).max() > 2 ** 30:
            lines.append(f"  body {i} (superblock {i // S}, chunk {(i % S) // 64}, lane {i % 64}): delta {dl.tolist()} is no "
                         "integer vector: a stale or unwritten slot, or padding that leaks")
            continue
        c = decode(lat, int(i), dl, R, src)
        who = "; ".join(f"{'+' if x['sign'] > 0 else '-'}{x['k']} x partner {x['j']} (superblock {x['superblock']}, chunk "
                        f"{x['chunk']}, lane {x['lane']}, ring offset d = {x['d']})" for x in c[:3]) or "no single partner"
        lines.append(f"  body {i} (superblock {i // S}, chunk {(i % S) // 64}, lane {i % 64}): delta {dl.astype(np.int64).tolist()}: {who}")
    return "\n".join(lines)


# ---- the cases of tests/test_direct_lattice_gpu.py (the CPU tests check their bounds) ------------------------------------
ONE_SIDED_SIZES = (2, 255, 256, 257, 513, 1025, 2049)
ONE_SIDED_FORMS = ((0, 1), (0, 2), (0, 4), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4))   # (variant, targets per lane)
ONE_SIDED_SPLITS = (0, 1, 3, 64)
SYM_R = (2, 4, 6, 8, 12, 16)
SYM_SPLITS = (0, 1, 5, 4096)
RECT_R = (2, 4, 6, 8, 16)
RECT_SPLITS = (0, 3)
RECT_MASSES = ("equal", "equal3", "a_differs", "general")
FIELD_SOURCES = (255, 257, 2049)
FIELD_POINTS = (300, 40000)


def sym_sizes(R):
    """by superblock count, the smallest that reach each branch: NB = 1 (diagonal only), 2 (even: one body in the last
    superblock, the partner at d = D skipped for A >= D), 3 (odd), 4 (full superblocks), 5 (ragged inside a chunk)"""
    S = 256 * R
    return (2, S - 1, S, S + 1, 2 * S + 1, 4 * S, 4 * S + 64 * 3 + 1)


# long rings, beyond the minimal sizes: (bodies per lane or 0 = the automatic choice, n) -> NB = 40 (even, 20 superblocks
# with A >= D), 39 (odd), 40 with one body in the last superblock, and what a plain call runs at all 20,480 sites
LONG_RINGS = ((2, NSITES), (2, 39 * 512), (2, 39 * 512 + 1), (0, NSITES))


def rect_shapes(R):
    S = 256 * R
    return ((1, 2 * S + 1), (S, S), (S + 1, 3 * S - 1), (2 * S + 65, 257))


def rect_sets(R, shape, assignment, masses):
    """two disjoint sets cut from one lattice.  equal: all 1; equal3: all 3; a_differs: A all 2, B all 1 (uniform within each set, not
    across: the general path through the cross-set test of mass_range); general: g0123"""
    na, nb = shape
    if masses in ("equal", "equal3"):
        lat = lattice(na + nb, assignment, "ones" if masses == "equal" else "threes")
    elif masses == "a_differs":
        m = np.ones(na + nb, np.int64)
        m[:na] = 2
        lat = lattice(na + nb, assignment, m)
    else:
        lat = lattice(na + nb, assignment, "g0123")
    return lat.cut(0, na), lat.cut(na, na + nb)


def field_points2(count, src, seed=5):
    """TWICE the coordinates of `count` points: every third one on a body (coincident), the rest anywhere on the
    half-integer lattice inside the box"""
    rng = np.random.default_rng(seed + count)
    pts2 = np.stack([rng.integers(-LX, LX - 1, count), rng.integers(-LY, LY - 1, count), rng.integers(-LZ, LZ - 1, count)], 1)
    on = np.arange(0, count, 3)
    pts2[on] = 2 * src.p[rng.integers(0, src.n, on.size)]
    return pts2.astype(np.int64)
