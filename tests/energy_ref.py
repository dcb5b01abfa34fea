"""fp64 restatement of the energy reductions of csrc/energy.hip for the tests (numpy only; every input is the fp32 value the
kernels read, widened to fp64), and the seeded body sets the energy tests share.

  kinetic    KE = sum_i 1/2 m_i v_i^2
  potential  PE = -G sum_{i<j} m_i m_j / sqrt(r_ij^2 + eps^2), eps^2 = fl32(eps * eps); a pair with r^2 + eps^2 == 0
             contributes nothing (the kernels' rule: csrc/energy.hip, the comment in the pair loop of potential_kernel)
  shard      (KE, PE share) of nbody_hip_energies_packed: PE share = -G/2 sum_i m_i sum_{j != self_offset + i} m_j / sqrt(.),
             the exclusion only where 0 <= self_offset + i < n_sources
  plan       (bx, tiles, splits, tiles_per_split): the host arithmetic in front of potential_kernel restated.  It picks and
             classifies shapes; no expected value comes from it.
  phi        phi_i = -G sum_{j != i} m_j / sqrt(.): potential_ref.direct_phi, the reference of the per-body potential, up to
             2,049 bodies; above that the same sum over the pair sweep of this file (a quarter of the time at 12,288 bodies;
             tests/test_energy_cpu.py holds the two to each other)
"""
import numpy as np

from potential_ref import direct_phi

SLOTS = 2048          # kNumCU * 8: the blocks the launch plan aims at
TILE = 256            # PTS = kBlock
KE_GRID_CAP = 1024    # blocks of the grid-stride kernels (kinetic_kernel, kinetic_packed_kernel, term_sum_kernel)


def _eps2(eps):
    return float(np.float32(eps) * np.float32(eps))


def _g(G):
    return float(np.float32(G))


def kinetic(vel, m):
    v = np.asarray(vel, np.float64)[:, :3]
    return float((0.5 * np.asarray(m, np.float64) * (v * v).sum(1)).sum())


def _inv_r(tp, sp, e2):
    """1 / sqrt(r^2 + eps^2) of every (target, source) pair, 0 where r^2 + eps^2 == 0"""
    r2 = np.full((tp.shape[0], sp.shape[0]), e2)
    for a in range(3):
        d = sp[None, :, a] - tp[:, None, a]
        r2 += d * d
    ok = r2 > 0
    return np.where(ok, 1.0 / np.sqrt(np.where(ok, r2, 1.0)), 0.0)


def potential(pos, m, G, eps, chunk=64):
    """every unordered pair once, from its lower index"""
    pos = np.asarray(pos, np.float64)[:, :3]
    m = np.asarray(m, np.float64)
    n, e2, total = len(m), _eps2(eps), 0.0
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        inv = _inv_r(pos[a:b], pos[a:], e2)                    # sources from the chunk's first body on ...
        inv[np.tril_indices(b - a, 0, inv.shape[1])] = 0.0     # ... and of those only j > i
        total += float((m[a:b] * (inv * m[None, a:]).sum(1)).sum())
    return -_g(G) * total


def phi(pos, m, G, eps, chunk=64):
    if len(m) <= 2049:
        return direct_phi(pos, m, _g(G), eps)
    pos = np.asarray(pos, np.float64)[:, :3]
    m = np.asarray(m, np.float64)
    n, e2 = len(m), _eps2(eps)
    out = np.empty(n)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        inv = _inv_r(pos[a:b], pos, e2)
        inv[np.arange(b - a), np.arange(a, b)] = 0.0
        out[a:b] = -_g(G) * (inv * m[None, :]).sum(1)
    return out


def shard(tpos, tm, tvel, self_offset, spos, sm, G, eps, pairs=1 << 16):
    tm, sm = np.asarray(tm, np.float64), np.asarray(sm, np.float64)
    nt, ns, e2, total = len(tm), len(sm), _eps2(eps), 0.0
    if ns == 0:
        return kinetic(tvel, tm), 0.0
    tpos, spos = np.asarray(tpos, np.float64)[:, :3], np.asarray(spos, np.float64)[:, :3]
    chunk = max(1, pairs // ns)
    for a in range(0, nt, chunk):
        b = min(a + chunk, nt)
        inv = _inv_r(tpos[a:b], spos, e2)
        own = int(self_offset) + np.arange(a, b)               # (Python integers: self_offset may be +-2^40)
        hit = (own >= 0) & (own < ns)
        inv[np.flatnonzero(hit), own[hit]] = 0.0
        total += float((tm[a:b] * (inv * sm[None, :]).sum(1)).sum())
    return kinetic(tvel, tm), -0.5 * _g(G) * total


def body_share(pos, m, G, eps, k):
    """what PE loses when body k is removed: twice body k's share as a shard of one"""
    pos = np.asarray(pos)
    return 2.0 * shard(pos[k:k + 1], np.asarray(m)[k:k + 1], np.zeros((1, 3)), k, pos, m, G, eps)[1]


def plan(n):
    bx = (n + TILE - 1) // TILE
    tiles = (n + TILE - 1) // TILE
    splits = max(1, min(64, (SLOTS + bx - 1) // bx, tiles))
    tiles_per_split = (tiles + splits - 1) // splits
    splits = (tiles + tiles_per_split - 1) // tiles_per_split
    return bx, tiles, splits, tiles_per_split


def regime(n):
    """which of the four shapes of the plan n has"""
    _, tiles, splits, per = plan(n)
    if splits == 1:
        return "one split"
    if per == 1:
        return "one tile per split"
    return "short last split" if tiles % per else "exact splits"


# ---- the body sets of tests/test_energy_cpu.py and tests/test_energy_gpu.py ----------------------------------------------------
G = 1.5                                    # (a value fp32 holds exactly)
EPS = (0.01, 0.0)
TOL = 1e-6                                 # KE and PE totals, relative
TOL_PHI = 1e-5                             # phi per body, relative
# 11520 = 45 * 256 is the last N whose splits hold one tile each (46 blocks: ceil(2048 / 46) = 45 < 46 tiles); 11521 the first
# with two tiles per split
ENERGY_SIZES = [1, 2, 3, 255, 256, 257, 511, 512, 513, 2049, 11520, 11521, 11777, 12288]
KINETIC_SIZES = [262144, 262145, 524289]   # the grid-stride loops take a second turn from 262145 on
PHI_SIZES = [1, 2, 255, 256, 257, 513, 2049, 11777, 12288]
FLOAT_SIZES = [257, 2049, 11777]
REUSE_SIZES = [12288, 3, 257, 11777, 1]
N_PACKED = 1000 + 13                       # the source set of the nbody_hip_energies_packed cases
ZERO_MASS_SIZES = {513: (1, 300), N_PACKED: (2, 900), 262145: (1, 262140)}    # the sets with two bodies of mass 0
_SENTINELS = (0, 255, 256, 262143, 262144)


def sentinels(n):
    """the indices where a dropped or doubled body is most likely: the ends, both sides of the first tile boundary, both
    sides of the first turn of a grid-stride loop"""
    return sorted({k for k in _SENTINELS if k < n} | {n - 1})


def sentinel_mass(n):
    """heavy enough that the loss of ONE such body moves KE and PE by 100 x TOL (tests/test_energy_cpu.py holds every set
    to that), light enough that the sentinels together stay a few per cent of the mass"""
    return np.float32(4.0 + 4e-3 * n)


_sets = {}


def bodies(n, seed=0):
    """(pos [n, 3], vel [n, 3], m [n]) in fp32: positions uniform in a box of one body per unit volume, masses uniform in
    [0.5, 2], speeds in [0.5, 1.5] in random directions; the sentinels heavy; ZERO_MASS_SIZES"""
    key = (n, seed)
    if key not in _sets:
        rng = np.random.default_rng(7000 + 31 * n + seed)
        pos = rng.uniform(0.0, max(1.0, n ** (1.0 / 3.0)), (n, 3)).astype(np.float32)
        m = rng.uniform(0.5, 2.0, n).astype(np.float32)
        d = rng.normal(size=(n, 3))
        vel = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (n, 1))).astype(np.float32)
        m[sentinels(n)] = sentinel_mass(n)
        if seed == 0:
            m[list(ZERO_MASS_SIZES.get(n, ()))] = 0.0
        for a in (pos, vel, m):
            a.setflags(write=False)
        _sets[key] = (pos, vel, m)
    return _sets[key]


def denormal_case(n=257):
    """eps = 0: the LAST body at (1e-20, 0, 0), every other body at least 1 from it and from the origin.  The padded target
    lanes of the last block sit AT the origin with mass 0: their r^2 to that body is 1e-40, a denormal, and the body lies in
    the one source tile that even the triangular sweep gives them (the tile of the block's own bodies)."""
    pos, vel, m = (a.copy() for a in bodies(n, seed=1))
    pos += np.float32(2.0)
    pos[n - 1] = (1e-20, 0.0, 0.0)
    return pos, vel, m


def as_ic(pos, vel, m):
    """the initial-condition dict of tests/gpu_util.to_device"""
    ic = {f"pos_{c}": np.ascontiguousarray(pos[:, k]) for k, c in enumerate("xyz")}
    ic.update({f"vel_{c}": np.ascontiguousarray(vel[:, k]) for k, c in enumerate("xyz")})
    ic["mass"] = np.ascontiguousarray(m)
    return ic
