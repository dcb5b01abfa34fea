"""tests/hash_pair_ref.py checked without a GPU: the integer restatement of hash_dist2, the reference against the oracle
(two independent statements of the decision), and the CONDITIONS on the populations that make
tests/test_hash_pairs_gpu.py sharp -- enough pairs exactly on the edge, every mutant of the decision visible far
above the tier-1 bound, the planted pairs where they were meant to be.

Where this departs from the letter of the issue, and why:
  * 5 N pairs at d2 == cutoff2 cannot exist for cutoff 4: only 6 lattice vectors have length 4, half the sites are
    occupied and a quarter of the partners fall outside the lattice -- 2.25 per body, a little more with the
    duplicates.  Asserted there: 2 N (and 5 N at 14, the largest lattice value below 16).  The sparse populations are
    built so that every body has one tie: 0.9 N at the cutoff, 0.45 N below it.
  * On an integer lattice no d2 lies between cutoff2 and its float neighbours, so replacing cutoff2 by the neighbour
    BELOW moves no body of a ties population (asserted: none), the neighbour above acts like `<=`.  The neighbour below
    is what the stars of the one-ulp populations one float below cutoff2 are for.  Two more mutants (cutoff2 two floats
    below, three above) make the stars two floats below and one and two above flip as well.
  * The oracle's fp64 sum takes h = |d|^2 + eps2 without rounding, the reference takes the float32 value (the "gold"
    kind); 1e-6 holds between the oracle and the reference's exact_h form (same pairs, same terms), and the two forms
    of the reference differ by at most 6 u kappa (three roundings of d2 and one of the sum, to the power 3/2).
  * eps = 0 with coincident bodies: the oracle divides by zero there (the GUARD kernels skip such pairs, the reference
    counts them as 0); those bodies are compared on their zeros only.
"""
import numpy as np
import pytest

import hash_pair_ref as hp
from gpu_util import C_SUM, U, hash_bound, rel_err

F = np.float32
MUTANTS = {"<=": dict(le=True), "below": dict(shift_ulps=-1), "above": dict(shift_ulps=1),
           "two below": dict(shift_ulps=-2), "three above": dict(shift_ulps=3)}


def flips(ulps, mutant):
    """does a pair whose d2 lies `ulps` floats from cutoff2 change sides under the mutant?"""
    kw = MUTANTS[mutant]
    now = ulps <= 0 if kw.get("le") else ulps < kw["shift_ulps"]
    return now != (ulps < 0)


def moved(key, mutant):
    """per body |a_mutant - a| / |a| in units of the tier-1 bound with the largest C_SUM"""
    r, v = hp.reference_of(key, hp.EPS_FRACTION), hp.reference_of(key, hp.EPS_FRACTION, **MUTANTS[mutant])
    assert C_SUM[0] == max(C_SUM.values())
    norm = np.linalg.norm(r["acc"], axis=1)
    return np.linalg.norm(v["acc"] - r["acc"], axis=1) / np.where(norm > 0, norm, 1e-300) / hash_bound(r["kappa"], "gold", 0)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def test_round24_is_float32_rounding():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.integers(0, 1 << 53, 200000), rng.integers(0, 1 << 26, 100000),
                        ((np.arange(1 << 12) + (1 << 23)) << 4) + 8,            # ties, the kept bits even and odd
                        [0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 25) - 1, (1 << 25) + 2, (1 << 25) + 6]])
    assert np.array_equal(hp.round24(v).astype(np.float64), v.astype(np.float64).astype(F).astype(np.float64))


def test_dist2_equals_numpy_float32_where_every_intermediate_is_exact():
    rng = np.random.default_rng(2)
    ijk = rng.integers(-2300, 2301, (200000, 3))                 # 3 x 2300^2 < 2^24: nothing rounds
    x = ijk.astype(F)
    assert np.array_equal(hp.dist2_fp32(*ijk.T), (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]).astype(np.int64))
    # and where it rounds: one rounding per operation, the fused ones formed exactly in fp64 first
    big = rng.integers(-(1 << 13), (1 << 13) + 1, (200000, 3)).astype(np.float64)
    a = (big[:, 0] * big[:, 0]).astype(F).astype(np.float64)
    b = (big[:, 1] * big[:, 1] + a).astype(F).astype(np.float64)
    c = (big[:, 2] * big[:, 2] + b).astype(F)
    assert np.array_equal(hp.dist2_fp32(*big.astype(np.int64).T), c.astype(np.int64))


@pytest.mark.parametrize("key", hp.KEYS, ids=str)
def test_cutoff2_is_the_float32_square(key):
    for k in (0,) + (hp.scale_exponents(hp.population(key)) if key in hp.SCALED else ()):
        p = hp.population(key, k)
        assert F(p.c2_units) * F(p.unit * p.unit) == p.cutoff2 == F(p.cutoff * p.cutoff)
        assert float(p.cutoff2) == p.c2_units * p.unit * p.unit


def test_cut_const_and_the_clamped_fma_take_the_decision():
    """t = clamp(fma(d2, -1 / h, K)) with the constants of cut_const is exactly 1 where d2 < cutoff2 and exactly 0 elsewhere,
    over the whole range of cut_const_ok: powers of two, their neighbours, other mantissas, the limits themselves"""
    lo, hi, _ = hp.limits()
    rng = np.random.default_rng(3)
    cut = [lo, hp.neighbour(lo, 1), hi, hp.neighbour(hi, -1)]
    for e in range(-101, 102):
        p = F(2.0) ** e
        cut += [hp.neighbour(p, -1), p, hp.neighbour(p, 1), F(1.5) * p, hp.neighbour(F(2.0) * p, -2)]
        cut += list((F(1.0) + rng.integers(1, 1 << 23, 7).astype(F) * F(2.0 ** -23)) * p)
    cut = sorted({float(c) for c in cut if lo <= c <= hi})
    tiny, info = np.finfo(F).smallest_subnormal, np.finfo(F)
    n = 0
    for c in cut:
        c2 = F(c)
        nbig, k = hp.cut_const(c2)
        assert float(k) == int(k) and 2 ** 23 < int(k) <= 2 ** 24
        for d2 in (F(0.0), tiny, info.tiny, hp.neighbour(c2, -2), hp.neighbour(c2, -1), c2, hp.neighbour(c2, 1),
                   F(0.5) * c2, F(2.0) * c2, info.max, F(np.inf)):
            t = hp.clamped_fma(d2, nbig, k)
            assert t == (F(1.0) if d2 < c2 else F(0.0)), (c2, d2, t)
            n += 1
    assert n > 26000


def test_limits_are_read_from_the_source():
    lo, hi, guard = hp.limits()
    assert 2.0 ** -100 <= lo < 2.0 ** -99 and 2.0 ** 99 < hi <= 2.0 ** 100 and 0 < guard < 1e-6
    for key in hp.SCALED:
        p = hp.population(key)
        k_in, k_out, k_neg = hp.scale_exponents(p)
        assert k_out == k_in + 1 and k_neg < 0
        assert lo <= p.scaled(k_in).cutoff2 <= hi < p.scaled(k_out).cutoff2 and np.isfinite(p.scaled(k_out).cutoff2)
        e = p.scaled(k_neg).eps(hp.EPS_FRACTION)
        assert 0 < F(e * e) < guard <= F(p.eps(hp.EPS_FRACTION) ** 2) and p.scaled(k_neg).cutoff2 >= lo
        for k in (k_in, k_out, k_neg):                      # the same lattice, the same cells, the same mantissas
            s = p.scaled(k)
            assert np.array_equal(s.cells(), p.cells()) and s.dims() == p.dims()
            assert np.array_equal(np.ldexp(s.posm[:, :3], -k), p.posm[:, :3])
            assert np.array_equal(np.ldexp(s.posm[:, 3], -2 * k), p.posm[:, 3])
            assert np.ldexp(s.eps(hp.EPS_FRACTION), -k) == p.eps(hp.EPS_FRACTION)


# ---- the reference against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", [hp.EPS_FRACTION, 0.0])
@pytest.mark.parametrize("key", hp.KEYS, ids=str)
def test_reference_and_oracle_agree(oracle, key, fraction):
    p = hp.population(key)
    ic, eps = p.ic(), p.eps(fraction)
    _, gold, _ = oracle.spatial_hash_forces_cond(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], 1.0,
                                                 float(F(eps * eps)), float(p.cell), float(p.cutoff))
    r, x = hp.reference_of(key, fraction), hp.reference_of(key, fraction, exact_h=True)
    d2 = hp.pair_d2(p, r["pairs"])
    coincident = np.zeros(p.n, bool)
    coincident[r["pairs"][0][d2 == 0]] = True
    ok = np.ones(p.n, bool) if fraction else ~coincident          # (eps = 0: the oracle divides by zero on those)
    assert np.all(np.isfinite(gold[ok])) and coincident.any() == (key[0] == "ties")
    nz = np.linalg.norm(r["acc"], axis=1) > 0
    assert np.array_equal(nz[ok], np.linalg.norm(gold[ok], axis=1) > 0), "exact zeros"
    assert np.array_equal(np.linalg.norm(x["acc"], axis=1) > 0, nz)
    err = rel_err(x["acc"][nz & ok], gold[nz & ok])
    print(f"{p.name} eps {eps}: reference (exact h) against the oracle's fp64 sum: max {err.max():.3e}")
    assert err.max() <= 1e-6
    both = rel_err(r["acc"][nz], x["acc"][nz])
    assert np.all(both <= 6 * U * r["kappa"][nz] + 1e-12)


# ---- conditions on the populations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", hp.KEYS, ids=str)
def test_cells_hold_every_accepted_pair(key):
    """cell >= 1.01 cutoff, so every accepted pair lies in neighbouring cells -- and the grid gets a start array"""
    p = hp.population(key)
    assert float(p.cell) >= 1.01 * float(p.cutoff)
    xyz = p.cells_xyz()
    i, j = hp.reference_of(key, hp.EPS_FRACTION, le=True)["pairs"]     # (with the pairs exactly at the cutoff)
    assert np.abs(xyz[i] - xyz[j]).max() <= 1
    assert 0 < np.prod(p.dims()) <= 16 * p.n + 4096
    lo, hi = np.array(p.bounds[:3]), np.array(p.bounds[3:])
    assert np.all(p.pos() >= lo) and np.all(p.pos() <= hi)
    if key[0] == "ties" and key[2] == "faces":
        assert np.any(p.ints % 6 == 0) and float(p.cell) == 6.0     # bodies exactly on cell faces


@pytest.mark.parametrize("key", hp.TIES + hp.SPARSE, ids=str)
def test_ties_are_plentiful(key):
    p = hp.population(key)
    d2 = hp.pair_d2(p, hp.reference_of(key, hp.EPS_FRACTION, le=True)["pairs"])
    c2 = p.c2_units
    at, under = int((d2 == c2).sum()), int((d2 == hp.below_lattice(c2)).sum())
    vec = {s: len(hp.lattice_vectors(s)) for s in (14, 15, 16, 17, 24, 25, 26)}
    assert vec == {14: 48, 15: 0, 16: 6, 17: 48, 24: 24, 25: 30, 26: 72}
    want_at, want_under = ((0.9, 0.45) if key[3] else ((5, 5) if key[1] == 5 else (2, 5)))
    print(f"{p.name}: {p.n} bodies, {at / p.n:.2f} N pairs at cutoff2, {under / p.n:.2f} N at the lattice value below, "
          f"{int((d2 == 0).sum())} coincident")
    assert at >= want_at * p.n and under >= want_under * p.n and (d2 == 0).sum() >= 0.15 * p.n
    assert np.all((p.mass >= 0.5) & (p.mass <= 1.5))
    occ = len(np.unique(p.ints, axis=0)) / hp.TIES_L ** 3
    assert (0.02 < occ < 0.04) if key[3] else (0.45 < occ < 0.55)
    per_cell = np.bincount(p.cells())
    if key[3]:
        assert (per_cell[per_cell > 0] < 6).any() and (per_cell >= 6).any()     # light cells and crowded ones (split form)
    else:
        assert per_cell.max() > 64 and p.n > 4 * 512     # cells of more than 64 targets, windows of several LDS batches


@pytest.mark.parametrize("key", hp.TIES + hp.SPARSE, ids=str)
def test_ties_make_the_mutants_visible(key):
    for name in ("<=", "above"):
        m = moved(key, name)
        print(f"{hp.population(key).name}: `{name}` moves {100 * (m > 100).mean():.1f} % of the bodies by > 100 bounds")
        assert (m > 100).mean() >= 0.9
    assert not moved(key, "below").any()     # no lattice value between cutoff2 and the float below it: see the docstring


@pytest.mark.parametrize("key", hp.STARS, ids=str)
def test_planted_pairs(key):
    p = hp.population(key)
    c = key[1]
    ulps = hp.planted_ulps(p)
    # every class that was meant to be there is there (a permutation of a searched offset may round elsewhere)
    assert set(hp.ONE_ULP[c]) <= set(ulps.tolist()) and {-1, 0} <= set(ulps.tolist())
    for (ctr, sat, want), got in zip(p.planted, ulps):
        off = tuple(int(v) for v in p.ints[sat] - p.ints[ctr])
        if (c, want) not in hp.ONE_ULP_SEARCHED:
            assert got == want, (off, got, want)
        assert off in hp.signed_permutations(hp.ONE_ULP[c][want])
    # the searched offsets, derived again
    for cc, u in hp.ONE_ULP_SEARCHED:
        if cc == c:
            assert hp.search_offset(cc, u) == hp.ONE_ULP[cc][u]
            assert F(int(hp.dist2_fp32(*hp.ONE_ULP[cc][u]))) == hp.neighbour(F(p.c2_units), u)
    # a centre sees its satellite and at most the one body 0.4 cutoff away: none, one or two accepted partners
    r = hp.reference_of(key, hp.EPS_FRACTION)
    cnt = np.array([r["count"][ctr] for ctr, _, _ in p.planted])
    assert {0, 1} <= set(cnt.tolist()) and cnt.max() <= 2
    for (ctr, sat, _), u, n_acc in zip(p.planted, ulps, cnt):
        mine = r["pairs"][1][r["pairs"][0] == ctr]
        assert (sat in mine) == (u < 0) and n_acc == len(mine)
    # where the satellite sits in its centre's window: places 0 .. 7 of a run, the last place of runs and windows of 33 and 65
    w = hp.window_places(p)
    assert set(range(8)) <= set(w[:, 0].tolist())
    last = w[(w[:, 0] == w[:, 1] - 1) & (w[:, 2] == w[:, 3] - 1)]
    assert {33, 65} <= set(last[:, 1].tolist()) and {33, 65} <= set(last[:, 3].tolist())
    for u in set(ulps.tolist()):
        if u in (-1, 0):     # both sides of the edge itself at every place
            assert set(range(8)) <= set(w[ulps == u, 0].tolist())
    # stars are at least three cells apart: no accepted pair between two stars, no window reaches another star
    xyz = p.cells_xyz()
    gcell = xyz // 4
    assert np.all(xyz % 4 <= 2)
    i, j = r["pairs"]
    assert np.array_equal(gcell[i], gcell[j])
    assert np.bincount(np.unique(gcell, axis=0, return_inverse=True)[1].ravel()).min() >= 3     # three bodies a star
    # every mutant flips exactly the classes it should, and both bodies of a flipped pair move by > 100 bounds
    for name in MUTANTS:
        m = moved(key, name)
        for (ctr, sat, _), u in zip(p.planted, ulps):
            if flips(int(u), name):
                assert m[ctr] > 100 and m[sat] > 100, (name, int(u), m[ctr], m[sat])
    assert all(any(flips(int(u), name) for name in ("<=", "below", "above")) for u in (-1, 0))
    assert all(any(flips(int(u), name) for name in MUTANTS) for u in set(ulps.tolist()))


@pytest.mark.parametrize("key", hp.FIELD, ids=str)
def test_field_sites_sit_on_the_edge(key):
    """the points of the field test: half of them on a body (a coincident pair), nearly all exactly at the cutoff from
    several bodies -- and the population cut along z has ties across the cut"""
    p = hp.population(key)
    sites = hp.field_sites()
    eps = p.eps(hp.EPS_FRACTION)
    ref, wide = hp.reference(p, eps, targets=sites), hp.reference(p, eps, targets=sites, le=True)
    assert (wide["count"] > ref["count"]).mean() > 0.9
    occupied = {tuple(v) for v in p.ints.tolist()}
    on_body = np.array([tuple(v) in occupied for v in sites.tolist()])
    assert 0.4 < on_body.mean() < 0.6
    moved = np.linalg.norm(wide["acc"] - ref["acc"], axis=1) / np.maximum(np.linalg.norm(ref["acc"], axis=1), 1e-300)
    assert (moved > 100 * hash_bound(ref["kappa"], "gold", 2)).mean() > 0.9
