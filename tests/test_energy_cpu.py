"""tests/energy_ref.py checked without a GPU: against closed forms, against the oracle's fp64 mode on bodies of unequal mass,
its shard pieces against its whole, and the body sets of tests/test_energy_gpu.py against the two conditions that make
that file's comparisons mean something -- the shapes cover the four regimes of the launch plan, and the loss of any ONE
sentinel body moves the reference by 100 x the tolerance the comparison uses."""
import math

import numpy as np
import pytest

import energy_ref as er
from oracle_bind import host_state

F = np.float32


def rel(a, b):
    return abs(a - b) / abs(b)


# ---- closed forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.25])
def test_two_bodies(eps):
    pos = np.array([[-1.5, 0, 0], [2.5, 0, 0]], F)
    vel = np.array([[1, 2, 2], [0, -4, 3]], F)
    m = np.array([3.0, 0.5], F)
    e2 = float(F(eps) * F(eps))
    pe = -1.5 * 3.0 * 0.5 / math.sqrt(16.0 + e2)
    assert er.kinetic(vel, m) == 0.5 * 3.0 * 9.0 + 0.5 * 0.5 * 25.0
    assert rel(er.potential(pos, m, 1.5, eps), pe) < 1e-15
    phi = er.direct_phi(pos, m, 1.5, eps)
    assert np.allclose(phi, [-1.5 * 0.5 / math.sqrt(16.0 + e2), -1.5 * 3.0 / math.sqrt(16.0 + e2)], rtol=1e-15, atol=0)
    for k in (0, 1):      # each body as a shard of one: half the pair
        ke, share = er.shard(pos[k:k + 1], m[k:k + 1], vel[k:k + 1], k, pos, m, 1.5, eps)
        assert rel(share, 0.5 * pe) < 1e-15 and ke == er.kinetic(vel[k:k + 1], m[k:k + 1])
    # the same body as a target that is NOT one of the sources sees both of them, itself at r = 0 included
    _, share = er.shard(pos[:1], m[:1], vel[:1], 2, pos, m, 1.5, 0.25)
    assert rel(share, -0.75 * 3.0 * (3.0 / 0.25 + 0.5 / math.sqrt(16.0 + 0.0625))) < 1e-15


def test_equilateral_triangle_with_unequal_masses():
    """(1,0,0), (0,1,0), (0,0,1): side sqrt 2, every coordinate exact in fp32"""
    pos, m = np.eye(3, dtype=F), np.array([1.0, 2.0, 4.0], F)
    for eps in (0.0, 0.5):
        r = math.sqrt(2.0 + float(F(eps) * F(eps)))
        assert rel(er.potential(pos, m, 1.5, eps), -1.5 * (2.0 + 4.0 + 8.0) / r) < 1e-15
        want = -1.5 * np.array([6.0, 5.0, 3.0]) / r          # phi_i = -G (the other two masses) / r
        assert np.allclose(er.direct_phi(pos, m, 1.5, eps), want, rtol=1e-15, atol=0)
        assert rel(0.5 * float((m * er.direct_phi(pos, m, 1.5, eps)).sum()), er.potential(pos, m, 1.5, eps)) < 1e-15


def test_a_coincident_pair_without_softening_contributes_nothing():
    pos = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 7]], F)
    m = np.array([2.0, 3.0, 5.0], F)
    assert er.potential(pos[:2], m[:2], 1.0, 0.0) == 0.0
    assert rel(er.potential(pos, m, 1.0, 0.0), -(2.0 * 5.0 + 3.0 * 5.0) / 4.0) < 1e-15
    assert er.shard(pos[:1], m[:1], pos[:1], 5, pos[:2], m[:2], 1.0, 0.0)[1] == 0.0       # disjoint by index, coincident in space
    assert rel(er.potential(pos[:2], m[:2], 1.0, 0.5), -6.0 / 0.5) < 1e-15            # with softening the pair counts
    assert er.potential(pos[:1], m[:1], 1.0, 0.0) == 0.0 and er.potential(pos[:0], m[:0], 1.0, 0.0) == 0.0


# ---- against the oracle's fp64 loops, unequal masses ---------------------------------------------------------------------------
@pytest.mark.parametrize("eps", er.EPS)
def test_reference_against_the_oracle_fp64_mode(oracle, eps):
    """ragged N, masses in [0.5, 2] and the heavy sentinels.  The oracle adds eps * eps in fp64, the reference (as the
    kernels) fl32(eps * eps): 6e-8 of 1e-4 in an r^2 of order 1 or more -- below 1e-10 of PE."""
    n = 1501
    pos, vel, m = er.bodies(n)
    assert np.unique(m).size > n // 2
    s = host_state(er.as_ic(pos, vel, m))
    ke, pe = oracle.kinetic_energy(s, 256, 2), oracle.potential_energy(s, er.G, eps, 256, 2)
    print(f"against the oracle, eps {eps}: KE {rel(er.kinetic(vel, m), ke):.2e}, PE {rel(er.potential(pos, m, er.G, eps), pe):.2e}")
    assert rel(er.kinetic(vel, m), ke) < 1e-13
    assert rel(er.potential(pos, m, er.G, eps), pe) < 1e-10
    assert rel(0.5 * float((m * er.direct_phi(pos, m, er.G, eps)).sum()), pe) < 1e-10
    # the two spellings of phi: potential_ref.direct_phi (what er.phi is up to 2,049 bodies) and the sweep it takes above
    pos, vel, m = er.bodies(2050)
    assert np.array_equal(er.phi(pos[:1501], m[:1501], er.G, eps), er.direct_phi(pos[:1501], m[:1501], er.G, eps))
    assert np.allclose(er.phi(pos, m, er.G, eps), er.direct_phi(pos, m, er.G, eps), rtol=1e-13, atol=0)


# ---- the pieces of a partition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(0, 301, 777, 1013), (0, 1, 255, 256, 257, 1012, 1013), (0, 1013)])
def test_shard_pieces_sum_to_the_whole(cuts):
    pos, vel, m = er.bodies(er.N_PACKED)
    for eps in er.EPS:
        ke = pe = 0.0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            k, p = er.shard(pos[lo:hi], m[lo:hi], vel[lo:hi], lo, pos, m, er.G, eps)
            ke, pe = ke + k, pe + p
        assert rel(ke, er.kinetic(vel, m)) < 1e-14
        assert rel(pe, er.potential(pos, m, er.G, eps)) < 1e-13


def test_shard_self_exclusion_is_by_index_only():
    """a target whose index falls outside [0, n_sources) sees every source, its own copy at r = 0 included"""
    pos, vel, m = er.bodies(er.N_PACKED)
    t = slice(0, 7)
    _, own = er.shard(pos[t], m[t], vel[t], 0, pos, m, er.G, 0.01)
    for off in (-7, er.N_PACKED, 1 << 40, -(1 << 40)):
        _, other = er.shard(pos[t], m[t], vel[t], off, pos, m, er.G, 0.01)
        extra = -0.5 * er.G * float((m[t].astype(np.float64) ** 2).sum()) / math.sqrt(float(F(0.01) * F(0.01)))
        assert rel(other - own, extra) < 1e-9
    _, part = er.shard(pos[t], m[t], vel[t], -3, pos, m, er.G, 0.01)     # targets 3..6 are taken for sources 0..3
    assert part != own and part != other


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
def test_the_shapes_cover_the_four_regimes_of_the_plan():
    assert {er.regime(n) for n in er.ENERGY_SIZES} == {"one split", "one tile per split", "short last split", "exact splits"}
    assert {er.regime(n) for n in er.PHI_SIZES} == {"one split", "one tile per split", "short last split", "exact splits"}
    assert [er.regime(n) for n in (1, 255, 256)] == ["one split"] * 3
    assert [er.plan(n) for n in (257, 511, 512, 513)] == [(2, 2, 2, 1), (2, 2, 2, 1), (2, 2, 2, 1), (3, 3, 3, 1)]
    assert {n % 256 for n in er.ENERGY_SIZES if 255 <= n <= 513} == {255, 0, 1}      # last tile: 255 bodies, full, one body
    assert er.plan(2049) == (9, 9, 9, 1)
    assert er.plan(11520) == (45, 45, 45, 1) and er.regime(11520) == "one tile per split"    # the last such N ...
    assert er.plan(11521) == (46, 46, 23, 2) and er.regime(11521) == "exact splits"          # ... and the first with two
    assert er.plan(11777) == (47, 47, 24, 2) and er.regime(11777) == "short last split" and 11777 % 256 == 1
    assert er.plan(12288) == (48, 48, 24, 2) and er.regime(12288) == "exact splits"
    assert all(0 < n <= 262144 for n in er.ENERGY_SIZES + er.PHI_SIZES + er.REUSE_SIZES)
    assert set(er.PHI_SIZES + er.FLOAT_SIZES + er.REUSE_SIZES) <= set(er.ENERGY_SIZES)      # (one body set per size)
    # the grid-stride kernels: 1024 blocks of 256 lanes reach 262144 bodies in one turn
    assert er.KE_GRID_CAP * er.TILE == 262144 == er.KINETIC_SIZES[0] and er.KINETIC_SIZES[1] == 262145
    assert er.KINETIC_SIZES[2] > 2 * 262144                                                  # a third turn, of one body
    assert er.regime(er.N_PACKED) == "one tile per split" and 768 < er.N_PACKED < 1024       # a short last tile


# ---- the sentinels -----------------------------------------------------------------------------------------------------------------
def test_body_share_is_what_removing_the_body_takes():
    for n in (257, 513):
        pos, vel, m = er.bodies(n)
        for eps in er.EPS:
            whole = er.potential(pos, m, er.G, eps)
            for k in er.sentinels(n):
                keep = np.arange(n) != k
                assert rel(er.body_share(pos, m, er.G, eps, k), whole - er.potential(pos[keep], m[keep], er.G, eps)) < 1e-11


SETS = {f"n={n}": (lambda n=n: er.bodies(n), True) for n in er.ENERGY_SIZES + [er.N_PACKED]}
SETS.update({f"n={n}, KE only": (lambda n=n: er.bodies(n), False) for n in er.KINETIC_SIZES})
SETS["denormal"] = (er.denormal_case, True)


@pytest.mark.parametrize("name", list(SETS))
def test_the_loss_of_one_sentinel_is_100_tolerances(name):
    """every body set of the GPU file: without the body at 0, 255, 256, n - 1 (262143, 262144) the reference KE -- and, where
    the set is used for a PE, the reference PE at both softenings -- differs by at least 100 x 1e-6 of itself"""
    make, with_pe = SETS[name]
    pos, vel, m = make()
    n = len(m)
    named = er.sentinels(n)
    assert named == sorted({k for k in (0, 255, 256, 262143, 262144) if k < n} | {n - 1})
    assert np.all(m[named] == er.sentinel_mass(n)) and np.count_nonzero(m == er.sentinel_mass(n)) == len(named)
    zeros = er.ZERO_MASS_SIZES.get(n, ()) if name != "denormal" else ()
    assert np.flatnonzero(m == 0).tolist() == sorted(zeros) and not set(zeros) & set(named)
    ke = er.kinetic(vel, m)
    worst = min((ke - er.kinetic(np.delete(vel, k, 0), np.delete(m, k))) / ke for k in named)
    msg = f"{name}: the lightest sentinel is {worst:.2e} of KE"
    assert worst >= 100 * er.TOL, msg
    if with_pe and n >= 2:
        for eps in er.EPS if name != "denormal" else (0.0,):
            pe = er.potential(pos, m, er.G, eps)
            worst = min(er.body_share(pos, m, er.G, eps, k) / pe for k in named)
            msg += f", {worst:.2e} of PE (eps {eps})"
            assert worst >= 100 * er.TOL, msg
    print(msg)
    # the sentinels together do not carry the sums (a wrong ORDINARY body still shows)
    assert float(m[named].sum()) < 0.1 * float(m.sum()) or n <= 16 * len(named)
