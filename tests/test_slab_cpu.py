"""tests/slab_ref.py checked without a GPU: its layer owners against the host entry point nbody_hip_slab_layer_owner (plain
host code of csrc/slab.hip, the twin of the device function), its fill against a brute force that shares no code with it,
and its exact fused multiply-add against a case where rounding through a double gives another fp32.  Every comparison is
== on integers or bit patterns."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import slab_ref as ref

F = np.float32
CELLS = [F(1.0), F(0.5), F(0.7), F(1.0) / F(3.0)]
WORLDS = [1, 2, 5, 32, 64]


def host_owner(nb, layer, lo_z, cell, W, cuts):
    buf = (C.c_float * max(len(cuts), 1))(*[float(c) for c in cuts])
    return nb._lib.load().nbody_hip_slab_layer_owner(int(layer), float(lo_z), float(cell), W, buf)


up, down, crafted_cuts = ref.up, ref.down, ref.crafted_cuts


@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("cell", CELLS, ids=lambda c: f"cell{float(c):.3f}")
def test_owner_cuts_against_the_host_entry_point(nb, cell, W):
    rng = np.random.default_rng(1000 * W + int(float(cell) * 100))
    for trial in range(3):
        lo_z = F(rng.uniform(-50.0, 50.0))
        gz = int(rng.integers(1, 120))
        for name, cuts in crafted_cuts(lo_z, cell, gz, W, rng).items():
            want = [ref.owner_cuts(z, lo_z, cell, cuts) for z in range(gz)]
            got = [host_owner(nb, z, lo_z, cell, W, cuts) for z in range(gz)]
            assert got == want, (name, float(lo_z), gz, cuts.tolist())
            assert all(0 <= o < W for o in want) and all(b >= a for a, b in zip(want, want[1:])), name   # monotone
            if name == "all_below":
                assert set(want) == {W - 1}
            if name == "all_above":
                assert set(want) == {0}
            if name == "two_equal":
                assert 1 not in want
    # a cut exactly at a centre sends that layer up, one ulp above it keeps the layer down
    lo_z, z = F(-3.25), 7
    c = ref.layer_centre(z, lo_z, cell)
    assert ref.owner_cuts(z, lo_z, cell, [c]) == 1 and ref.owner_cuts(z, lo_z, cell, [down(c)]) == 1
    assert ref.owner_cuts(z, lo_z, cell, [up(c)]) == 0
    if W == 2:
        assert host_owner(nb, z, lo_z, cell, 2, [c]) == 1 and host_owner(nb, z, lo_z, cell, 2, [up(c)]) == 0


def test_the_host_entry_point_rejects_what_it_cannot_hold(nb):
    cuts = [0.0] * 64
    assert host_owner(nb, 0, 0.0, 1.0, 0, cuts) == -1
    assert host_owner(nb, 0, 0.0, 1.0, 65, cuts) == -1
    assert nb._lib.load().nbody_hip_slab_layer_owner(0, 0.0, 1.0, 2, None) == -1


def test_owner_equal_ranges():
    """every rank's layers are [r gz // W, (r+1) gz // W), also with fewer layers than ranks"""
    for gz in range(1, 201):
        for W in range(1, 65):
            owners = [ref.owner_equal(z, gz, W) for z in range(gz)]
            for r in range(W):
                mine = [z for z in range(gz) if owners[z] == r]
                assert mine == list(range(r * gz // W, (r + 1) * gz // W)), (gz, W, r)
            assert np.array_equal(ref.owner_equal(np.arange(gz), gz, W), owners)


def brute_fill(ids, holes, arrivals):
    """what the header of nbody_hip_slab_fill promises, on lists: -> the ids of the slots [0, n_new)"""
    slots = list(ids)
    for h in holes:
        slots[h] = None
    n_new = len(ids) - len(holes) + len(arrivals)
    slots += [None] * max(0, n_new - len(slots))
    free = list(holes) + list(range(len(ids), n_new))
    for t, a in enumerate(arrivals):
        slots[free[t]] = a
    open_holes = [h for h in free[len(arrivals):] if h < n_new]
    movers = [p for p in range(n_new, len(ids)) if slots[p] is not None]
    assert len(open_holes) == len(movers)
    for h, p in zip(open_holes, movers):
        slots[h], slots[p] = slots[p], None
    return slots[:n_new]


def test_fill_against_a_brute_force():
    cases = 0
    for n_old in range(0, 10):
        ids = list(range(100, 100 + n_old))
        for L in range(0, n_old + 1):
            for holes in itertools.combinations(range(n_old), L):
                for A in range(0, n_old + 3):
                    n_new = n_old - L + A
                    cap = max(n_old, n_new)
                    arr = np.zeros((A, 16), F)
                    arr[:, 12] = (np.arange(A, dtype=np.int32) + 1000).view(F)
                    arr[:, 0], arr[:, 5], arr[:, 9] = np.arange(A) + 0.25, np.arange(A) + 0.5, np.arange(A) + 0.75
                    posm, vel, acc = (np.full((cap, 4), -1.0, F) for _ in range(3))
                    posm[:n_old, 0] = vel[:n_old, 1] = acc[:n_old, 1] = np.arange(n_old)
                    gid = np.full(cap, -7, np.int32)
                    gid[:n_old] = ids
                    assert ref.fill(posm, vel, acc, gid, n_old, np.array(holes, np.int64), arr) == n_new
                    got = gid[:n_new].tolist()
                    stay = [i for k, i in enumerate(ids) if k not in holes]
                    assert sorted(got) == sorted(stay + list(range(1000, 1000 + A)))           # each exactly once
                    assert all(got[k] == ids[k] for k in range(min(n_old, n_new)) if k not in holes)   # stayers rest
                    came = [k for k, g in enumerate(got) if g >= 1000]
                    assert [got[k] for k in came] == list(range(1000, 1000 + A))               # arrivals in order
                    assert got == brute_fill(ids, holes, list(range(1000, 1000 + A)))
                    for k, g in enumerate(got):                                                # the payload follows the id
                        if g >= 1000:
                            assert (posm[k, 0], vel[k, 1], acc[k, 1]) == (g - 1000 + 0.25, g - 1000 + 0.5, g - 1000 + 0.75)
                        else:
                            assert posm[k, 0] == vel[k, 1] == acc[k, 1] == g - 100
                    cases += 1
    assert cases == sum(2 ** n * (n + 3) for n in range(10))


def test_fill_without_ids():
    posm, vel, acc = (np.arange(24, dtype=F).reshape(6, 4) + k for k in (0, 100, 200))
    arr = np.arange(16, dtype=F).reshape(1, 16) + 500
    assert ref.fill(posm, vel, acc, None, 6, np.array([1, 4]), arr) == 5
    assert posm[:5, 0].tolist() == [0, 500, 8, 12, 20] and vel[1].tolist() == [504, 505, 506, 507]
    assert acc[1].tolist() == [508, 509, 510, 511] and acc[4, 0] == 220


def test_fma32_rounds_once():
    """c = 1 + 2^-23 (odd), a b = 2^-24 (1 - 2^-46): the sum lies 2^-70 BELOW the midpoint of c and its successor.  A
    double cannot hold that: it rounds to the midpoint itself, which then goes to the even neighbour, upwards."""
    a, b, c = F(2.0 ** -12) * (F(1) + F(2.0 ** -23)), F(2.0 ** -12) * (F(1) - F(2.0 ** -23)), F(1) + F(2.0 ** -23)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    mid = Fraction(float(c)) + Fraction(1, 2 ** 24)
    assert exact == mid - Fraction(1, 2 ** 70)
    once = ref.fma32(a, b, c)
    via_double = F(float(a) * float(b) + float(c))
    assert once.view(np.uint32) == c.view(np.uint32)
    assert via_double.view(np.uint32) == np.nextafter(c, F(2)).view(np.uint32)
    assert once != via_double
    # and the easy properties: exact products, ties to even, denormals, signed zeros, overflow
    assert ref.fma32(F(3), F(5), F(7)) == F(22)
    assert ref.fma32(F(1), F(1), F(2.0 ** -24)) == F(1)                         # tie -> even (down)
    assert ref.fma32(F(1) + F(2.0 ** -23), F(1), F(2.0 ** -24)) == F(1) + F(2.0 ** -22)   # tie -> even (up)
    assert ref.fma32(F(2.0 ** -100), F(2.0 ** -49), F(0)) == F(2.0 ** -149)
    assert ref.fma32(F(2.0 ** -100), F(2.0 ** -50), F(0)) == F(0)                # half the smallest denormal: tie -> 0
    assert np.signbit(ref.fma32(F(-0.0), F(1), F(-0.0))) and not np.signbit(ref.fma32(F(2), F(3), F(-6)))
    assert ref.fma32(F(3e38), F(2), F(0)) == F(np.inf)
    rng = np.random.default_rng(5)   # where the double IS exact (small integers) both ways agree
    for x, y, z in rng.integers(-2000, 2000, (200, 3)):
        assert ref.fma32(F(x), F(y), F(z)) == F(float(x) * float(y) + float(z))


def test_fma32_array_keeps_the_exact_helper_for_the_elements_that_need_it():
    """the quick path (through a double, the doubtful elements through fma32) against fma32 on every element"""
    rng = np.random.default_rng(6)
    a, b, c = (rng.normal(size=3000) * 10.0 ** rng.integers(-3, 4, 3000)).astype(F), rng.normal(size=3000).astype(F), None
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-4, 5, 3000) * 2.0 ** -24)).astype(F)   # cancellation
    c[::3] = rng.normal(size=1000).astype(F)
    # the case of test_fma32_rounds_once, a tie that is exact (stays a tie), an exact zero, -0, a denormal result, overflow
    odd = F(1) + F(2.0 ** -23)
    extra = [(F(2.0 ** -12) * odd, F(2.0 ** -12) * (F(1) - F(2.0 ** -23)), odd), (F(1), F(2.0 ** -24), odd), (F(2), F(3), F(-6)),
             (F(-0.0), F(1), F(-0.0)), (F(2.0 ** -100), F(2.0 ** -49), F(2.0 ** -140)), (F(3e38), F(2), F(1))]
    a, b, c = (np.concatenate([x, np.array([e[k] for e in extra], F)]) for k, x in enumerate((a, b, c)))
    quick, exact = ref.fma32_array(a, b, c), ref.fma32_array(a, b, c, exact_only=True)
    assert np.array_equal(quick.view(np.uint32), exact.view(np.uint32))
    assert quick[-6].view(np.uint32) == odd.view(np.uint32) and np.signbit(quick[-3]) and quick[-1] == F(np.inf)


def test_geometry_and_layer():
    lo, dims = ref.geometry([0.0, 0.0, 0.0, 9.0, 0.5, 2.999], 1.0)
    assert [v.view(np.uint32) for v in lo] == [(F(0) - F(0.001)).view(np.uint32)] * 3
    assert dims == [11, 2, 5]   # ceil(9.002) + 1, ceil(0.502) + 1, ceil(3.001) + 1
    assert ref.geometry([0, 0, 0, 3e38, 0, np.inf], 1e-3)[1] == [ref.GRID_TOO_LARGE, 3, ref.GRID_TOO_LARGE]
    z = np.array([-1e30, -0.001, 0.0, 0.998, 0.999, 1.0, 3.5, 1e30], F)
    assert ref.layer(z, lo[2], 1.0, 5).tolist() == [0, 0, 0, 0, 1, 1, 3, 4]
    assert ref.layer(z, lo[2], 1.0, 1).tolist() == [0] * 8


def test_partition_small():
    """a partition small enough to write down: 6 bodies, W = 3, rank 1, layers 0..5 (two per rank)"""
    posm = np.zeros((6, 4), F)
    posm[:, 2] = [2.5, 0.5, 5.5, 3.5, 4.5, 1.5]
    posm[:, 3] = np.arange(6) + 1
    vel, acc = posm + 10, posm + 20
    gid = np.arange(6, dtype=np.int32) * 11
    r = ref.partition(posm, vel, acc, gid, [0, 0, 0.002, 0, 0, 5.5], 1.0, 3, 1, 4)
    assert r["info"].tolist() == [2, 2, 7, 1] and r["layer"].tolist() == [2, 0, 5, 3, 4, 1]
    assert r["dest"].tolist() == [1, 0, 2, 1, 2, 0]          # 7 layers over 3 ranks: [0, 2) [2, 4) [4, 7)
    assert r["holes"].tolist() == [1, 2, 4, 5] and r["send"].tolist() == [2, 2, 2]
    assert r["rows"][:, 12].view(np.int32).tolist() == [11, 55, 22, 44]
    assert r["rows"][:, 13].view(np.int32).tolist() == [0, 1, 5, 4]
    assert r["rows"][:, 3].tolist() == [2, 6, 3, 5] and np.all(r["rows"][:, [7, 11, 14, 15]] == 0)
    assert r["rows"][:, 4:7].tolist() == (posm[[1, 5, 2, 4], :3] + 10).tolist()
    assert r["rows"][:, 8:11].tolist() == (posm[[1, 5, 2, 4], :3] + 20).tolist()
    assert r["hist"].tolist() == [1, 1, 1, 1]                # the first hist_cap = 4 layers although gz = 7 > hist_cap
