"""The integer-lattice reference of the Direct kernels (direct_lattice_ref.py) kept honest, without a GPU: the O(N)
formula against a brute-force double loop, an fp32 emulation of the pair arithmetic that must reproduce it bit for bit
in any summation order, the sensitivity of u to one pair, and the 2^24 bound for every case of the GPU file."""
import numpy as np
import pytest

import direct_lattice_ref as L


def _brute_all_pairs(lat):
    u = np.zeros((lat.n, 3), np.int64)
    for i in range(lat.n):
        for j in range(lat.n):
            if j != i:
                u[i] += lat.m[j] * (lat.p[j] - lat.p[i])
    return u


def test_lattice_generator():
    s = L.all_sites()
    assert s.shape == (L.NSITES, 3) and len({tuple(r) for r in s.tolist()}) == L.NSITES
    assert s.min(0).tolist() == [-16, -16, -10] and s.max(0).tolist() == [15, 15, 9]
    assert int(((s.max(0) - s.min(0)) ** 2).sum()) == L.D2_MAX < 2 ** 16
    for assignment in L.ASSIGNMENTS:
        lat = L.lattice(L.NSITES, assignment, "g0123")
        assert len({tuple(r) for r in lat.p.tolist()}) == L.NSITES
        assert lat.packed.dtype == np.float32 and lat.packed.shape == (L.NSITES, 4)
        assert np.array_equal(lat.packed[:, :3].astype(np.int64), lat.p) and np.array_equal(lat.packed[:, 3].astype(np.int64), lat.m)
    assert np.array_equal(L.lattice(300, "index").p, s[:300])
    a, b = L.lattice(5000, "permuted"), L.lattice(700, "permuted")
    assert np.array_equal(a.p[:700], b.p) and not np.array_equal(a.p, s[:5000])   # one fixed permutation, prefixes nest
    nz = L.lattice(3073, "permuted", "g123", nonzero=True)
    assert np.all(nz.p != 0) and len({tuple(r) for r in nz.p.tolist()}) == 3073
    # the mass patterns: what the device's min / max test will see
    for n in (2, 97, 2049, L.NSITES):
        assert set(L.mass_pattern(n, "ones").tolist()) == {1} and set(L.mass_pattern(n, "threes").tolist()) == {3}
        for pat in L.GENERAL_MASSES:
            m = L.mass_pattern(n, pat)
            assert m.min() != m.max() and set(m.tolist()) <= {0, 1, 2, 3}
        # the zero-mass pattern: at most 1/97 of the sources are invisible; the {1, 2, 3} pattern has none
        assert int((L.mass_pattern(n, "g0123") == 0).sum()) == n // 97 <= n / 97
        assert int((L.mass_pattern(n, "g123") == 0).sum()) == 0
    for shape in L.rect_shapes(2):
        a, b = L.rect_sets(2, shape, "permuted", "a_differs")
        assert set(a.m.tolist()) == {2} and set(b.m.tolist()) == {1} and (a.n, b.n) == shape
        assert not {tuple(r) for r in a.p.tolist()} & {tuple(r) for r in b.p.tolist()}
        a, b = L.rect_sets(2, shape, "index", "equal3")
        assert set(a.m.tolist()) == {3} == set(b.m.tolist())


@pytest.mark.parametrize("assignment", L.ASSIGNMENTS)
@pytest.mark.parametrize("masses", ["threes", "g0123"])
def test_formula_against_brute_force(assignment, masses):
    n = 300
    lat = L.lattice(n, assignment, masses)
    assert np.array_equal(L.expect_all_pairs(lat), _brute_all_pairs(lat))
    # two disjoint sets: a set's bodies against the other's == all pairs minus the set's own pairs
    a, b = lat.cut(0, 113), lat.cut(113, n)
    ua, ub = L.expect_two_sets(a, b)
    whole = _brute_all_pairs(lat)
    assert np.array_equal(ua, whole[:113] - _brute_all_pairs(a))
    assert np.array_equal(ub, whole[113:] - _brute_all_pairs(b))
    # arbitrary points, a third of them on a body, the rest on the half-integer lattice
    pts2 = L.field_points2(300, lat)
    assert np.any(pts2 % 2 != 0)
    on = {tuple(r) for r in (2 * lat.p).tolist()}
    assert sum(tuple(r) in on for r in pts2.tolist()) >= 100
    u2, msum = L.expect_points(pts2, lat)
    b2, bm = L.brute_points(pts2, lat)
    assert np.array_equal(u2, b2) and msum == bm == int(lat.m.sum())
    # the bodies themselves as points: the all-pairs result
    u2, _ = L.expect_points(2 * lat.p, lat)
    assert np.array_equal(u2, 2 * whole)


def test_r2_is_exactly_eps2_for_every_pair():
    """every difference vector two lattice sites (or a site and a half-integer point of the box) can have: a superset of
    the pairs of every n and every assignment"""
    h = np.arange(-63, 64, dtype=np.float32) / 2
    hz = np.arange(-39, 40, dtype=np.float32) / 2
    d = np.stack(np.meshgrid(h, h, hz, indexing="ij"), -1).reshape(-1, 3)
    r2 = L.pair_r2(d)
    assert r2.dtype == np.float32 and np.all(r2 == np.float32(L.EPS2))
    inv = np.float32(1.0) / np.sqrt(r2)
    assert np.all(inv == np.float32(2.0 ** -20)) and np.all((inv * inv) * inv == np.float32(L.UNIT))
    # and the emulation does round: a term above half an ulp of 2^40 shows (2^16 itself is a tie, to even)
    far = L.pair_r2(np.array([[256.0, 0.0, 0.0], [257.0, 0.0, 0.0]], np.float32))
    assert far[0] == np.float32(L.EPS2) and far[1] == np.float32(L.EPS2 + 2.0 ** 17)


@pytest.mark.parametrize("assignment", L.ASSIGNMENTS)
@pytest.mark.parametrize("n", [2049, L.NSITES])
def test_fp32_running_sum_reproduces_the_formula(n, assignment):
    """one fp32 accumulator over ALL sources of a body in a random order -- worse than any kernel's order -- gives the
    int64 formula bit for bit; the pairs' r2 on the way.  All bodies at n = 2,049; at n = 20,480 the first and the last
    256 and 512 at random (every difference vector there can be is in test_r2_is_exactly_eps2_for_every_pair, and
    test_bounds_of_every_gpu_case bounds the sum of the magnitudes of every body: no order of any body can round)"""
    lat = L.lattice(n, assignment, "g0123")
    ref = L.expect_all_pairs(lat)
    rng = np.random.default_rng(n)
    bodies = np.arange(n) if n <= 2049 else np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n),
                                                                      rng.choice(n, 512, replace=False)]))
    p32 = lat.p.astype(np.float32)
    for i in bodies:
        assert np.all(L.pair_r2(p32 - p32[i]) == np.float32(L.EPS2))
        got = L.running_sum32(L.pair_terms(lat, i), rng.permutation(n))
        assert np.array_equal(got.astype(np.float64) / L.UNIT, ref[i]), i
    assert np.array_equal(L.units(L.acc_rows(ref)), ref)


@pytest.mark.parametrize("masses", ["ones", "g123", "g0123"])
def test_sensitivity_and_decode(masses):
    """One pair (i, j) removed, doubled or credited to body i + 1, through the fp32 emulation: u changes by at least one
    whole unit, and decode names the pair."""
    n = L.NSITES
    lat = L.lattice(n, "permuted", masses)
    ref = L.expect_all_pairs(lat)
    rng = np.random.default_rng(7)
    visible = np.nonzero(lat.m > 0)[0]
    assert n - visible.size == (n // 97 if masses == "g0123" else 0)
    for _ in range(200):
        i = int(rng.integers(0, n - 1))
        j = int(rng.choice(visible))
        if j == i:
            continue
        order = rng.permutation(n)
        t = L.pair_terms(lat, i)
        R = int(rng.choice(L.SYM_R))
        for name, factor in (("removed", 0.0), ("doubled", 2.0)):
            tt = t.copy()
            tt[j] *= np.float32(factor)
            u = L.running_sum32(tt, order).astype(np.float64) / L.UNIT
            delta = u - ref[i]
            assert np.abs(delta).max() >= 1 and np.array_equal(delta, np.rint(delta)), (name, i, j)
            assert np.array_equal(delta, (factor - 1) * lat.m[j] * (lat.p[j] - lat.p[i]))
            c = lat.decode(i, delta, R)
            assert c and (i, j) in [(x["i"], x["j"]) for x in c], (name, i, j, c)
            if masses == "ones":     # equal masses: the partner, or its mirror image in p_i with the other sign
                k1 = [x for x in c if x["k"] == 1]
                assert 1 <= len(k1) <= 2 and {x["sign"] for x in k1} <= {1, -1} and len({x["sign"] for x in k1}) == len(k1)
                assert all(np.array_equal(x["sign"] * (lat.p[x["j"]] - lat.p[i]), k1[0]["sign"] * (lat.p[k1[0]["j"]] - lat.p[i])) for x in k1)
            me = [x for x in c if x["j"] == j][0]
            assert (me["superblock"], me["chunk"], me["lane"]) == L.where(j, R) and me["sign"] == (1 if factor else -1)
        # credited to the neighbouring body: i loses the pair, i + 1 gains (p_j - p_i) m_j on top of its own sum
        t1 = np.concatenate([L.pair_terms(lat, i + 1), t[j][None]])
        u1 = L.running_sum32(t1, rng.permutation(n + 1)).astype(np.float64) / L.UNIT
        d1 = u1 - ref[i + 1]
        assert np.abs(d1).max() >= 1 and np.array_equal(d1, lat.m[j] * (lat.p[j] - lat.p[i]))
    # the message of a failing comparison names body and partner
    u = ref.astype(np.float64)
    i, j = 4097, 12345
    u[i] -= lat.m[j] * (lat.p[j] - lat.p[i])
    u[9] = 0.5
    text = L.describe(lat, u, ref, 16)
    assert "2 of 20480 bodies differ" in text and f"partner {j} (superblock 3, chunk 0, lane 57, ring offset d = 2)" in text
    assert "body 9 (superblock 0, chunk 0, lane 9)" in text and "no integer vector" in text


def _gpu_cases():
    for n in L.ONE_SIDED_SIZES:
        for masses in ("threes", "g0123"):
            yield n, masses, False
    for R in L.SYM_R:
        for n in L.sym_sizes(R):
            for masses in L.MASSES:
                yield n, masses, False
    yield 3073, "g123", True     # the SoA and fused paths: sites without a zero coordinate, three kicks (3 u < 2^24)
    for _, n in L.LONG_RINGS:
        for masses in ("ones", "g0123"):
            yield n, masses, False


def test_bounds_of_every_gpu_case():
    """max |u| < 2^24 (and every partial sum with it: |partial| <= sum_j m_j |p_j - p_i|_inf-wise, bounded the same
    way) for every (n, masses, assignment) the GPU file runs: its exactness claim, checked wherever the suite runs"""
    seen = set()
    for n, masses, nonzero in _gpu_cases():
        if (n, masses, nonzero) in seen:
            continue
        seen.add((n, masses, nonzero))
        assert n <= L.NSITES
        for assignment in L.ASSIGNMENTS:
            lat = L.lattice(n, assignment, masses, nonzero=nonzero)
            assert (3 if nonzero else 1) * np.abs(L.expect_all_pairs(lat)).max() < 2 ** 24
            # no partial sum of any order can exceed the sum of the magnitudes
            assert (lat.m[:, None] * np.abs(lat.p)).sum(0).max() + lat.m.sum() * np.abs(lat.p).max() < 2 ** 24
    assert max(n for n, m, _ in seen if m in ("threes", "g123")) == 16577 and max(n for n, _, _ in seen) == L.NSITES
    for R in L.RECT_R:
        for shape in L.rect_shapes(R):
            assert sum(shape) <= L.NSITES
            for assignment in L.ASSIGNMENTS:
                for masses in L.RECT_MASSES:
                    a, b = L.rect_sets(R, shape, assignment, masses)
                    for u in L.expect_two_sets(a, b):
                        assert np.abs(u).max() + 2000 < 2 ** 24    # (+ the integer prefill of the accumulate forms)
    for ns in L.FIELD_SOURCES:
        for assignment in L.ASSIGNMENTS:
            src = L.lattice(ns, assignment, "g0123")
            for count in L.FIELD_POINTS:
                u2, msum = L.expect_points(L.field_points2(count, src), src)
                assert np.abs(u2).max() < 2 ** 24 and msum < 2 ** 24
    # targets that are not the sources: 333 points and the sub-range against 2,049 bodies, + the integer prefill
    for assignment in L.ASSIGNMENTS:
        src = L.lattice(2049, assignment, "g0123")
        u2, _ = L.expect_points(2 * L.lattice(L.NSITES, assignment).p, src)
        assert np.abs(u2).max() // 2 + 1000 < 2 ** 24
    # the coarse bound of the argument: 3 (mass) x 20,480 (bodies) x 31 (largest coordinate difference)
    assert 3 * L.NSITES * 31 < 2 ** 24
