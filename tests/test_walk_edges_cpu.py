"""tests/walk_edge_ref.py without a GPU: the exact fma, the case search on a node table made from tree_ref.RefTree (centre
of mass rounded to fp32), the reference's own statement of every case, the restatement's old outputs, and the wave
count on a hand-made tree."""
import os
from fractions import Fraction

import numpy as np
import pytest

import quadrupole_ref as qr
import tree_ref
import walk_edge_ref as we
from potential_ref import fp32_dist2

F = we.F
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# a b + c whose exact value misses a tie of fp32 by less than half a step of fp64: (A, B, C, s) for a = A, b = B,
# c = C 2^s with A B = 2^(s - 1) +- 1 (mod 2^s); rounding through a double gives the wrong neighbour on each of them
PLANTED = [(8389359, 15559695, 8388613, 31), (8389021, 16675659, 8388613, 31), (8389489, 14787183, 8388613, 31),
           (8390519, 13173319, 8388613, 33), (8457509, 13256365, 8388613, 36)]


def test_round32_is_one_rounding():
    assert we.round32(Fraction(1) + Fraction(1, 2 ** 24)) == F(1.0)                       # tie: to even
    assert we.round32(Fraction(1) + Fraction(3, 2 ** 24)) == F(1.0) + F(2.0 ** -22)       # tie: to even, upwards
    assert we.round32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 90)) == F(1.0) + F(2.0 ** -23)
    assert we.round32(Fraction(1) + Fraction(1, 2 ** 24) - Fraction(1, 2 ** 90)) == F(1.0)
    assert we.round32(-Fraction(3, 2 ** 150)) == F(-2.0 ** -148)                            # subnormal tie: to even
    rng = np.random.default_rng(3)
    for v in rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200):
        assert we.round32(Fraction(float(v))) == F(v)
    assert we.size2_of(F(0.3)) == F(F(2) * F(0.3)) * F(F(2) * F(0.3))


def test_fma32_against_fractions_on_planted_double_roundings():
    through_double = 0
    for A, B, C, s in PLANTED:
        for sa in (1.0, -1.0):
            for scale in (1.0, 2.0 ** -40):
                a, b, c = F(sa * A * scale), F(B * scale), F(sa * C * 2.0 ** s * scale * scale)
                exact = we.fma_exact(a, b, c)
                assert Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)) != Fraction(float(exact))
                assert we.fma32(a, b, c) == exact, (A, B, C, s)
                through_double += F(float(a) * float(b) + float(c)) != exact
    assert through_double == 4 * len(PLANTED)   # the inputs are what they claim: two roundings go wrong on every one
    # as arrays, among ordinary values, and on random inputs of mixed magnitude
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(4000) * 2.0 ** rng.integers(-8, 8, 4000)).astype(F)
    b = (rng.standard_normal(4000) * 2.0 ** rng.integers(-8, 8, 4000)).astype(F)
    c = (rng.standard_normal(4000) * 2.0 ** rng.integers(-12, 12, 4000)).astype(F)
    for k, (A, B, C, s) in enumerate(PLANTED):
        a[7 * k], b[7 * k], c[7 * k] = A, B, C * 2.0 ** s
    got = we.fma32(a, b, c)
    want = np.array([we.fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert np.array_equal(got, want)
    # the distance chain: vectorised against the Fraction routine, body against node centre
    p = (rng.integers(-700, 700, (300, 3)) / 64.0).astype(F)
    com = (rng.standard_normal((300, 3)) * 4).astype(F)
    d = (com - p).astype(F)
    vec = we.dist2_fma32(d[:, 0], d[:, 1], d[:, 2])
    for k in range(300):
        d2, dist2 = we.dist2_exact(com[k], p[k], 0.05)
        assert d2 == vec[k] and dist2 == F(vec[k] + F(F(0.05) * F(0.05)))


def test_theta_edge_is_the_neighbouring_pair():
    rng = np.random.default_rng(9)
    for _ in range(40):
        size2, dist2 = F(rng.uniform(0.01, 4.0)), F(rng.uniform(0.5, 60.0))
        edge = we.theta_edge(size2, dist2)
        if float(size2) / float(dist2) > 4.0:
            assert edge is None
            continue
        lo, hi = edge
        assert hi == we.next32(lo) and 0 < lo and hi <= 2
        assert not size2 < we.threshold(lo, dist2) and size2 < we.threshold(hi, dist2)
        assert abs(float(lo) ** 2 * float(dist2) / float(size2) - 1) < 1e-6
    assert we.theta_edge(F(100.0), F(1.0)) is None      # still opened at theta = 2
    assert we.theta_edge(F(4.0), F(1.0)) is None        # size2 == theta2 dist2 at theta = 2: opened there, no edge inside
    lo, hi = we.theta_edge(F(4.0), we.next32(F(1.0)))
    assert hi <= F(2.0) and hi == we.next32(lo)


@pytest.fixture(scope="module")
def world(oracle):
    ic = we.population()
    out = {"ic": ic, "n": len(ic["mass"])}
    for name, params in (("deep", (20, 1)), ("wide", (20, 4))):
        ref = tree_ref.RefTree(oracle, ic, *params)
        out[name] = we.EdgeRestatement(we.node_table(ref), ref.order, we.positions(ic), ic["mass"])
    out["deep_cases"] = {eps: we.theta_cases(out["deep"], eps) for eps in (0.0, 0.05)}
    out["wide_cases"] = {eps: we.theta_cases(out["wide"], eps, prefer_many=True) for eps in (0.0, 0.05)}
    return out


def test_population_and_search_meet_the_conditions(world):
    n = world["n"]
    assert 560 <= n <= 600
    pos = we.positions(world["ic"])
    assert len(np.unique(pos, axis=0)) == n
    assert set(np.log2(world["ic"]["mass"]).tolist()) == {-3.0, -2.0, -1.0, 0.0}
    r = world["deep"]
    internal = np.flatnonzero(~r.leaf & (r.parent >= 0))
    have = {(int(r.nchild[r.parent[k]]), int(r.sibrank[k])) for k in internal}
    assert have == set(we.COMBOS)              # the committed seed: all 36 (children, rank) with an internal child
    cases, share = we.check_theta_cases(world["deep_cases"], world["wide_cases"])
    per_combo = {c: sum(k.combo == c for k in cases) for c in we.COMBOS}
    print(f"{len(cases)} cases, {share:.3f} exact equalities, per combination {min(per_combo.values())}.."
          f"{max(per_combo.values())}, smallest margin {min(c.margin for c in cases):.2e}")
    assert min(per_combo.values()) >= 2
    for c in cases:
        assert c.count <= n // 2               # a unit of the split walk at two replicas holds it


def test_every_case_flips_alone_in_the_reference(world):
    for name in ("deep", "wide"):
        r = world[name]
        for eps, found in world[name + "_cases"].items():
            for c in found.values():
                a = r.walk_detail([c.target], c.theta_open, 1.0, eps, 1)
                b = r.walk_detail([c.target], c.theta_accept, 1.0, eps, 1)
                da, db = r.decisions_of(a, 0), r.decisions_of(b, 0)
                assert da[c.node] is False and db[c.node] is True, c
                assert [k for k in db if da[k] != db[k]] == [c.node], c
                gone = set(da) - set(db)       # tests only the opening walk takes: the node's subtree, nothing else
                assert all(r.first[c.node] <= r.first[k] < r.last[k] <= r.last[c.node] for k in gone), c
                assert not set(db) - set(da)
                assert b.tested[0] == a.tested[0] - len(gone)
                assert b.accepted[0] == a.accepted[0] + 1 - sum(da[k] for k in gone)
                # the decision from the record alone, through Fractions
                com, half = r.com32[c.node], r.nodes["half_size"][c.node]
                assert we.decide(com, half, r.pos32[c.target], c.theta_open, eps) is False
                assert we.decide(com, half, r.pos32[c.target], c.theta_accept, eps) is True
                if c.equality:
                    assert we.threshold(c.theta_open, we.dist2_exact(com, r.pos32[c.target], eps)[1]) == we.size2_of(half)
                # the flip is worth 100 x the tolerance of the comparisons, on their scale
                ma = np.linalg.norm(a.acc[0] - b.acc[0]) / max(a.scale_acc[0], b.scale_acc[0])
                mp = abs(a.phi[0] - b.phi[0]) / max(a.scale_phi[0], b.scale_phi[0])
                assert min(ma, mp) >= we.MARGIN, (c, ma, mp)


def test_point_cases(world):
    r = world["deep"]
    for theta in (1.0, 0.5):
        found = we.point_cases(r, theta)
        assert len(found) >= 8
        for c in found:
            we.check_point_case(r.nodes, c)
            assert c.decisions[0] is False     # on the edge: opened
            step = c.points[2, c.axis] - c.points[1, c.axis]
            assert step > 0 and np.array_equal(np.delete(c.points[1], c.axis), np.delete(c.points[0], c.axis))
        # a neighbour on the far side is accepted somewhere: the three points do not all decide alike
        assert any(True in c.decisions for c in found)


def test_restatement_reproduces_its_recorded_outputs(oracle):
    """golden/restatement_twogalaxies2048.npz: quadrupole_ref.Restatement as it stood before walk() learned `detail`, on
    the node table of tree_ref.RefTree over golden/twogalaxies2048_barnes_hut.npz (every 16th body, theta 0.5)"""
    z = np.load(os.path.join(GOLDEN, "twogalaxies2048_barnes_hut.npz"))
    want = np.load(os.path.join(GOLDEN, "restatement_twogalaxies2048.npz"))
    ic = {k: z[k] for k in ("pos_x", "pos_y", "pos_z", "mass")}
    ref = tree_ref.RefTree(oracle, ic, 20, 1)
    table = we.node_table(ref)
    targets = want["targets"]
    for cls in (qr.Restatement, we.EdgeRestatement):
        r = cls(table, ref.order, we.positions(ic), ic["mass"])
        for eps in (0.0, 0.05):
            for order in (1, 2):
                a, p = r.walk(targets, 0.5, 1.0, eps, order)
                assert np.array_equal(a, want[f"acc_o{order}_eps{eps}"]), (cls.__name__, eps, order)
                assert np.array_equal(p, want[f"phi_o{order}_eps{eps}"]), (cls.__name__, eps, order)
            assert np.array_equal(r.interaction_counts(targets, 0.5, eps), want[f"counts_eps{eps}"])
            if cls is we.EdgeRestatement:
                d = r.walk_detail(targets, 0.5, 1.0, eps, 1)
                assert np.array_equal(np.stack([d.accepted, d.leaf_bodies], 1), want[f"counts_eps{eps}"])
                assert np.array_equal(d.acc, want[f"acc_o1_eps{eps}"])
                assert np.all(d.tested > d.accepted) and np.all(d.scale_acc >= np.linalg.norm(d.acc, axis=1))


def _hand_tree():
    """root (130 bodies) -> leaf of 64 bodies near x = -10 | node B of 66 bodies near x = +10 -> leaf of 65 | leaf of 1"""
    rng = np.random.default_rng(1)
    left = np.array([-10.0, 0, 0]) + rng.uniform(-0.5, 0.5, (64, 3))
    right = np.array([10.0, 0, 0]) + rng.uniform(-0.5, 0.5, (66, 3))
    pos = np.concatenate([left, right]).astype(F)
    m = np.ones(130, F)
    t = np.zeros(5, we.NODE_DTYPE)
    t["children"] = -1
    t["children"][0, [1, 6]] = (1, 2)
    t["children"][2, [0, 7]] = (3, 4)
    t["particle_count"] = (130, 64, 66, 65, 1)
    t["is_leaf"] = (False, True, False, True, True)
    t["half_size"] = (16.0, 1.0, 1.0, 0.5, 0.5)
    for k, (a, b) in enumerate(((0, 130), (0, 64), (64, 130), (64, 129), (129, 130))):
        t["center_of_mass"][k] = pos[a:b].astype(np.float64).mean(0)
        t["total_mass"][k] = b - a
    return we.EdgeRestatement(t, np.arange(130), pos, m)


def test_wave_visits_on_a_hand_made_tree():
    r = _hand_tree()
    everyone = np.arange(130)
    # theta = 0: every wave (0..63, 64..127, 128..129) pops the root (1), its group (2) and B's group (2)
    d = r.walk_detail(everyone, 0.0, 1.0, 0.05, 1, first=0)
    assert d.visited == 3 * 5
    assert np.array_equal(d.tested, np.full(130, 2)) and d.accepted.sum() == 0 and np.all(d.leaf_bodies == 129)
    # theta = 0.5: B (size 2) is accepted from the left (distance 20) and opened from inside; the root is opened
    d = r.walk_detail(everyone, 0.5, 1.0, 0.05, 1, first=0)
    assert d.visited == (1 + 2) + 2 * 5
    assert np.array_equal(d.accepted, np.r_[np.ones(64, int), np.zeros(66, int)])
    assert np.array_equal(d.leaf_bodies, np.r_[np.full(64, 63), np.full(66, 129)])
    # a range that starts at 32: its first wave holds bodies of both sides, its second only the right
    d = r.walk_detail(np.arange(32, 130), 0.5, 1.0, 0.05, 1, first=32)
    assert d.visited == 5 + 5
    d = r.walk_detail(np.arange(0, 64), 0.5, 1.0, 0.05, 1, first=0)
    assert d.visited == 3
    d = r.walk_detail([5], 0.5, 1.0, 0.05, 1, first=5)
    assert d.visited == 3 and d.tested[0] == 2 and d.accepted[0] == 1
    # theta = 2 from far away accepts even the root's neighbour... and a body may accept a node that holds it
    d = r.walk_detail(everyone, 2.0, 1.0, 0.05, 1, first=0)
    assert d.accepted[:64].min() >= 1
