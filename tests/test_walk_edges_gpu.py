"""The opening decision of every Barnes-Hut walk on a real GPU, node by node at its edges (tests/walk_edge_ref.py).

For every theta-edge case -- an internal node, a target outside it, and the two neighbouring fp32 thetas between which
that one decision changes -- every form of the walk runs over ALL bodies at both thetas and is compared with the
restatement whose decisions are exact: values on the scale |a_ref|, or sum |terms| / 16 where the terms cancel (a
case's flip is worth at least 1e-3 of its target on that scale; the bounds: FORCE_TOL below), the visit histogram and
nodes_visited exactly.  Range walks, theta 0 and 2, and points on the exact edge of the field walk follow.

Trees: per shape (max_depth, leaf_max) three builds over the same bodies: plain ids at order 1, even-aligned ids
(walkForm(2) before the build) at order 1, and order 2.  Shapes: deep (20, 1); wide (20, 4), whose edge nodes sit beside
leaves of several bodies (only leaf_max > 1 puts such a leaf beside an INTERNAL sibling: in a depth-limited tree
(4, 1) they sit at the deepest level, among leaves; that tree, `cut`, joins the whole walks at theta 0 and 2).
nodes_visited exists only with counting on, which turns the plain walk into its Count instantiation: it is compared
for Count (orders 1 and 2) and Pair.

One case, stated once: with the node opened, its internal descendants may be accepted in its place, so the accepted
count of the target changes by 1 - (accepted descendants), not always by one; the one-body walks are held to the
reference's tested and accepted counts at both thetas and to that decomposition (test_walk_edges_cpu.py proves it of
the reference).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import walk_edge_ref as we
from gpu_util import acc_of, to_device

pytestmark = pytest.mark.gpu
TOL = 1e-5      # the suite's restatement tolerance (test_bh_quadrupole_gpu.TOL)
# Forces against the restatement as it stands (every accepted node evaluated at the fp64 centre of ITS BODIES) do not meet
# TOL on this population: the clumps sit at |c| ~ 10 and are seen from |d| ~ 0.05, so the fp32 rounding of a record's
# centre alone costs a term 2^-24 |c| / |d| ~ 1e-5.  Measured on MI355X, worst over every case, theta 0 and theta 2:
#   plain 3.931e-05 (order 2: 5.627e-05), count / split 2 / split 16 / field the same figures, pair 3.939e-05,
#   range walks 1.777e-05; phi: potential and field 4.011e-06 (order 2: 7.070e-06).
# The restatement evaluated at the record's centre instead (walk_edge_ref.record_centred) predicts 3.934e-05 and
# 5.614e-05 of that, body for body.  So two bounds: against the restatement as it stands, 4 x the worst value of the
# Plain form (phi stays at TOL); against the record-centred restatement, TOL.
FORCE_TOL = 4 * 3.931e-05
G = 1.0
SHAPES = {"deep": (20, 1), "wide": (20, 4), "cut": (4, 1)}
SHARED = 1024   # units per replica that leave every internal node in the shared zone (unit_max = 1)


class World:
    pass


def _hist(t):
    from nbody_amd._lib import check
    out = (C.c_ulonglong * 130)()
    check(t.ctx._lib.nbody_hip_tree_visit_histogram(t._h, C.byref(out)))
    h = np.array(list(out), np.int64)
    k = np.arange(65)
    return int((k * h[:65]).sum()), int((k * h[65:]).sum())


def _build(nb, d, params, order, aligned):
    t = nb.BarnesHutTree(d.count)
    t.setParams(*params)
    t.setMultipoleOrder(order)
    t.walkForm(2 if aligned else 0)   # before the build: the even-aligned ids exist only on request at this size
    t.build(d)
    t.tuning(1, 0)
    return t


@pytest.fixture(scope="module")
def world(nb, ctx):
    w = World()
    w.nb, w.ctx = nb, ctx
    w.ic = we.population()
    w.n = len(w.ic["mass"])
    w.pos = we.positions(w.ic)
    w.d, _ = to_device(nb, w.ic)
    w.points = torch.from_numpy(np.ascontiguousarray(w.pos)).cuda()
    w.trees, w.r, w.refs = {}, {}, {}
    for shape, params in SHAPES.items():
        tr = {"plain": _build(nb, w.d, params, 1, False), "aligned": _build(nb, w.d, params, 1, True),
              "quad": _build(nb, w.d, params, 2, False)}
        assert tr["aligned"].idLayout()[0] and not tr["plain"].idLayout()[0]
        nodes = tr["plain"].copyNodesToHost().copy()
        order = tr["plain"].sorted_indices_.copy()
        for other in ("aligned", "quad"):   # one export serves the three builds: the same records, bit for bit
            o = tr[other].copyNodesToHost()
            for f in ("center_of_mass", "half_size", "children", "is_leaf", "particle_count", "total_mass"):
                assert np.array_equal(o[f], nodes[f]), (shape, other, f)
            assert np.array_equal(tr[other].sorted_indices_, order)
        w.trees[shape] = tr
        w.r[shape] = we.EdgeRestatement(nodes, order, w.pos, w.ic["mass"])
    w.cases = {"deep": {eps: we.theta_cases(w.r["deep"], eps) for eps in (0.0, 0.05)},
               "wide": {eps: we.theta_cases(w.r["wide"], eps, prefer_many=True) for eps in (0.0, 0.05)}}
    return w


def _ref(w, shape, theta, eps, order):
    """the reference over all bodies, computed once per (tree, theta, eps, order) and left alone"""
    key = (shape, float(theta), float(eps), order)
    if key not in w.refs:
        w.refs[key] = _detail(w.r[shape], np.arange(w.n), theta, eps, order, 0)
    return w.refs[key]


def _detail(r, targets, theta, eps, order, first):
    """walk_detail, and as .rec the same walk evaluated at the records' centres (see FORCE_TOL)"""
    ref = r.walk_detail(targets, theta, G, eps, order, first=first)
    ref.rec = r.record_centred().walk_detail(targets, theta, G, eps, order)
    assert np.array_equal(ref.rec.tested, ref.tested) and np.array_equal(ref.rec.accepted, ref.accepted)
    return ref


def _self_term(w, shape, eps, ref):
    """what the field walk adds to phi at a body's own position: -G m / sqrt(eps2) where the walk reaches the body's own
    leaf; nothing under the eps ~ 0 guard, and nothing for a body that accepts a node which holds it"""
    eps2 = np.float32(np.float32(eps) * np.float32(eps))
    if float(eps2) < 1e-12:
        return np.zeros(w.n)
    r = w.r[shape]
    slot, node, far = ref.pairs
    inside = far & (r.first[node] <= r.rank[slot]) & (r.rank[slot] < r.last[node])
    reached = np.bincount(slot[inside], minlength=w.n) == 0
    return np.where(reached, G * w.ic["mass"].astype(np.float64) / np.sqrt(float(eps2)), 0.0)


class Worst:
    """largest error per form; check() asserts every body of a form against a reference"""

    def __init__(self, tag):
        self.tag, self.worst = tag, {}

    def check(self, form, ref, acc=None, phi=None, extra_phi=None):
        for name, against, force_tol in ((form, ref, FORCE_TOL), (form + " (record centres)", ref.rec, TOL)):
            ea = ep = np.zeros(1)
            if acc is not None:
                assert np.isfinite(acc).all(), (self.tag, name)
                ea = np.linalg.norm(np.asarray(acc, np.float64) - against.acc, axis=1) / against.scale_acc
            if phi is not None:
                assert np.isfinite(phi).all(), (self.tag, name)
                shift = 0.0 if extra_phi is None else extra_phi
                ep = np.abs(np.asarray(phi, np.float64) - (against.phi - shift)) / (against.scale_phi + shift)
            a, p = self.worst.get(name, (0.0, 0.0))
            self.worst[name] = (max(a, float(ea.max())), max(p, float(ep.max())))
            assert ea.max() <= force_tol, (self.tag, name, "force", float(ea.max()), int(np.argmax(ea)))
            assert ep.max() <= TOL, (self.tag, name, "phi", float(ep.max()), int(np.argmax(ep)))

    def report(self):
        for form, (a, p) in sorted(self.worst.items()):
            print(f"WORST {self.tag} {form}: force {a:.3e} phi {p:.3e}", flush=True)


def _forces(t, w, theta, eps):
    t.computeForces(w.d, float(theta), G, float(eps))
    return acc_of(w.d)


def _potential(t, w, theta, eps, ref):
    phi = torch.empty(w.n, dtype=torch.float32, device="cuda")
    pe = t.computePotential(w.d, float(theta), G, float(eps), phi)
    pe_ref = 0.5 * (w.ic["mass"].astype(np.float64) * ref.phi).sum()
    assert abs(pe - pe_ref) <= 1e-6 * abs(pe_ref)
    return phi.cpu().numpy()


def _unit_levels(w, count, K):
    """units per replica at which a node of `count` bodies lies in the shared zone, and (where K units can hold it)
    inside a unit: unit_max = n / (level K), shared <=> count > unit_max"""
    levels = [SHARED]
    if count is None:
        levels.append(1)
    elif count <= w.n // K:
        level = max(1, w.n // (K * count))
        assert w.n // (level * K) >= count
        levels.append(level)
    return levels


def _all_forms(w, shape, theta, eps, worst, count=None):
    """every form of the walk over all bodies at (theta, eps) against the reference: values and integers"""
    tr = w.trees[shape]
    plain, aligned, quad = tr["plain"], tr["aligned"], tr["quad"]
    for order, t in ((1, plain), (2, quad)):
        ref = _ref(w, shape, theta, eps, order)
        tag = "" if order == 1 else " order 2"
        t.tuning(1, 0)
        t.walkForm(1)
        t.countVisits(False)
        worst.check("plain" + tag, ref, _forces(t, w, theta, eps))
        t.countVisits(True)
        worst.check("count" + tag, ref, _forces(t, w, theta, eps))
        assert t.stats()["nodes_visited"] == ref.visited, (shape, theta, eps, order)
        assert _hist(t) == (int(ref.tested.sum()), int(ref.accepted.sum())), (shape, theta, eps, order)
        t.countVisits(False)
        for K in (2, 16):
            for level in _unit_levels(w, count, K):
                t.tuning(K, level)
                worst.check(f"split {K}" + tag, ref, _forces(t, w, theta, eps))
        t.tuning(1, 0)
        worst.check("potential" + tag, ref, phi=_potential(t, w, theta, eps, ref))
        out = t.computeField(w.points, float(theta), G, float(eps)).cpu().numpy()
        worst.check("field" + tag, ref, out[:, :3], out[:, 3], extra_phi=_self_term(w, shape, eps, ref))
    ref = _ref(w, shape, theta, eps, 1)
    aligned.tuning(1, 0)
    for form in (3, 2):
        aligned.walkForm(form)
        aligned.countVisits(True)
        worst.check(f"pair {form}", ref, _forces(aligned, w, theta, eps))
        assert aligned.stats()["nodes_visited"] == ref.visited, (shape, theta, eps, form)
        aligned.countVisits(False)
    aligned.walkForm(0)   # the default of a tree without replicas: the pair walk
    worst.check("pair 0", ref, _forces(aligned, w, theta, eps))
    aligned.walkForm(1)   # and the plain walk over the aligned ids
    worst.check("plain aligned", ref, _forces(aligned, w, theta, eps))
    aligned.walkForm(2)


def _one_body(w, shape, case, theta):
    """the Count walk of the target alone, a range of one: (tested, accepted) of that body, and its row"""
    from nbody_amd._lib import check
    t = w.trees[shape]["plain"]
    r = w.r[shape]
    t.tuning(1, 0)
    t.walkForm(1)
    t.countVisits(True)
    out = torch.full((w.n, 4), float("nan"), dtype=torch.float32, device="cuda")
    check(w.ctx._lib.nbody_hip_tree_compute_forces_packed(t._h, int(r.rank[case.target]), 1, float(theta), G, float(case.eps),
                                                         out.data_ptr()))
    got = _hist(t)
    visited = t.stats()["nodes_visited"]
    t.countVisits(False)
    rows = out.cpu().numpy()
    assert np.isnan(rows[np.arange(w.n) != case.target]).all()   # nobody else's row is touched
    return got, visited, rows[case.target, :3]


def test_cases_meet_the_conditions(world):
    w = world
    cases, share = we.check_theta_cases(w.cases["deep"], w.cases["wide"])
    per_combo = {c: sum(k.combo == c for k in cases) for c in we.COMBOS}
    print(f"CASES {len(cases)}, exact equalities {share:.3f}, per combination "
          + " ".join(f"{c[0]}/{c[1]}:{v}" for c, v in per_combo.items()), flush=True)
    for shape in ("deep", "wide"):
        r = w.r[shape]
        for eps, found in w.cases[shape].items():
            for c in found.values():   # the decision from the exported record, through Fractions
                com, half = r.com32[c.node], r.nodes["half_size"][c.node]
                assert we.decide(com, half, w.pos[c.target], c.theta_open, eps) is False
                assert we.decide(com, half, w.pos[c.target], c.theta_accept, eps) is True
                assert c.count <= w.n // 2


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("shape", ["deep", "wide"])
def test_theta_edges_every_form(world, shape, eps, part):
    w = world
    r = w.r[shape]
    found = w.cases[shape][eps]
    worst = Worst(f"{shape} eps {eps}")
    for combo in sorted(found)[part::2]:
        c = found[combo]
        counts = {}
        for theta in (c.theta_open, c.theta_accept):
            _all_forms(w, shape, theta, eps, worst, count=c.count)
            ref = _ref(w, shape, theta, eps, 1)
            (tested, accepted), visited, row = _one_body(w, shape, c, theta)
            assert (tested, accepted) == (int(ref.tested[c.target]), int(ref.accepted[c.target])), (c, theta)
            assert visited == r.walk_detail([c.target], theta, G, eps, 1, first=int(r.rank[c.target])).visited
            assert np.linalg.norm(row - ref.rec.acc[c.target]) <= TOL * ref.rec.scale_acc[c.target], (c, theta)
            counts[theta] = (tested, accepted, r.decisions_of(ref, c.target))
        # between the two thetas: this node accepted, the tests below it gone, nothing else
        (t0, a0, d0), (t1, a1, d1) = counts[c.theta_open], counts[c.theta_accept]
        gone = [k for k in d0 if k not in d1]
        assert d0[c.node] is False and d1[c.node] is True
        assert t1 == t0 - len(gone) and a1 - a0 == 1 - sum(d0[k] for k in gone), c
    worst.report()


@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("theta", [0.0, 2.0])
@pytest.mark.parametrize("shape", ["deep", "wide", "cut"])
def test_theta_zero_and_two(world, shape, theta, eps):
    w = world
    worst = Worst(f"{shape} theta {theta} eps {eps}")
    _all_forms(w, shape, np.float32(theta), eps, worst)
    ref = _ref(w, shape, np.float32(theta), eps, 1)
    if theta == 0.0:
        assert ref.accepted.sum() == 0 and np.all(ref.leaf_bodies == w.n - 1)
    else:   # bodies that accept a node which holds them
        r = w.r[shape]
        slot, node, far = ref.pairs
        inside = far & (r.first[node] <= r.rank[slot]) & (r.rank[slot] < r.last[node])
        print(f"{shape} theta 2 eps {eps}: {int(inside.sum())} acceptances of a node by a body inside it", flush=True)
        if shape != "cut":
            assert inside.any()
    worst.report()


def test_range_walks(world):
    from nbody_amd._lib import check
    w = world
    shape, eps = "deep", 0.05
    case = w.cases[shape][eps][(8, 7)]
    theta = case.theta_open
    r = w.r[shape]
    whole = _ref(w, shape, theta, eps, 1)
    tr = w.trees[shape]
    lib = w.ctx._lib
    tr["plain"].walkForm(1)
    whole_rows = _forces(tr["plain"], w, theta, eps)
    worst = Worst("ranges")
    for count in (1, 63, 64, 65, 257):
        for first in sorted({0, 1, 63, w.n - count}):
            targets = r.order[first:first + count]
            ref = _detail(r, targets, theta, eps, 1, first)
            assert np.array_equal(ref.acc, whole.acc[targets])
            for name, form in (("plain", 1), ("aligned", 2)):
                t = tr[name]
                t.tuning(1, 0)
                t.walkForm(form)
                t.countVisits(True)
                out = torch.full((w.n, 4), float("nan"), dtype=torch.float32, device="cuda")
                check(lib.nbody_hip_tree_compute_forces_packed(t._h, first, count, float(theta), G, eps, out.data_ptr()))
                assert t.stats()["nodes_visited"] == ref.visited, (name, first, count)
                if form == 1:
                    assert _hist(t) == (int(ref.tested.sum()), int(ref.accepted.sum())), (first, count)
                t.countVisits(False)
                rows = out.cpu().numpy()
                rest = np.ones(w.n, bool)
                rest[targets] = False
                assert np.isnan(rows[rest]).all() and (rows[targets, 3] == 0).all()
                worst.check(f"range {name}", ref, rows[targets, :3])
                diff = np.linalg.norm(rows[targets, :3].astype(np.float64) - whole_rows[targets], axis=1)
                assert np.all(diff <= TOL * ref.scale_acc), (name, first, count)
    worst.report()


@pytest.mark.parametrize("order", [1, 2])
def test_point_edges_of_the_field_walk(world, order):
    w = world
    shape = "deep"
    r = w.r[shape]
    t = w.trees[shape]["plain" if order == 1 else "quad"]
    rng = np.random.default_rng(17)
    others = rng.uniform(-9.0, 9.0, (300, 3)).astype(np.float32)
    worst = {}
    for theta in (1.0, 0.5):
        found = we.point_cases(r, theta)
        assert len(found) >= 8, (theta, len(found))
        assert any(True in c.decisions for c in found)
        for c in found:
            we.check_point_case(r.nodes, c)   # fl(theta2 dist2) == size2 from the exported record
            assert c.decisions[0] is False and c.margin >= we.MARGIN
            rp = r.at_points(c.points)
            ref = rp.walk_detail(r.n + np.arange(3), theta, G, 0.0, order)
            alone = [t.computeField(torch.from_numpy(c.points[k:k + 1].copy()).cuda(), theta, G, 0.0).cpu().numpy()[0]
                     for k in range(3)]
            batch = np.concatenate([others[:150], c.points, others[150:]])
            inside = t.computeField(torch.from_numpy(batch).cuda(), theta, G, 0.0).cpu().numpy()[150:153]
            for k in range(3):
                assert np.array_equal(alone[k].view(np.uint32), inside[k].view(np.uint32)), (c.node, theta, k)
                ea = np.linalg.norm(alone[k][:3] - ref.acc[k]) / ref.scale_acc[k]
                ep = abs(alone[k][3] - ref.phi[k]) / ref.scale_phi[k]
                worst[theta] = max(worst.get(theta, 0.0), float(ea), float(ep))
                assert ea <= TOL and ep <= TOL, (c.node, theta, k, float(ea), float(ep), c.decisions)
    for theta, v in worst.items():
        print(f"WORST points order {order} theta {theta}: {v:.3e}", flush=True)
