"""Barnes-Hut path (through the C ABI).  Contract from the reference's tests
(tests/test_barnes_hut.cpp:15-201, tests/test_spatial_hash.cpp:186-249): nodes > 0, root mass =
sum m within 0.1 %, finite accelerations, err(theta=0.3) <= 1.1 err(theta=0.8), theta=0.1 =>
< 10 % magnitude error vs Direct.  Beyond the reference: body-by-body parity (1e-5 relative)
with the oracle's tree, which is built on the same quantised octree."""
import numpy as np
import pytest
import torch

import tree_ref
from gpu_util import acc_of, rel_err, to_device

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _direct(nb, d, G, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(G)
    c.setSofteningParameter(eps)
    c.computeForces(d)
    return acc_of(d)


# tests/test_barnes_hut.cpp:15-36 TreeConstruction, :38-62 MassConservation, :64-94 ComputeForces
def test_tree_construction_mass_conservation_finite(nb, ctx):
    ic = nb.ic.sphere(100, seed=42, radius=5.0)
    d, h = to_device(nb, ic)
    tree = nb.BarnesHutTree(100)
    tree.build(d)
    assert tree.getNodeCount() > 0 and tree.verifyTreeStructure()
    tree.copyNodesToHost()
    assert tree.verifyMassConservation(h)
    calc = nb.BarnesHutCalculator(0.5)
    calc.setGravitationalConstant(1.0)
    calc.setSofteningParameter(0.1)
    calc.computeForces(d)
    assert np.all(np.isfinite(acc_of(d)))
    assert calc.getMethod() == nb.ForceMethod.BARNES_HUT and calc.getTheta() == 0.5


# the tree itself: OctreeNode records are a consistent octree over the Morton order
def test_tree_structure(nb, oracle, ctx):
    n = 5000
    ic = nb.ic.plummer(n, seed=7)
    d, h = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.build(d)
    nodes = tree.copyNodesToHost()
    order = tree.sorted_indices_
    assert np.array_equal(np.sort(order), np.arange(n))
    center, half = oracle.bh_root(ic["pos_x"], ic["pos_y"], ic["pos_z"])
    root = nodes[0]
    assert np.allclose(root["center"], center, atol=1e-6) and root["half_size"] == np.float32(half)
    assert root["particle_count"] == n and not root["is_leaf"]
    assert abs(root["total_mass"] - ic["mass"].sum()) < 1e-5
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)
    leaves = internal = covered = 0
    for k, nd in enumerate(nodes):
        ch = nd["children"][nd["children"] >= 0]
        if nd["is_leaf"]:
            leaves += 1
            assert ch.size == 0 and nd["particle_count"] >= 1
            covered += nd["particle_count"]
            b = nd["particle_index"]
            assert np.all(np.abs(pos[b] - nd["center"]) <= nd["half_size"] * 1.001 + 1e-6)
            if nd["particle_count"] == 1:
                assert np.array_equal(nd["center_of_mass"], pos[b])
        else:
            internal += 1
            assert ch.size >= 1 and nd["particle_count"] > 1
            assert nodes[ch]["particle_count"].sum() == nd["particle_count"]
            assert np.allclose(nodes[ch]["half_size"], nd["half_size"] / 2)
            assert abs(nodes[ch]["total_mass"].sum() - nd["total_mass"]) < 1e-6 * max(1, nd["total_mass"])
            # children sit in the octant their slot names
            for o in range(8):
                c = nd["children"][o]
                if c >= 0:
                    sign = np.array([1 if o & 4 else -1, 1 if o & 2 else -1, 1 if o & 1 else -1])
                    assert np.allclose(nodes[c]["center"], nd["center"] + sign * nd["half_size"] / 2,
                                       rtol=0, atol=1e-5)
    assert covered == n and leaves + internal == len(nodes)
    st = tree.stats()
    assert st["node_count"] == len(nodes) and st["level_base"][0] == 0 and st["level_base"][1] == 1
    # same node count as the oracle's tree
    idx = np.arange(8)
    *_, rm, nc = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], idx, 1.0,
                                          1e-4, 0.5)
    assert nc == len(nodes)
    # ... and node by node the tree of tests/tree_ref.py, which states the nodes from the keys alone
    ref = tree_ref.RefTree(oracle, ic, 20, 1)
    assert np.array_equal(order, ref.order) and st["level_base"] == ref.level_base_plain
    tree_ref.check_nodes(ref, nodes, tag="plummer n = 5000")


# body-by-body parity with the oracle's traversal of the same tree
@pytest.mark.parametrize("n,theta,eps,seed", [(30, 0.5, 0.1, 42), (50, 0.5, 0.1, 42), (1000, 0.3, 0.05, 1),
                                              (4096, 0.5, 0.01, 2), (4096, 0.8, 0.01, 3),
                                              (20000, 0.5, 0.001, 4), (3000, 0.0, 0.02, 5),
                                              (2000, 0.5, 0.0, 6)])
def test_forces_match_oracle_tree(nb, oracle, ctx, n, theta, eps, seed):
    ic = nb.ic.plummer(n, seed=seed) if n >= 1000 else nb.ic.sphere(n, seed=seed, radius=5.0)
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(theta)
    calc.setGravitationalConstant(1.7)
    calc.setSofteningParameter(eps)
    calc.computeForces(d)
    a = acc_of(d)
    eps2 = float(np.float32(eps) * np.float32(eps))
    idx = np.arange(n)
    bx, by, bz, root_mass, nodes = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"],
                                                           ic["mass"], idx, 1.7, eps2, theta)
    ref = np.stack([bx, by, bz], 1)
    e = rel_err(a, ref)
    assert e.max() < TOL, (e.max(), int(np.argmax(e)))
    st = calc.getTree().stats()
    assert st["node_count"] == nodes
    assert abs(st["root_mass"] - root_mass) < 1e-6 * root_mass
    calc.computeForces(d)
    assert np.array_equal(acc_of(d), a)  # bitwise reproducible


# theta = 0 opens everything: Barnes-Hut == Direct
def test_theta_zero_equals_direct(nb, ctx):
    ic = nb.ic.plummer(3000, seed=9)
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(0.0)
    calc.setSofteningParameter(0.01)
    calc.computeForces(d)
    a = acc_of(d)
    ref = _direct(nb, d, 1.0, 0.01)
    assert rel_err(a, ref).max() < TOL


# tests/test_barnes_hut.cpp:131-201 + tests/test_spatial_hash.cpp:186-249: the theta contract
@pytest.mark.parametrize("n,radius", [(30, 5.0), (50, 10.0), (2000, 5.0)])
def test_theta_contract_vs_direct(nb, ctx, n, radius):
    ic = nb.ic.sphere(n, seed=42, radius=radius)
    d, _ = to_device(nb, ic)
    ref = _direct(nb, d, 1.0, 0.1)
    rmag = np.linalg.norm(ref, axis=1)
    errs = {}
    for theta in (0.1, 0.3, 0.5, 0.8):
        calc = nb.BarnesHutCalculator(theta)
        calc.setSofteningParameter(0.1)
        calc.computeForces(d)
        mag = np.linalg.norm(acc_of(d), axis=1)
        errs[theta] = float(np.max(np.abs(mag - rmag) / np.maximum(rmag, 1e-10)))
    assert errs[0.1] < 0.10
    assert errs[0.3] <= 1.1 * errs[0.8] + 1e-7
    assert errs[0.5] < 0.10


# docs claim theta = 0.5 => ~1 % (site/en/benchmarks/algorithm-comparison.md:24): median error
def test_accuracy_at_theta_half(nb, ctx):
    ic = nb.ic.plummer(65536, seed=3)
    d, _ = to_device(nb, ic)
    ref = _direct(nb, d, 1.0, 0.01)
    calc = nb.BarnesHutCalculator(0.5)
    calc.setSofteningParameter(0.01)
    calc.computeForces(d)
    e = rel_err(acc_of(d), ref)
    assert np.median(e) < 0.01 and np.percentile(e, 99) < 0.05


def test_edge_cases_and_errors(nb, oracle, ctx):
    # one body, two bodies, coincident bodies (bucket leaf at the deepest level)
    d, _ = to_device(nb, dict(pos_x=np.array([1.0]), pos_y=np.array([2.0]), pos_z=np.array([3.0]),
                              mass=np.array([5.0])))
    calc = nb.BarnesHutCalculator(0.5)
    calc.setSofteningParameter(0.01)
    calc.computeForces(d)
    assert np.all(acc_of(d) == 0)
    d, _ = to_device(nb, dict(pos_x=np.array([0.0, 1.0]), pos_y=np.zeros(2), pos_z=np.zeros(2),
                              mass=np.ones(2)))
    calc = nb.BarnesHutCalculator(0.5)
    calc.setSofteningParameter(0.0)
    calc.computeForces(d)
    a = acc_of(d)
    assert abs(a[0, 0] - 1) < 1e-5 and abs(a[1, 0] + 1) < 1e-5
    ic = nb.ic.sphere(400, seed=3, radius=2.0)
    for k in ("pos_x", "pos_y", "pos_z"):
        ic[k][10:14] = ic[k][9]   # five coincident bodies
    d, h = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(0.4)
    calc.setSofteningParameter(0.05)
    calc.computeForces(d)
    a = acc_of(d)
    assert np.all(np.isfinite(a))
    idx = np.arange(400)
    ref = np.stack(oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], idx, 1.0,
                                            float(np.float32(0.05) ** 2), 0.4)[:3], 1)
    assert rel_err(a, ref).max() < TOL
    assert calc.getTree().verifyMassConservation(h)
    # errors
    with pytest.raises(nb.ValidationException):
        calc.getTree().computeForces(d, 2.5, 1.0, 0.1)
    big, _ = to_device(nb, nb.ic.sphere(500, seed=1))
    with pytest.raises(nb.ValidationException):
        calc.getTree().build(big)
    cfg = nb.SimulationConfig(force_method=nb.ForceMethod.BARNES_HUT, barnes_hut_theta=0.7)
    c2 = nb.createForceCalculator(cfg.force_method, cfg)
    assert isinstance(c2, nb.BarnesHutCalculator) and c2.getTheta() == pytest.approx(0.7)


# larger leaves (leaf_max > 1) keep the contract and agree with the oracle's tree of that shape
def test_leaf_max_variant(nb, oracle, ctx):
    n = 8000
    ic = nb.ic.plummer(n, seed=12)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.setParams(10, 8)
    tree.build(d)
    tree.computeForces(d, 0.5, 1.0, 0.01)
    a = acc_of(d)
    idx = np.arange(n)
    r = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], idx, 1.0,
                                 float(np.float32(0.01) ** 2), 0.5, 10, 8)
    assert rel_err(a, np.stack(r[:3], 1)).max() < TOL
    assert tree.getNodeCount() == r[4]


# BASELINE config 4 at full size (N = 1,048,576 two-galaxy, theta = 0.5): EVERY body against the oracle's walk of
# the same tree (~1-2 s on the box), on the default pair walk, before and with the cost-ordered schedule (the
# second and third walks after a build are scheduled from the node visits the previous one recorded); node
# count and root mass equal; then the size-independent checks
def test_full_size_two_galaxies(nb, oracle, ctx):
    n = 1 << 20
    ic = nb.ic.two_galaxies(n, seed=42)
    ic["mass"] = (ic["mass"] / np.float32(n)).astype(np.float32)
    d, h = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(0.5)
    calc.setSofteningParameter(0.1)
    calc.computeForces(d)
    a = acc_of(d)
    assert np.all(np.isfinite(a))
    tree = calc.getTree()
    st = tree.stats()
    assert abs(st["root_mass"] - 1.0) < 1e-3 and tree.verifyMassConservation(h)   # :511-519
    assert n < st["node_count"] < 3 * n
    bx, by, bz, root_mass, nodes = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"],
                                                           np.arange(n), 1.0, float(np.float32(0.1) ** 2), 0.5)
    tref = np.stack([bx, by, bz], 1)
    assert st["node_count"] == nodes and abs(st["root_mass"] - root_mass) < 1e-6 * root_mass
    for walk in range(3):
        if walk:
            calc.computeForces(d)   # scheduled longest-first from the previous walk's visit counts
        e = rel_err(acc_of(d), tref)
        msg = (f"N = {n} walk {walk}: all {n} bodies, max {e.max():.3e}, p99.99 {np.quantile(e, 0.9999):.3e}, "
               f"median {np.median(e):.3e}, above 1e-5: {(e > TOL).sum()}")
        print(msg)
        assert e.max() < TOL, msg
        assert np.array_equal(acc_of(d), a)  # the schedule does not change a bit
    # sampled bodies against the exact sum (oracle, fp64-accumulated): the theta = 0.5 contract
    idx = np.linspace(0, n - 1, 96).astype(np.int64)
    ref = np.stack(oracle.direct_forces_indexed(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], idx,
                                                1.0, float(np.float32(0.1) ** 2), 1), 1)
    e = rel_err(a[idx], ref)
    assert np.median(e) < 0.01 and e.max() < 0.10
    # theta = 0 on the same tree is the exact sum
    tree.computeForces(d, 0.0, 1.0, 0.1)
    assert rel_err(acc_of(d)[idx], ref).max() < TOL


# the split walk (few bodies: K replicas share each wave's walk) against the plain walk: same
# interactions, different summation grouping -> equal to fp rounding; every setting reproducible
@pytest.mark.parametrize("n,eps,max_depth", [(6000, 0.02, 10), (6000, 0.0, 10), (700, 0.05, 10), (5000, 0.02, 3),
                                             (5000, 0.02, 2), (64, 0.05, 10)])
def test_split_walk_equals_plain_walk(nb, ctx, n, eps, max_depth):
    ic = nb.ic.plummer(n, seed=21)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.setParams(max_depth, 1)
    tree.build(d)
    tree.tuning(1, 0)
    tree.computeForces(d, 0.6, 1.0, eps)
    plain = acc_of(d)
    assert np.isfinite(plain).all()
    for replicas, level in ((2, 1), (4, 2), (16, 3), (16, 64), (8, 1024), (0, 0)):  # (replicas, units per replica)
        tree.tuning(replicas, level)
        tree.computeForces(d, 0.6, 1.0, eps)
        a = acc_of(d)
        assert rel_err(a, plain).max() < 5e-6, (replicas, level)
        tree.computeForces(d, 0.6, 1.0, eps)
        assert np.array_equal(acc_of(d), a), (replicas, level)
    with pytest.raises(nb.ValidationException):
        tree.tuning(17, 0)


# the pair walk (two siblings per packed instruction, node records as pair blocks) against the plain walk: the same
# interaction lists, a sibling group summed as (even siblings) + (odd siblings) -> equal to fp32 rounding;
# reproducible; ragged sizes, eps = 0 (coincident-body guard), depth-limited and wide leaves (body-by-body path)
@pytest.mark.parametrize("n,eps,max_depth,leaf_max", [(40000, 0.02, 20, 1), (40001, 0.0, 20, 1), (3000, 0.05, 10, 1),
                                                      (129, 0.05, 20, 1), (20000, 0.02, 3, 1), (20000, 0.01, 20, 8),
                                                      (20000, 0.0, 4, 1), (300001, 0.02, 20, 1), (131072, 0.02, 20, 1)])
def test_pair_walk_equals_plain_walk(nb, ctx, n, eps, max_depth, leaf_max):
    ic = nb.ic.two_galaxies(n, seed=23)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.setParams(max_depth, leaf_max)
    tree.walkForm(2)   # before the build: small trees get the even-aligned node ids of the pair walk only on request
    tree.build(d)
    tree.tuning(1, 0)
    tree.walkForm(1)
    tree.computeForces(d, 0.5, 1.0, eps)
    plain = acc_of(d)
    assert np.isfinite(plain).all()
    first = None
    for form in (3, 2, 0):  # 3: plain order; 2 / 0: the second call runs the cost-ordered schedule
        tree.walkForm(form)
        tree.computeForces(d, 0.5, 1.0, eps)
        a = acc_of(d)
        assert rel_err(a, plain).max() < 1e-5, form
        tree.computeForces(d, 0.5, 1.0, eps)
        assert np.array_equal(acc_of(d), a), form
        first = a if first is None else first
        assert np.array_equal(a, first), form  # the schedule does not change a bit
    # node visits are those of the plain walk
    tree.walkForm(2)
    tree.countVisits(True)
    tree.computeForces(d, 0.5, 1.0, eps)
    pair_visits = tree.stats()["nodes_visited"]
    tree.walkForm(1)
    tree.computeForces(d, 0.5, 1.0, eps)
    assert tree.stats()["nodes_visited"] == pair_visits
    tree.countVisits(False)
    with pytest.raises(nb.ValidationException):
        tree.walkForm(4)
    if n < 98304:   # a small tree built with plain ids refuses the pair walk instead of walking misaligned blocks
        tree.walkForm(0)
        tree.build(d)
        tree.computeForces(d, 0.5, 1.0, eps)
        auto = acc_of(d)
        assert rel_err(auto, plain).max() < 1e-5
        tree.walkForm(2)
        with pytest.raises(nb.NBodyError, match="before the build"):
            tree.computeForces(d, 0.5, 1.0, eps)
        tree.walkForm(0)


# the cost-ordered schedule under extreme skew: a compact core inside a wide box (a few waves carry most of the
# node visits, so the per-XCD ranges hit their caps); every body walked exactly once, bit for bit the plain order
def test_pair_walk_schedule_skewed_costs(nb, ctx):
    n = 400000
    ic = nb.ic.plummer(n, seed=9, a=0.05, rmax=200.0)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.build(d)
    tree.walkForm(3)
    tree.computeForces(d, 0.5, 1.0, 1e-3)
    plain_order = acc_of(d)
    assert np.isfinite(plain_order).all()
    tree.walkForm(2)
    for _ in range(3):  # first call records the costs, the next ones are scheduled
        tree.computeForces(d, 0.5, 1.0, 1e-3)
        assert np.array_equal(acc_of(d), plain_order)


# non-finite positions (a blown-up run) must not hang or fault the walk: a NaN / inf body spoils the monopoles above
# it, and the sums that use them, but every form of the walk terminates (the pair walk counts a NaN distance as
# "far", the plain walk opens down to the leaf) and a later build of finite bodies is clean again
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_walk_survives_non_finite_positions(nb, ctx, bad):
    n = 150000
    ic = nb.ic.plummer(n, seed=5)
    ic["pos_x"][1234] = bad
    ic["pos_z"][77777] = -bad
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.build(d)
    for form in (1, 2, 2, 3):
        tree.walkForm(form)
        tree.computeForces(d, 0.5, 1.0, 0.01)
        assert acc_of(d).shape == (n, 3)
    good = nb.ic.plummer(n, seed=5)
    d2, _ = to_device(nb, good)
    tree.walkForm(0)
    tree.build(d2)
    tree.computeForces(d2, 0.5, 1.0, 0.01)
    assert np.isfinite(acc_of(d2)).all()


# sizes on both sides of the automatic switches (prefix monopoles, replicas 4 -> 2, split walk -> pair walk)
@pytest.mark.parametrize("n", [16384, 50000, 70000, 98303, 98304])
def test_forces_match_oracle_tree_mid_sizes(nb, oracle, ctx, n):
    ic = nb.ic.two_galaxies(n, seed=8)
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(0.5)
    calc.setSofteningParameter(0.02)
    calc.computeForces(d)
    a = acc_of(d)
    r = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], np.arange(n), 1.0,
                                 float(np.float32(0.02) ** 2), 0.5)
    assert rel_err(a, np.stack(r[:3], 1)).max() < TOL
    assert calc.getTree().stats()["node_count"] == r[4]


# 8e: ranks walk disjoint ranges of the same (replicated) tree; together they give the whole walk
@pytest.mark.parametrize("n,parts", [(300000, 4), (300000, 1), (9000, 3), (600000, 2)])
def test_range_walks_equal_whole_walk(nb, ctx, n, parts):
    import ctypes as C
    from gpu_util import packed
    from nbody_amd._lib import check
    ic = nb.ic.two_galaxies(n, seed=4)
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(0.5)
    calc.setSofteningParameter(0.05)
    calc.computeForces(d)
    whole = acc_of(d)
    posm = packed(ic)
    lib = ctx._lib
    h = C.c_void_p()
    check(lib.nbody_hip_tree_create(ctx.handle, n, C.byref(h)))
    try:
        check(lib.nbody_hip_tree_build_packed(h, posm.data_ptr(), n))
        out = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
        cuts = [(n * k) // parts for k in range(parts + 1)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            check(lib.nbody_hip_tree_compute_forces_packed(h, lo, hi - lo, 0.5, 1.0, 0.05, out.data_ptr()))
        got = out.cpu().numpy()
        assert np.isfinite(got).all()            # every row written by some range
        assert (got[:, 3] == 0).all()
        if n // parts >= 98304:                   # the walk without replicas on both sides: bit for bit
            assert np.array_equal(got[:, :3], whole)
        else:                                     # the split walk's replica count depends on the range length
            assert rel_err(got[:, :3], whole).max() < 5e-6
        # a rank walks the same range every step: the second walk of a range runs the cost-ordered schedule
        lo, hi = cuts[-2], cuts[-1]
        check(lib.nbody_hip_tree_compute_forces_packed(h, lo, hi - lo, 0.5, 1.0, 0.05, out.data_ptr()))
        assert np.array_equal(out.cpu().numpy(), got)
        with pytest.raises(nb.ValidationException):
            check(lib.nbody_hip_tree_compute_forces_packed(h, n - 5, 6, 0.5, 1.0, 0.05, out.data_ptr()))
        check(lib.nbody_hip_tree_compute_forces_packed(h, n, 0, 0.5, 1.0, 0.05, out.data_ptr()))  # empty range: no-op
    finally:
        lib.nbody_hip_tree_destroy(h)


# BASELINE config 4 in small, against the committed golden vectors (tests/golden/make_golden.py)
def test_golden_two_galaxies_2048(nb, ctx):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twogalaxies2048_barnes_hut.npz"))
    ic = {k: g[k] for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(float(g["theta"]))
    calc.setGravitationalConstant(float(g["G"]))
    calc.setSofteningParameter(float(g["eps"]))
    calc.computeForces(d)
    assert rel_err(acc_of(d), g["acc"]).max() < TOL
    st = calc.getTree().stats()
    assert st["node_count"] == int(g["node_count"])
    assert abs(st["root_mass"] - float(g["root_mass"])) < 1e-6 * float(g["root_mass"])


# BASELINE config 4 as an acceptance test: N = 1,048,576, Barnes-Hut theta = 0.5, eps = 0.1, dt = 1e-3,
# 10,000 Velocity-Verlet steps, total energy (KE + exact all-pairs PE, both fp64) sampled every 500
# steps.  Requirement (ref: openspec/specs/force-computation.md:79-81): drift < 1 % per 1,000 steps;
# asserted here 10x tighter over 10x as many steps.  The two-galaxy system of SURVEY 8d is dominated by
# free-streaming kinetic energy (KE 3.46 vs PE -0.049 with unit total mass), so |dE|/|E0| flatters
# it: |dE|/|PE0| is asserted as well.  The bound Plummer sphere (E0 = KE + PE ~ -0.15) is the strict case.
@pytest.mark.parametrize("which,eps,tol_e,tol_pe", [("two_galaxies", 0.1, 1e-3, 2e-2), ("plummer", 0.01, 1e-4, 1e-4)])
def test_config4_energy_drift_10k_steps(nb, ctx, which, eps, tol_e, tol_pe):
    import time
    n, G, dt, theta, steps, every = 1 << 20, 1.0, 1e-3, 0.5, 10000, 500
    if which == "plummer":
        ic = nb.ic.plummer(n, seed=42)
    else:
        ic = nb.ic.two_galaxies(n, seed=42)
        ic["mass"] = (ic["mass"] / np.float32(n)).astype(np.float32)  # unit total mass
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(theta)
    calc.setGravitationalConstant(G)
    calc.setSofteningParameter(eps)
    integ = nb.Integrator()
    calc.computeForces(d)
    ke0, pe0 = integ.computeEnergiesF64(d, G, eps)
    e0 = ke0 + pe0
    worst = 0.0
    t_steps = 0.0
    for s0 in range(0, steps, every):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(every):
            integ.integrate(d, calc, dt)
        torch.cuda.synchronize()
        t_steps += time.perf_counter() - t0
        ke, pe = integ.computeEnergiesF64(d, G, eps)
        assert np.isfinite(ke) and np.isfinite(pe)
        worst = max(worst, abs(ke + pe - e0))
    print(f"{which}: N = {n}, {steps} steps at {1e3 * t_steps / steps:.3f} ms/step; KE0 {ke0:.6e} PE0 {pe0:.6e}; "
          f"max |dE|/|E0| = {worst / abs(e0):.3e}, max |dE|/|PE0| = {worst / abs(pe0):.3e}")
    assert worst / abs(e0) < tol_e, f"max |dE|/|E0| = {worst / abs(e0):.3e}"
    assert worst / abs(pe0) < tol_pe, f"max |dE|/|PE0| = {worst / abs(pe0):.3e}"


# Trees deeper than the 30-bit keys of the reference's Morton code (ref: force_barnes_hut.cu:23-38; its
# host insertion goes down to depth 20, :363): max_depth 11..21 switches to 63-bit keys (21 bits per axis).
# Body by body against the oracle's tree of the same shape, on a cluster whose core is far denser than
# a depth-10 cell, with coincident bodies (which stay together in a deepest leaf at any depth).
@pytest.mark.parametrize("max_depth,leaf_max", [(11, 1), (14, 1), (21, 1), (16, 4), (10, 1)])
def test_deep_tree_matches_oracle(nb, oracle, ctx, max_depth, leaf_max):
    n = 6000
    ic = nb.ic.plummer(n, seed=13, a=0.002, rmax=40.0)      # scale length 0.002 ...
    for c in range(8):                                        # ... inside a box of +-8 (eight far bodies): the whole
        for b, k in enumerate(("pos_x", "pos_y", "pos_z")):   # core sits in a handful of depth-10 cells
            ic[k][c] = 8.0 if (c >> b) & 1 else -8.0
    for k in ("pos_x", "pos_y", "pos_z"):
        ic[k][100:140] = ic[k][100]                           # 40 coincident bodies
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.setParams(max_depth, leaf_max)
    tree.build(d)
    eps, theta, G = 1e-4, 0.6, 1.0
    tree.computeForces(d, theta, G, eps)
    a = acc_of(d)
    r = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], np.arange(n), G,
                                 float(np.float32(eps) ** 2), theta, max_depth, leaf_max)
    assert tree.getNodeCount() == r[4]
    assert abs(tree.stats()["root_mass"] - r[3]) < 1e-6 * r[3]
    ref = np.stack(r[:3], 1)
    nz = np.linalg.norm(ref, axis=1) > 0
    assert rel_err(a[nz], ref[nz]).max() < TOL
    nodes = tree.copyNodesToHost()
    deepest = nodes["particle_count"][nodes["is_leaf"]].max()
    half = nodes["half_size"]
    assert np.isclose(half.min(), half[0] * 2.0 ** -min(max_depth, int(np.round(np.log2(half[0] / half.min())))))
    if max_depth == 21 and leaf_max == 1:
        assert deepest == 40          # only the coincident bodies still share a leaf
    if max_depth == 10:
        assert deepest > 100          # 30-bit keys cannot resolve the core
    # the geometry of every node contains its bodies' centre of mass
    inside = np.all(np.abs(nodes["center_of_mass"] - nodes["center"]) <= half[:, None] * 1.0001 + 1e-6, axis=1)
    assert inside[nodes["total_mass"] > 0].all()


# the depth a tree reached is reported beyond level 10 (round 2 exported 12 levels only: getMaxDepth saturated)
def test_max_depth_reported_for_deep_trees(nb, ctx):
    n = 50000
    ic = nb.ic.plummer(n, seed=3, a=0.01, rmax=50.0)     # a compact core in a wide box
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.build(d)
    lb = tree.stats()["level_base"]
    assert len(lb) == 24 and lb[0] == 0 and lb[1] == 1
    depth = tree.getMaxDepth()
    assert 10 < depth <= 20, depth
    assert all(lb[l] < lb[l + 1] for l in range(depth + 1)) and lb[depth + 1] == tree.getNodeCount()
    tree.setParams(8, 1)
    tree.build(d)
    assert tree.getMaxDepth() == 8


# A tree that needs more nodes than its arrays hold (nbody_hip_tree_limit_nodes forces it; without the hook the
# arrays stop at 2^28 - 1 nodes) is CUT where the numbering passes the capacity: the nodes beyond do not exist and
# their parents are leaves of several bodies, which interact body by body.  Forces stay right: theta = 0 still
# gives the exact direct sum, theta = 0.5 is at least as close to it as the full tree.  (Round 2 tested the
# condition on the clamped total, so the fallback was dead and truncated subtrees would have been dropped.)
@pytest.mark.parametrize("n,limit", [(20000, 9000), (20000, 21000), (120000, 100000), (5000, 16)])
def test_node_overflow_is_cut_not_wrong(nb, oracle, ctx, n, limit):
    ic = nb.ic.plummer(n, seed=21)
    d, h = to_device(nb, ic)
    eps, G = 0.01, 1.0
    direct = _direct(nb, d, G, eps)
    full = nb.BarnesHutTree(n)
    full.build(d)
    full.computeForces(d, 0.5, G, eps)
    a_full = acc_of(d)
    total_nodes = full.getNodeCount()
    assert total_nodes > limit
    tree = nb.BarnesHutTree(n)
    tree.limitNodes(limit)
    tree.build(d)
    assert 0 < tree.getNodeCount() <= limit          # ids (holes of the even-aligned groups included) stop at the cap
    assert abs(tree.stats()["root_mass"] - ic["mass"].sum()) < 1e-5
    tree.computeForces(d, 0.0, G, eps)                    # opens everything: every leaf body by body
    assert rel_err(acc_of(d), direct).max() < TOL
    tree.computeForces(d, 0.5, G, eps)
    a_cut = acc_of(d)
    e_cut, e_full = rel_err(a_cut, direct), rel_err(a_full, direct)
    print(f"n = {n}: {total_nodes} nodes cut to {limit}; median error vs direct {np.median(e_cut):.2e} (full tree {np.median(e_full):.2e})")
    assert np.median(e_cut) <= np.median(e_full) * 1.05 and e_cut.max() < 0.1
    tree.computeForces(d, 0.5, G, eps)
    assert np.array_equal(acc_of(d), a_cut)
    # the nodes reachable from the root still partition the bodies (nodes whose group straddles the capacity are
    # written but orphaned: their parent is a leaf)
    nodes = tree.copyNodesToHost()
    stack, covered, biggest = [0], 0, 0
    while stack:
        nd = nodes[stack.pop()]
        if nd["is_leaf"]:
            covered += int(nd["particle_count"])
            biggest = max(biggest, int(nd["particle_count"]))
        else:
            stack.extend(int(c) for c in nd["children"] if c >= 0)
    assert covered == n and biggest > 1
    tree.limitNodes(0)                                     # back to the bound: the full tree again
    tree.build(d)
    assert tree.getNodeCount() == total_nodes
    with pytest.raises(nb.ValidationException):
        tree.limitNodes(5)


def test_deep_tree_parameter_errors(nb, ctx):
    tree = nb.BarnesHutTree(1000)
    with pytest.raises(nb.ValidationException):
        tree.setParams(22, 1)
    with pytest.raises(nb.ValidationException):
        tree.setParams(0, 1)
    big = nb.BarnesHutTree(60_000_000)
    with pytest.raises(nb.ValidationException, match="2\\^28 nodes"):
        big.setParams(21, 1)          # 12 n nodes would not fit the 28-bit node ids
    big.setParams(21, 64)             # with wider leaves it does


# N = 2^21 Plummer sphere: the core holds dozens of bodies per depth-10 cell; at depth 16 every leaf holds
# one body again (up to exact coincidences).  Sampled bodies against the oracle's depth-16 tree.
def test_deep_tree_large_plummer(nb, oracle, ctx):
    import time
    n = 1 << 21
    ic = nb.ic.plummer(n, seed=42, a=0.1, rmax=100.0)    # a 10x more compact core than the bench's sphere
    d, _ = to_device(nb, ic)
    out = {}
    for depth in (10, 16):
        tree = nb.BarnesHutTree(n)
        tree.setParams(depth, 1)
        tree.build(d)
        tree.computeForces(d, 0.5, 1.0, 1e-3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            tree.build(d)
        torch.cuda.synchronize()
        tb = (time.perf_counter() - t0) / 3
        t0 = time.perf_counter()
        for _ in range(3):
            tree.computeForces(d, 0.5, 1.0, 1e-3)
        torch.cuda.synchronize()
        tw = (time.perf_counter() - t0) / 3
        nodes = tree.copyNodesToHost()
        leaf = nodes["is_leaf"]
        out[depth] = dict(acc=acc_of(d), nodes=int(tree.getNodeCount()), max_leaf=int(nodes["particle_count"][leaf].max()),
                          build_ms=tb * 1e3, walk_ms=tw * 1e3)
        print(f"N = {n}, max_depth {depth}: {out[depth]['nodes']} nodes, largest leaf {out[depth]['max_leaf']} bodies, "
              f"build {tb * 1e3:.2f} ms, walk {tw * 1e3:.2f} ms")
        del tree, nodes
    assert out[10]["max_leaf"] > 100 and out[16]["max_leaf"] * 50 < out[10]["max_leaf"]
    idx = np.concatenate([np.linspace(0, n - 1, 96).astype(np.int64),
                          np.argsort(ic["pos_x"] ** 2 + ic["pos_y"] ** 2 + ic["pos_z"] ** 2)[:96]])
    r = oracle.barnes_hut_forces(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], idx, 1.0,
                                 float(np.float32(1e-3) ** 2), 0.5, 16, 1)
    assert out[16]["nodes"] == r[4]
    assert rel_err(out[16]["acc"][idx], np.stack(r[:3], 1)).max() < TOL
    # both trees approximate the same sum: they agree to the theta = 0.5 accuracy
    e = rel_err(out[16]["acc"][idx], out[10]["acc"][idx])
    assert np.median(e) < 0.01
