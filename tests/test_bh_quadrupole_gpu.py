"""Barnes-Hut multipole order 2 (nbody_hip_tree_set_multipole_order) on a real GPU: the moments against the bodies, the
walk and the potential against the fp64 restatement (tests/quadrupole_ref.py), the interaction lists of order 1, the
accuracy against Direct, the paths that must agree, order 1 untouched, errors, ParticleSystem and the facade."""
import os
import subprocess

import numpy as np
import pytest
import torch

import quadrupole_ref as qr
import tree_ref
from gpu_util import acc_of, packed, rel_err, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")
TOL = 1e-5


def _fixture():
    z = np.load(os.path.join(GOLDEN, "twogalaxies2048_barnes_hut.npz"))
    return {k: z[k] for k in KEYS}


def _pop(nb, which):
    if which == "twogalaxies2048":
        return _fixture()
    if which == "plummer20000":
        return nb.ic.plummer(20000, seed=12)
    if which == "plummer65536":
        return nb.ic.plummer(65536, seed=3)
    raise KeyError(which)


def _pos(ic):
    return np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)


def _tree(nb, d, order, params=None, limit=0):
    t = nb.BarnesHutTree(d.count)
    if params:
        t.setParams(*params)
    if limit:
        t.limitNodes(limit)
    t.setMultipoleOrder(order)
    t.build(d)
    return t


def _forces(t, d, theta, G, eps):
    t.computeForces(d, theta, G, eps)
    return acc_of(d).astype(np.float64)


def _phi(t, d, theta, G, eps):
    phi = torch.empty(d.count, dtype=torch.float32, device="cuda")
    pe = t.computePotential(d, theta, G, eps, phi)
    return phi.cpu().numpy().astype(np.float64), pe


def _direct(nb, d, G, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(G)
    c.setSofteningParameter(eps)
    c.computeForces(d)
    a = acc_of(d).astype(np.float64)
    phi = torch.empty(d.count, dtype=torch.float32, device="cuda")
    pe = c.computePotential(d, phi)
    return a, phi.cpu().numpy().astype(np.float64), pe


def _restatement(t, ic):
    nodes = t.copyNodesToHost()
    return qr.Restatement(nodes, t.sorted_indices_, _pos(ic), ic["mass"])


# 1. Moments: every node of the export against fp64 S from its bodies
@pytest.mark.parametrize("which", ["plummer65536", "twogalaxies2048"])
def test_moments_against_bodies(nb, oracle, ctx, which):
    ic = _pop(nb, which)
    d, _ = to_device(nb, ic)
    t = _tree(nb, d, 2)
    mom = t.copyMomentsToHost().astype(np.float64)
    r = _restatement(t, ic)
    assert mom.shape == (len(r.M), 6)
    tr = r.S[:, :3].sum(1)
    err = np.abs(mom - r.S).max(1)
    worst = float((err / np.maximum(tr, 1e-300))[tr > 0].max())
    print(f"{which}: {len(tr)} nodes, worst |S - S_ref| / tr S = {worst:.3e}")
    assert np.all(err <= 4e-7 * tr + 1e-30), np.flatnonzero(err > 4e-7 * tr)[:10]
    one = r.last - r.first == 1
    assert np.all(mom[one] == 0.0)
    # positive semi-definite within rounding: the eigenvalues of every node's S
    full = np.stack([mom[:, [0, 3, 4]], mom[:, [3, 1, 5]], mom[:, [4, 5, 2]]], 1)
    lam = np.linalg.eigvalsh(full)
    assert np.all(lam[:, 0] >= -1e-6 * np.maximum(tr, 1e-300))
    # the same moments against tests/tree_ref.py, whose body ranges do not come from the export under test
    ref = tree_ref.RefTree(oracle, ic, 20, 1)
    tree_ref.check_nodes(ref, t.copyNodesToHost(), tag=which)
    tree_ref.check_moments(ref, mom, tag=which)
    t1 = _tree(nb, d, 1)
    with pytest.raises(nb.StateException):
        t1.copyMomentsToHost()


# 2. Restatement parity: order 1 validates the restatement against the oracle-pinned walk, then order 2
def _parity(nb, ic, d, t, theta, eps, order, G=1.0, targets=None, tag=""):
    r = _restatement(t, ic)
    idx = np.arange(d.count) if targets is None else targets
    a_ref, phi_ref = r.walk(idx, theta, G, eps, order)
    a = _forces(t, d, theta, G, eps)[idx]
    e = rel_err(a, a_ref)
    phi, pe = _phi(t, d, theta, G, eps)
    ep = np.abs(phi[idx] - phi_ref) / np.abs(phi_ref)
    print(f"{tag} order {order} theta {theta} eps {eps}: force max rel err {e.max():.3e}, phi {ep.max():.3e}")
    assert e.max() <= TOL, (e.max(), int(np.argmax(e)))
    assert ep.max() <= TOL, (ep.max(), int(np.argmax(ep)))
    if targets is None:
        pe_ref = 0.5 * (ic["mass"].astype(np.float64) * phi_ref).sum()
        assert abs(pe - pe_ref) <= 1e-6 * abs(pe_ref)


@pytest.mark.parametrize("which", ["twogalaxies2048", "plummer20000"])
@pytest.mark.parametrize("theta", [0.3, 0.5, 0.8])
@pytest.mark.parametrize("eps", [0.1, 1e-3, 0.0])
def test_restatement_parity(nb, ctx, which, theta, eps):
    ic = _pop(nb, which)
    d, _ = to_device(nb, ic)
    for order in (1, 2):
        _parity(nb, ic, d, _tree(nb, d, order), theta, eps, order, tag=which)


@pytest.mark.parametrize("params,limit,a", [((21, 4), 0, 0.2), ((20, 1), 9000, 1.0)])
def test_restatement_parity_deep_and_cut_trees(nb, ctx, params, limit, a):
    # deep trees with leaves of up to four bodies (a compact core); a tree cut at 9,000 nodes (the case of
    # test_node_overflow_is_cut_not_wrong: leaves of several bodies where the numbering passed the capacity)
    ic = nb.ic.plummer(20000, seed=21 if limit else 13, a=a)
    d, _ = to_device(nb, ic)
    for order in (1, 2):
        _parity(nb, ic, d, _tree(nb, d, order, params, limit), 0.5, 1e-3, order, tag=f"params {params} limit {limit}")


# 3. Same interaction lists as order 1; theta = 0 is the Direct sum
@pytest.mark.parametrize("n", [6000, 131072])
def test_same_interaction_lists(nb, ctx, n):
    ic = nb.ic.two_galaxies(n, seed=5)
    d, _ = to_device(nb, ic)
    seen = []
    for order in (1, 2):
        t = _tree(nb, d, order)
        t.walkForm(1)
        t.countVisits(True)
        t.computeForces(d, 0.5, 1.0, 0.05)
        seen.append((t.stats()["nodes_visited"], _hist(t)))
    assert seen[0] == seen[1]


def _hist(t):
    import ctypes as C
    out = (C.c_ulonglong * 130)()
    from nbody_amd._lib import check
    check(t.ctx._lib.nbody_hip_tree_visit_histogram(t._h, C.byref(out)))
    return list(out)


def test_theta_zero_equals_direct(nb, ctx):
    ic = nb.ic.plummer(3000, seed=9)
    d, _ = to_device(nb, ic)
    ref, phi_ref, pe_ref = _direct(nb, d, 1.0, 0.01)
    t = _tree(nb, d, 2)
    assert rel_err(_forces(t, d, 0.0, 1.0, 0.01), ref).max() < TOL
    phi, pe = _phi(t, d, 0.0, 1.0, 0.01)
    assert (np.abs(phi - phi_ref) / np.abs(phi_ref)).max() < TOL and abs(pe - pe_ref) <= 1e-6 * abs(pe_ref)


# 4. Accuracy against Direct.  Tier 1 (structural): order 2 <= 0.5 x order 1 at theta 0.3 / 0.5, <= 0.8 x at 0.8.
# Tier 2 (regression): <= 1.6 x the values measured on MI355X (profiles/r05_bh_quadrupole_tests.log).
MEASURED = {  # order 2, tests/test_bh_quadrupole_gpu.py on MI355X (profiles/r05_bh_quadrupole_tests.log)
    "config4": {0.3: {"median": 8.7103e-05, "p99": 4.4570e-04, "rms": 1.4552e-04, "phi": 1.7075e-05, "pe": 5.9091e-06},
                0.5: {"median": 6.0336e-04, "p99": 3.0788e-03, "rms": 1.0231e-03, "phi": 6.8241e-05, "pe": 4.6629e-05},
                0.8: {"median": 4.1719e-03, "p99": 2.2111e-02, "rms": 7.0810e-03, "phi": 4.9154e-04, "pe": 4.0971e-04}},
    "plummer65536": {0.3: {"median": 5.0353e-05, "p99": 2.1387e-04, "rms": 7.2693e-05, "phi": 1.0576e-05, "pe": 4.7561e-07},
                     0.5: {"median": 3.5098e-04, "p99": 1.6166e-03, "rms": 5.2372e-04, "phi": 5.2198e-05, "pe": 1.2638e-06},
                     0.8: {"median": 2.3435e-03, "p99": 1.0569e-02, "rms": 3.5385e-03, "phi": 2.6661e-04, "pe": 2.0250e-06}},
}


def _accuracy(nb, d, theta, G, eps, ref, phi_ref, pe_ref, order):
    t = _tree(nb, d, order)
    e = rel_err(_forces(t, d, theta, G, eps), ref)
    phi, pe = _phi(t, d, theta, G, eps)
    ep = (phi - phi_ref) / np.abs(phi_ref)
    return t, {"median": float(np.median(e)), "p99": float(np.percentile(e, 99)), "rms": float(np.sqrt((e * e).mean())),
               "phi": float(np.sqrt((ep * ep).mean())), "pe": abs(pe - pe_ref) / abs(pe_ref)}


@pytest.mark.parametrize("which", ["config4", "plummer65536"])
def test_accuracy_against_direct(nb, ctx, which):
    if which == "config4":
        ic, G, eps = nb.ic.two_galaxies(1 << 20, seed=42), 1.0, 0.1
    else:
        ic, G, eps = nb.ic.plummer(65536, seed=3), 1.0, 0.01
    d, _ = to_device(nb, ic)
    ref, phi_ref, pe_ref = _direct(nb, d, G, eps)
    for theta, factor in ((0.3, 0.5), (0.5, 0.5), (0.8, 0.8)):
        _, s1 = _accuracy(nb, d, theta, G, eps, ref, phi_ref, pe_ref, 1)
        t2, s2 = _accuracy(nb, d, theta, G, eps, ref, phi_ref, pe_ref, 2)
        print(f"{which} theta {theta}: order 1 " + " ".join(f"{k} {v:.4e}" for k, v in s1.items()))
        print(f"{which} theta {theta}: order 2 " + " ".join(f"{k} {v:.4e}" for k, v in s2.items()))
        for k in s1:
            assert s2[k] <= factor * s1[k], (theta, k, s2[k], s1[k])
            assert s2[k] <= 1.6 * MEASURED[which][theta][k], (theta, k, s2[k], MEASURED[which][theta][k])
        if which == "config4" and theta == 0.5:
            # 2,048 sampled bodies of config 4 at full size against the restatement
            sample = np.random.default_rng(7).choice(d.count, 2048, replace=False)
            _parity(nb, ic, d, t2, theta, eps, 2, G, sample, tag="config4 sampled")


# 5. The gradient of the order-2 phi is -a, with displacements that keep every interaction list
def test_gradient_of_phi_is_minus_the_force(nb, ctx):
    rng = np.random.default_rng(4)
    # two flattened clusters far apart: each sees the other through accepted internal nodes
    a = rng.normal(size=(96, 3)) * np.array([1.0, 0.8, 0.1])
    b = rng.normal(size=(96, 3)) * np.array([0.6, 1.0, 0.2]) + np.array([12.0, 3.0, 1.0])
    pos = np.concatenate([a, b]).astype(np.float32)
    m = rng.uniform(0.5, 2.0, len(pos)).astype(np.float32)
    ic = {"pos_x": pos[:, 0].copy(), "pos_y": pos[:, 1].copy(), "pos_z": pos[:, 2].copy(), "mass": m}
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k] = np.zeros(len(m), np.float32)
    d, _ = to_device(nb, ic)
    G, eps, theta, h = 1.0, 0.05, 0.7, 1e-3
    t = _tree(nb, d, 2)
    acc = _forces(t, d, theta, G, eps)
    r0 = _restatement(t, ic).interaction_counts(np.arange(len(m)), theta, eps)
    assert r0[:, 0].min() > 0  # every body accepts internal nodes
    phi = torch.empty(len(m), dtype=torch.float32, device="cuda")
    checked = 0
    for i in range(0, len(m), 8):
        grad = np.zeros(3)
        ok = True
        for ax, key in enumerate(("pos_x", "pos_y", "pos_z")):
            arr = getattr(d, key)
            x0 = ic[key][i]
            vals = []
            for x in (np.float32(x0 + h), np.float32(x0 - h)):
                arr[i] = float(x)
                t.build(d)
                moved = dict(ic)
                moved[key] = ic[key].copy()
                moved[key][i] = x
                ok &= np.array_equal(_restatement(t, moved).interaction_counts([i], theta, eps)[0], r0[i])
                t.computePotential(d, theta, G, eps, phi)
                vals.append(float(phi[i].item()))
            arr[i] = float(x0)
            grad[ax] = (vals[0] - vals[1]) / (float(np.float32(x0 + h)) - float(np.float32(x0 - h)))
        t.build(d)
        if not ok:
            continue  # a displacement changed the body's interaction list: phi jumps there by construction
        checked += 1
        ulp = float(np.spacing(np.float32(abs(vals[0]) + abs(vals[1]))))
        assert np.linalg.norm(grad + acc[i]) <= 2e-3 * np.linalg.norm(acc[i]) + np.sqrt(3) * ulp / (2 * h), (i, grad, acc[i])
    assert checked >= 12


# 6. Paths agree
def test_replicas_against_no_replicas_and_reproducible(nb, ctx):
    ic = nb.ic.plummer(6000, seed=21)
    d, _ = to_device(nb, ic)
    t = _tree(nb, d, 2)
    t.tuning(1, 0)
    plain = _forces(t, d, 0.6, 1.0, 0.02)
    for replicas, level in ((2, 1), (4, 2), (16, 3), (0, 0)):
        t.tuning(replicas, level)
        a = _forces(t, d, 0.6, 1.0, 0.02)
        assert rel_err(a, plain).max() < 5e-6, (replicas, level)
        assert np.array_equal(_forces(t, d, 0.6, 1.0, 0.02), a)


def test_walk_forms_and_ranges_are_bitwise_equal(nb, ctx):
    import ctypes as C
    from nbody_amd._lib import check
    n = 300000
    ic = nb.ic.two_galaxies(n, seed=4)
    d, _ = to_device(nb, ic)
    t = _tree(nb, d, 2)
    ref = _forces(t, d, 0.5, 1.0, 0.05)
    for form in (0, 1, 2, 3, 2):
        t.walkForm(form)
        t.build(d)
        assert np.array_equal(_forces(t, d, 0.5, 1.0, 0.05), ref), form
    # disjoint compute_forces_packed ranges of a packed build equal the whole walk bit for bit
    lib = ctx._lib
    h = C.c_void_p()
    check(lib.nbody_hip_tree_create(ctx.handle, n, C.byref(h)))
    try:
        check(lib.nbody_hip_tree_set_multipole_order(h, 2))
        check(lib.nbody_hip_tree_build_packed(h, packed(ic).data_ptr(), n))
        out = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
        for lo, hi in ((0, n // 2), (n // 2, n)):
            check(lib.nbody_hip_tree_compute_forces_packed(h, lo, hi - lo, 0.5, 1.0, 0.05, out.data_ptr()))
        assert np.array_equal(out.cpu().numpy()[:, :3].astype(np.float64), ref)
    finally:
        lib.nbody_hip_tree_destroy(h)


def _state(d):
    return {k: getattr(d, k).cpu().numpy().copy() for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z",
                                                              "acc_x", "acc_y", "acc_z")}


@pytest.mark.parametrize("n", [8192, 131072])
def test_integrate_paths_agree(nb, ctx, n):
    ic = nb.ic.two_galaxies(n, seed=6)
    runs = {}
    for mode in ("fused", "generic", "graph", "eager"):
        d, _ = to_device(nb, ic)
        c = nb.BarnesHutCalculator(0.5)
        c.setSofteningParameter(0.05)
        c.setMultipoleOrder(2)
        integ = nb.Integrator()
        c.computeForces(d)
        if mode in ("fused", "generic"):
            for _ in range(20):
                if mode == "fused":
                    integ.integrate(d, c, 1e-3)
                else:  # the generic sequence: drift, then the calculator's own computeForces
                    from nbody_amd._lib import check
                    import ctypes as C
                    s = d.struct()
                    check(integ.ctx._lib.nbody_hip_drift(integ.ctx.handle, C.byref(s), 1e-3))
                    c.computeForces(d)
                    integ.updateVelocities(d, 1e-3)
        else:  # across an order switch: 10 steps at order 2, 10 at order 1, 10 at order 2
            for order in (2, 1, 2):
                c.setMultipoleOrder(order)
                integ.integrate_steps(d, c, 1e-3, 10, graph=(mode == "graph"))
        torch.cuda.synchronize()
        runs[mode] = _state(d)
    for k in runs["fused"]:
        assert np.array_equal(runs["fused"][k], runs["generic"][k]), k
        assert np.array_equal(runs["graph"][k], runs["eager"][k]), k


# 7. Order 1 untouched
def test_order_one_untouched(nb, ctx):
    for n in (5000, 150000):
        ic = nb.ic.two_galaxies(n, seed=8)
        d, _ = to_device(nb, ic)
        got = []
        for mode in ("never", "explicit", "switched"):
            t = nb.BarnesHutTree(n)
            if mode == "explicit":
                t.setMultipoleOrder(1)
            if mode == "switched":
                t.setMultipoleOrder(2)
                t.build(d)
                t.computeForces(d, 0.5, 1.0, 0.05)
                t.setMultipoleOrder(1)
            t.build(d)
            a = _forces(t, d, 0.5, 1.0, 0.05)
            phi, pe = _phi(t, d, 0.5, 1.0, 0.05)
            got.append((a, phi, pe))
            assert t.getMultipoleOrder() == 1
        for a, phi, pe in got[1:]:
            assert np.array_equal(a, got[0][0]) and np.array_equal(phi, got[0][1]) and pe == got[0][2]


# 8. Errors
def test_errors(nb, ctx):
    ic = nb.ic.plummer(1000, seed=2)
    d, _ = to_device(nb, ic)
    t = nb.BarnesHutTree(1000)
    assert t.getMultipoleOrder() == 1
    for bad in (0, 3, -1):
        with pytest.raises(nb.ValidationException):
            t.setMultipoleOrder(bad)
    t.build(d)
    t.setMultipoleOrder(2)
    assert t.getMultipoleOrder() == 2
    with pytest.raises(nb.StateException):
        t.computeForces(d, 0.5, 1.0, 0.1)
    with pytest.raises(nb.StateException):
        t.computePotential(d, 0.5, 1.0, 0.1)
    with pytest.raises(nb.StateException):
        t.copyMomentsToHost()
    t.build(d)
    t.computeForces(d, 0.5, 1.0, 0.1)
    nodes = t.getNodeCount()
    out = np.zeros((nodes, 6), np.float32)
    from nbody_amd._lib import check
    with pytest.raises(nb.ValidationException):
        check(t.ctx._lib.nbody_hip_tree_copy_moments(t._h, out.ctypes.data, nodes - 1))
    check(t.ctx._lib.nbody_hip_tree_copy_moments(t._h, out.ctypes.data, nodes))
    assert np.array_equal(out, t.copyMomentsToHost())


# 9. ParticleSystem and the facade
def test_particle_system_order(nb, ctx):
    n = 4096
    ic = nb.ic.two_galaxies(n, seed=4)
    cfg = nb.SimulationConfig(particle_count=n, force_method=nb.ForceMethod.BARNES_HUT, G=1.0, softening=0.05,
                              barnes_hut_theta=0.6)
    ps = nb.ParticleSystem()
    ps.setBarnesHutMultipoleOrder(2)
    ps.initialize(cfg)
    ps.setForceMethod(nb.ForceMethod.DIRECT_N2)
    ps.setForceMethod(nb.ForceMethod.BARNES_HUT)
    ps.reset()  # (re-initialises with the built-in distribution)
    assert ps.getBarnesHutMultipoleOrder() == 2 and ps.force_calculator_.getMultipoleOrder() == 2
    ps.initialize(cfg, initial_conditions=ic)
    assert ps.force_calculator_.getMultipoleOrder() == 2
    ps.update(1e-3)
    got = _state(ps.getDeviceData())
    pe = ps.computeMethodPotentialEnergy()
    d, _ = to_device(nb, ic)
    c = nb.BarnesHutCalculator(0.6)
    c.setSofteningParameter(0.05)
    c.setMultipoleOrder(2)
    c.computeForces(d)
    nb.Integrator().integrate(d, c, 1e-3)
    want = _state(d)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    assert pe == c.computePotential(d)
    assert ps.force_calculator_.getTree().getMultipoleOrder() == 2


def test_facade_quadrupole_program(nb, ctx, tmp_path):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "quadrupole_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    out = str(tmp_path / "quad.bin")
    r = subprocess.run([exe, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    f = np.frombuffer(raw[8:8 + 28 * n], np.float32).reshape(7, n)
    pe_facade = float(np.frombuffer(raw[8 + 28 * n:], np.float64)[0])
    ic = {"pos_x": f[0].copy(), "pos_y": f[1].copy(), "pos_z": f[2].copy(), "mass": f[3].copy()}
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k] = np.zeros(n, np.float32)
    d, _ = to_device(nb, ic)
    c = nb.BarnesHutCalculator(0.5)
    c.setSofteningParameter(0.1)
    c.setMultipoleOrder(2)
    c.computeForces(d)
    assert np.array_equal(acc_of(d), f[4:7].T)
    assert c.computePotential(d) == pe_facade
