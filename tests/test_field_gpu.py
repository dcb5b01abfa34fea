"""Acceleration and potential at arbitrary points (nbody_hip_{direct,tree,grid}_field) on a real GPU: against fp64, against
the methods' own forces and potentials at the bodies' positions, against the restatement over the exported tree,
accuracy at config-4 size, the grid against brute force, bitwise invariance, non-interference with the integration,
gradients, errors and the facade.  Restatements: tests/field_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import field_ref as fr
import quadrupole_ref as qr
from gpu_util import U, acc_of, assert_hash_parity, rel_err, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")

# ---- the a-priori bound of the Direct field against fp64 (the pattern of tests/gpu_util.py) ---------------------------
# err_i <= max(1e-5 |a_i|, C u S_i), S_i = G sum_j m_j |d| (d^2 + eps^2)^-3/2 the sum of the term magnitudes, u = 2^-24.
# Per term (relative to |t_ij|, first order in u), csrc/direct.hip direct_field_kernel against the fp64 formula on the
# same fp32 inputs:
#   d = fl(r_j - x): 1u on the direction, and <= 2u on d^2 -> 3u on (d^2 + eps^2)^-3/2
#   d^2 + eps^2 by three fused multiply-adds: <= 3u on the sum -> 4.5u on its -3/2 power
#   v_rsq_f32 (<= 1 ulp = 2u), cubed -> 6u; the three roundings of (m inv) (inv inv) -> 3u          => C_TERMS = 17.5 -> 18
# Accumulation: a term enters its fp32 tile sum through an FMA and passes at most TS = 256 roundings (the tile of the
# kernel; constexpr TS in direct.hip) before the fold into fp64; the split sums are rounded to fp32 once more (1).  A
# component's error is <= (TS + 1) u sum |t_x| <= (TS + 1) u S; three components -> sqrt(3).  The final rounding: 1.
#   C_DIRECT = 18 + sqrt(3) (256 + 1) + 1 = 464.2
# The tree walk keeps one fp32 sum per sibling group (<= 8 one-body leaves at theta = 0) and no fp32 split sums:
#   C_TREE = 18 + sqrt(3) 8 + 1 = 32.9
# Worst cases, every rounding at its limit with the same sign; nothing here is fitted to the data.
TS = 256
C_TERMS = 18
C_DIRECT = C_TERMS + np.sqrt(3.0) * (TS + 1) + 1
C_TREE = C_TERMS + np.sqrt(3.0) * 8 + 1
# Regression tier of test 1, MEASURED on an MI355X, not derived: the margin max err / (u S) over the 20,480 points of
# test_direct_field_against_fp64 was 10.53 (forty times inside the worst case; max |da| / |a| 5.07e-6); 1.6 x that is held.
DIRECT_MARGIN_MEASURED = 10.53


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, {k: z[k] for k in KEYS}


def _pos(ic):
    return np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)


def _calc(nb, kind, G=1.0, eps=0.1, theta=0.5, cell=1.0, cutoff=1.0, order=1):
    c = {"direct": lambda: nb.DirectForceCalculator(), "bh": lambda: nb.BarnesHutCalculator(theta),
         "hash": lambda: nb.SpatialHashCalculator(cell, cutoff)}[kind]()
    c.setGravitationalConstant(G)
    c.setSofteningParameter(eps)
    if kind == "bh" and order != 1:
        c.setMultipoleOrder(order)
    return c


def _dev(points):
    return torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()


def _field(fn, points):
    """fn(device points) -> [M, 4] tensor; returns (a (M, 3), phi (M,)) as float64 numpy"""
    out = fn(_dev(points)).cpu().numpy().astype(np.float64)
    return out[:, :3], out[:, 3]


def _direct_ref(points, pos, m, G, eps, chunk=2048):
    """fr.direct_field in fp64 on the device (the big comparisons): (a, phi, S)"""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])).cuda().double()
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float32)).cuda().double()
    mm = torch.from_numpy(np.asarray(m, np.float64)).cuda()
    e2 = float(np.float32(eps) * np.float32(eps))
    acc, phi, S = [], [], []
    for a in range(0, len(x), chunk):
        d = p[None, :, :] - x[a:a + chunk, None, :]
        r2 = (d * d).sum(-1)
        ok = (r2 > 0) if e2 < 1e-12 else torch.ones_like(r2, dtype=torch.bool)
        inv = torch.where(ok, torch.rsqrt(torch.where(ok, r2 + e2, torch.ones_like(r2))), torch.zeros_like(r2))
        f = mm[None, :] * inv ** 3
        acc.append(G * (f[:, :, None] * d).sum(1))
        phi.append(-G * (mm[None, :] * inv).sum(1))
        S.append(G * (f * r2.sqrt()).sum(1))
    return torch.cat(acc).cpu().numpy(), torch.cat(phi).cpu().numpy(), torch.cat(S).cpu().numpy()


def _shell_points(rng, count, centre, r_lo, r_hi):
    """isotropic directions, radii log-uniform in [r_lo, r_hi] about `centre`"""
    v = rng.normal(size=(count, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    r = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), count))
    return (np.asarray(centre)[None, :] + v * r[:, None]).astype(np.float32)


def _vector_bound_check(tag, a, a_ref, S, C):
    err = np.linalg.norm(a - a_ref, axis=1)
    bound = np.maximum(1e-5 * np.linalg.norm(a_ref, axis=1), C * U * S)
    margin = float((err / np.maximum(U * S, 1e-300)).max())
    worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"{tag}: max |da| / |a| {rel_err(a, a_ref).max():.3e}, margin max err / (u S) {margin:.2f} (C = {C:.1f}), worst "
          f"err / bound {err[worst] / bound[worst]:.3e}", flush=True)
    assert np.all(err <= bound), (tag, worst, err[worst], bound[worst])
    return margin


# 1. Direct against fp64
def test_direct_field_against_fp64(nb, ctx):
    z, ic = _fixture("plummer4096_direct")
    G, eps = float(z["G"]), float(z["eps"])
    pos, m = _pos(ic), ic["mass"]
    com = (m[:, None].astype(np.float64) * pos).sum(0) / m.sum()
    r_half = float(np.median(np.linalg.norm(pos - com, axis=1)))
    pts = np.concatenate([_shell_points(np.random.default_rng(21), 16384, com, 0.01 * r_half, 10.0 * r_half), pos])
    d, _ = to_device(nb, ic)
    c = _calc(nb, "direct", G, eps)
    a, phi = _field(lambda p: c.computeField(d, p), pts)
    a_ref, phi_ref, S = fr.direct_field(pts, pos, m, G, eps)
    # (the device fp64 reference of the larger tests is the same restatement)
    a_t, phi_t, S_t = _direct_ref(pts, pos, m, G, eps)
    assert np.allclose(a_t, a_ref, rtol=1e-11, atol=1e-11 * S.max()) and np.allclose(phi_t, phi_ref, rtol=1e-12)
    assert np.allclose(S_t, S, rtol=1e-11)
    ephi = np.abs(phi - phi_ref) / np.abs(phi_ref)
    print(f"direct field, {len(pts)} points: max |dphi| / |phi| {ephi.max():.3e}")
    assert ephi.max() <= 1e-5
    margin = _vector_bound_check("direct field against fp64", a, a_ref, S, C_DIRECT)
    assert margin <= 1.6 * DIRECT_MARGIN_MEASURED, (margin, DIRECT_MARGIN_MEASURED)
    # a point on a body: that body adds no force and -G m / eps to phi (the reference above says the same)
    assert np.isfinite(a[16384:]).all() and np.isfinite(phi[16384:]).all()


# 2. A point on a body is that body minus itself
def _forces(c, d):
    c.computeForces(d)
    return acc_of(d).astype(np.float64)


def _phi_of(c, d):
    phi = torch.empty(d.count, dtype=torch.float32, device="cuda")
    c.computePotential(d, phi)
    return phi.cpu().numpy().astype(np.float64)


def test_direct_field_on_the_bodies(nb, ctx):
    z, ic = _fixture("plummer4096_direct")
    G, eps = float(z["G"]), float(z["eps"])
    d, _ = to_device(nb, ic)
    c = _calc(nb, "direct", G, eps)
    a, phi = _field(lambda p: c.computeField(d, p), _pos(ic))
    e = rel_err(a, _forces(c, d))
    self_term = G * ic["mass"].astype(np.float64) / float(np.float32(eps))
    ephi = np.abs(phi + self_term - _phi_of(c, d)) / np.abs(phi)  # |phi| = the sum of the term magnitudes, self included
    print(f"direct field on the bodies: force max rel {e.max():.3e}, phi + G m / eps against phi_i, of scale {ephi.max():.3e}")
    assert e.max() <= 1e-5 and ephi.max() <= 1e-5


@pytest.mark.parametrize("order", [1, 2])
def test_tree_field_on_the_bodies(nb, ctx, order):
    z, ic = _fixture("twogalaxies2048_barnes_hut")
    G, eps, theta = float(z["G"]), float(z["eps"]), float(z["theta"])
    d, _ = to_device(nb, ic)
    c = _calc(nb, "bh", G, eps, theta=theta, order=order)
    a, phi = _field(lambda p: c.computeField(d, p), _pos(ic))
    e = rel_err(a, _forces(c, d))
    self_term = G * ic["mass"].astype(np.float64) / float(np.float32(eps))
    ephi = np.abs(phi + self_term - _phi_of(c, d)) / np.abs(phi)
    print(f"tree field on the bodies, order {order}: force max rel {e.max():.3e}, phi of scale {ephi.max():.3e}")
    assert e.max() <= 1e-5 and ephi.max() <= 1e-5


@pytest.mark.parametrize("cutoff_cells", [1.0, 2.0])
def test_grid_field_on_the_bodies(nb, ctx, cutoff_cells):
    z, ic = _fixture("uniform4096_spatial_hash")
    G, eps, cell = float(z["G"]), float(z["eps"]), float(z["cell"])
    cutoff = cutoff_cells * cell
    pos, m = _pos(ic), ic["mass"]
    d, _ = to_device(nb, ic)
    c = _calc(nb, "hash", G, eps, cell=cell, cutoff=cutoff)
    a_f = _forces(c, d)
    phi_b = _phi_of(c, d)
    a, phi = _field(lambda p: c.computeField(d, p), pos)
    # the bodies' own cells define the window (for cutoff > cell it is not the sum over all bodies)
    _, _, cell_of, _ = c.getGrid().copyCellDataToHost()
    dims = c.getGrid().getGridDims()
    a_ref, phi_ref, S, scale = fr.hash_field(pos, cell_of, pos, m, G, eps, cutoff, cell_of, dims)
    nz = np.linalg.norm(a_ref, axis=1) > 0
    assert not a[~nz].any() and not a_f[~nz].any()
    assert_hash_parity(f"grid field on the bodies against computeForces, cutoff {cutoff}", rel_err(a[nz], a_f[nz]),
                       S[nz] / np.linalg.norm(a_ref[nz], axis=1), kind="gpu", n_total=len(m))
    assert_hash_parity(f"grid field on the bodies against fp64, cutoff {cutoff}", rel_err(a[nz], a_ref[nz]),
                       S[nz] / np.linalg.norm(a_ref[nz], axis=1), kind="gold", n_total=len(m))
    e2, rc2 = float(np.float32(eps) ** 2), float(np.float32(cutoff) * np.float32(cutoff))
    self_term = G * m.astype(np.float64) * (1.0 / np.sqrt(e2) - 1.0 / np.sqrt(rc2 + e2))  # the shifted term at r = 0
    ephi = np.abs(phi + self_term - phi_b) / scale
    print(f"grid field on the bodies, cutoff {cutoff}: phi + self term against phi_i, of scale {ephi.max():.3e}; against "
          f"fp64 {(np.abs(phi - phi_ref) / scale).max():.3e}")
    assert ephi.max() <= 1e-5 and (np.abs(phi - phi_ref) / scale).max() <= 1e-5


# 3. Tree at theta = 0: the Direct field in another order
@pytest.mark.parametrize("which", ["twogalaxies2048", "plummer65536"])
def test_tree_field_theta0_is_the_direct_field(nb, ctx, which):
    if which == "twogalaxies2048":
        z, ic = _fixture("twogalaxies2048_barnes_hut")
        G, eps = float(z["G"]), float(z["eps"])
    else:
        ic, G, eps = nb.ic.plummer(65536, seed=7), 1.0, 0.01
    pos, m = _pos(ic), ic["mass"]
    lo, hi = pos.min(0), pos.max(0)
    centre, half = 0.5 * (lo + hi), 0.5 * float((hi - lo).max())
    rng = np.random.default_rng(31)
    pts = np.concatenate([rng.uniform(lo, hi, (12288, 3)).astype(np.float32),                # inside the box
                          _shell_points(rng, 2048, centre, 2.0 * half, 6.0 * half),         # outside the root cube
                          pos[rng.choice(len(m), 2048, replace=False)]])                    # on bodies
    assert len(pts) == 16384
    d, _ = to_device(nb, ic)
    a_d, phi_d = _field(lambda p: _calc(nb, "direct", G, eps).computeField(d, p), pts)
    a_ref, phi_ref, S = _direct_ref(pts, pos, m, G, eps)
    for order in (1, 2):
        a_t, phi_t = _field(lambda p: _calc(nb, "bh", G, eps, theta=0.0, order=order).computeField(d, p), pts)
        # both sides are fp32 evaluations of the same sum: the two a-priori constants add
        err = np.linalg.norm(a_t - a_d, axis=1)
        bound = np.maximum(1e-5 * np.linalg.norm(a_ref, axis=1), (C_DIRECT + C_TREE) * U * S)
        ephi = np.abs(phi_t - phi_d) / np.abs(phi_ref)
        print(f"{which} order {order}: tree field (theta 0) against the Direct field: max |da| / |a| "
              f"{rel_err(a_t, a_d).max():.3e}, margin max err / (u S) {(err / (U * S)).max():.2f}, phi {ephi.max():.3e}")
        assert np.all(err <= bound), int(np.argmax(err / bound))
        assert ephi.max() <= 1e-5
        _vector_bound_check(f"{which} order {order}: tree field (theta 0) against fp64", a_t, a_ref, S, C_TREE)


# 4. Tree against the restatement over the exported tree: pins the interaction list
@pytest.mark.parametrize("order", [1, 2])
def test_tree_field_against_the_restatement(nb, ctx, order):
    z, ic = _fixture("twogalaxies2048_barnes_hut")
    G, eps, theta = float(z["G"]), float(z["eps"]), 0.5
    pos, m = _pos(ic), ic["mass"]
    d, _ = to_device(nb, ic)
    t = nb.BarnesHutTree(d.count)
    t.setMultipoleOrder(order)
    t.build(d)
    lo, hi = pos.min(0), pos.max(0)
    rng = np.random.default_rng(41)
    pts = np.concatenate([rng.uniform(lo, hi, (3072, 3)).astype(np.float32),
                          _shell_points(rng, 512, 0.5 * (lo + hi), 0.6 * float((hi - lo).max()), 4.0 * float((hi - lo).max())),
                          pos[rng.choice(len(m), 512, replace=False)]])
    a, phi = _field(lambda p: t.computeField(p, theta, G, eps), pts)
    rest = qr.Restatement(t.copyNodesToHost(), t.sorted_indices_, pos, m)
    if order == 2:  # the exported moments are the ones the walk uses: they agree with the bodies' (test_bh_quadrupole_gpu)
        assert t.copyMomentsToHost().shape == (len(rest.M), 6)
    a_ref, phi_ref, S = fr.tree_field(rest, pts, theta, G, eps, order)
    ea = np.linalg.norm(a - a_ref, axis=1) / S
    ephi = np.abs(phi - phi_ref) / np.abs(phi_ref)
    print(f"tree field against the restatement, order {order}: |da| / S max {ea.max():.3e}, |dphi| / |phi| max {ephi.max():.3e}")
    assert ea.max() <= 1e-5, int(np.argmax(ea))
    assert ephi.max() <= 1e-5, int(np.argmax(ephi))


# 5. Tree accuracy at config 4 (two galaxies, 2^20 bodies, eps = 0.1): a 512 x 512 raster in the orbital plane and 2^16
# random points, against the Direct field.  Three tiers: the orderings below hold unconditionally; 1.6 x the values
# MEASURED on an MI355X (FIELD_MEASURED: {(theta, order): (rms |da| / |a|, max |da| / |a|, rms |dphi| / |phi|,
# max |dphi| / |phi|)} -- the maxima of |da| / |a| belong to the few points between the galaxies where the field nearly
# vanishes); the ceiling 3e-2 of tests/test_potential_gpu.py for max |dphi| / |phi| at theta 0.5, order 1.
FIELD_MEASURED = {
    (0.3, 1): (4.7791e-03, 9.4606e-02, 1.5389e-03, 2.2646e-03), (0.3, 2): (2.2729e-04, 3.6250e-02, 1.1231e-05, 2.9190e-05),
    (0.5, 1): (1.5672e-02, 8.6440e-01, 4.3529e-03, 6.5918e-03), (0.5, 2): (1.6194e-03, 1.3211e-01, 8.3669e-05, 2.7600e-04),
    (0.8, 1): (5.2495e-02, 2.5516e+00, 1.1452e-02, 2.0704e-02), (0.8, 2): (1.1205e-02, 6.0130e-01, 5.9473e-04, 2.0250e-03),
}
FIELD_CEIL_PHI_MAX = 3e-2


def test_tree_field_accuracy_config4(nb, ctx):
    n, G, eps = 1 << 20, 1.0, 0.1
    ic = nb.ic.two_galaxies(n, seed=42)
    pos = _pos(ic)
    lo, hi = pos.min(0), pos.max(0)
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 512), np.linspace(lo[1], hi[1], 512), indexing="ij")
    raster = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1).astype(np.float32)
    pts = np.concatenate([raster, np.random.default_rng(51).uniform(lo, hi, (1 << 16, 3)).astype(np.float32)])
    d, _ = to_device(nb, ic)
    p_dev = _dev(pts)
    ref = _calc(nb, "direct", G, eps).computeField(d, p_dev).cpu().numpy().astype(np.float64)
    na, nphi = np.linalg.norm(ref[:, :3], axis=1), np.abs(ref[:, 3])
    stats = {}
    for order in (1, 2):
        t = nb.BarnesHutTree(n)
        t.setMultipoleOrder(order)
        t.build(d)
        for theta in (0.3, 0.5, 0.8):
            out = t.computeField(p_dev, theta, G, eps).cpu().numpy().astype(np.float64)
            ea = np.linalg.norm(out[:, :3] - ref[:, :3], axis=1) / na
            ep = np.abs(out[:, 3] - ref[:, 3]) / nphi
            stats[(theta, order)] = (float(np.sqrt((ea * ea).mean())), float(ea.max()), float(np.sqrt((ep * ep).mean())),
                                     float(ep.max()))
            print(f"config 4 field, theta {theta} order {order}: |da| / |a| rms {stats[(theta, order)][0]:.4e} max "
                  f"{stats[(theta, order)][1]:.4e}; |dphi| / |phi| rms {stats[(theta, order)][2]:.4e} max "
                  f"{stats[(theta, order)][3]:.4e}", flush=True)
    for theta in (0.3, 0.5, 0.8):  # order 2 is the better model at equal theta
        assert stats[(theta, 2)][0] < stats[(theta, 1)][0] and stats[(theta, 2)][2] < stats[(theta, 1)][2], theta
    for order in (1, 2):  # ref: tests/test_barnes_hut.cpp:131-201 -- a smaller opening angle is not less accurate
        assert stats[(0.3, order)][0] <= 1.1 * stats[(0.8, order)][0]
        assert stats[(0.3, order)][2] <= 1.1 * stats[(0.8, order)][2]
    assert stats[(0.5, 1)][3] <= FIELD_CEIL_PHI_MAX
    for key, got in stats.items():
        for g, want in zip(got, FIELD_MEASURED[key]):
            assert g <= 1.6 * want, (key, got, FIELD_MEASURED[key])


# 6. Grid against brute force: cutoff = cell, so the window is the truncated sum over all bodies wherever the point lies
def test_grid_field_against_brute_force(nb, ctx):
    z, ic = _fixture("uniform4096_spatial_hash")
    G, eps, cell = float(z["G"]), float(z["eps"]), float(z["cell"])
    cutoff = cell
    pos, m = _pos(ic), ic["mass"]
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    rng = np.random.default_rng(61)

    def outside(count, d_lo, d_hi):
        """points whose distance to the box is in [d_lo, d_hi): pushed out along one axis"""
        p = rng.uniform(lo, hi, (count, 3))
        ax, up = rng.integers(0, 3, count), rng.random(count) < 0.5
        dist = rng.uniform(d_lo, d_hi, count)
        p[np.arange(count), ax] = np.where(up, hi[ax] + dist, lo[ax] - dist)
        return p

    near, far = outside(1024, 0.0, cutoff), outside(1024, 1.05 * cutoff, 40.0 * cutoff)
    pts = np.concatenate([rng.uniform(lo, hi, (8192, 3)), near, far]).astype(np.float32)
    d, _ = to_device(nb, ic)
    g = nb.SpatialHashGrid(d.count, cell)
    g.build(d)
    out = g.computeField(_dev(pts), cutoff, G, eps).cpu().numpy()
    assert not out[9216:].any(), "points further than the cutoff from the box must get exact zeros"
    a, phi = out[:, :3].astype(np.float64), out[:, 3].astype(np.float64)
    a_ref, phi_ref, S, scale = fr.hash_field_all(pts, pos, m, G, eps, cutoff)
    nz = np.linalg.norm(a_ref, axis=1) > 0
    assert not a[~nz].any() and not phi[~nz].any()  # no pair inside the cutoff: exact zeros, inside the box too
    assert nz[:8192].sum() > 7000 and nz[8192:9216].sum() > 100
    assert_hash_parity("grid field against brute force", rel_err(a[nz], a_ref[nz]),
                       S[nz] / np.linalg.norm(a_ref[nz], axis=1), kind="gold", n_total=len(pts))
    ephi = np.abs(phi[nz] - phi_ref[nz]) / scale[nz]
    print(f"grid field against brute force: |dphi| / scale max {ephi.max():.3e}")
    assert ephi.max() <= 1e-5


# 7. Bitwise: permutations, splits, repeats
def _chunks(rng, count, k):
    cuts = np.sort(rng.choice(np.arange(1, count), k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    return list(zip(np.concatenate([[0], cuts]).astype(int), np.concatenate([cuts, [count]]).astype(int)))


def test_field_rows_are_functions_of_their_points(nb, ctx):
    ic = nb.ic.plummer(65536, seed=11)
    d, _ = to_device(nb, ic)
    pos = _pos(ic)
    rng = np.random.default_rng(71)
    pts = np.concatenate([rng.uniform(-3, 3, (20000, 3)), pos[:3000] + rng.normal(0, 1e-3, (3000, 3)),
                          pos[3000:3500]]).astype(np.float32)
    perm = rng.permutation(len(pts))
    p_dev, q_dev = _dev(pts), _dev(pts[perm])
    def bitwise(name, fn, splits=True):
        ref = fn(p_dev).cpu().numpy()
        assert np.isfinite(ref).all() and ref[:, 3].max() <= 0 and ref[:, 3].min() < 0, name
        assert np.array_equal(fn(p_dev).cpu().numpy(), ref), name                      # call to call
        assert np.array_equal(fn(q_dev).cpu().numpy(), ref[perm]), name                # permutation
        for k in (1, 3, 64) if splits else ():
            got = np.concatenate([fn(p_dev[a:b]).cpu().numpy() for a, b in _chunks(rng, len(pts), k)])
            assert np.array_equal(got, ref), (name, k)

    direct = _calc(nb, "direct", 1.0, 0.01)
    bitwise("direct", lambda p: direct.computeField(d, p), splits=False)  # (its source splits follow the point count)
    grid = nb.SpatialHashGrid(d.count, 0.5)
    grid.build(d)
    bitwise("grid", lambda p: grid.computeField(p, 2.0, 1.0, 0.01))  # (cutoff 2: every point of the cloud has partners)
    tree = nb.BarnesHutTree(d.count)
    for order in (1, 2):
        tree.setMultipoleOrder(order)
        tree.build(d)
        bitwise(f"tree order {order}", lambda p: tree.computeField(p, 0.5, 1.0, 0.01))


# 8. Non-interference: 20 steps with a field call after every step against the same 20 steps without
def _state(d):
    return {k: getattr(d, k).cpu().numpy().copy() for k in
            ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z")}


@pytest.mark.parametrize("kind,n", [("bh", 131072), ("bh", 4096), ("hash", 65536)])
def test_field_calls_do_not_change_the_integration(nb, ctx, kind, n):
    # bh at 131,072 bodies: above the size from which the pair walk runs the cost-ordered schedule of the previous walk
    ic = nb.ic.two_galaxies(n, seed=3) if kind == "bh" else nb.ic.plummer(n, seed=3)
    pts = _dev(np.random.default_rng(81).uniform(-5, 5, (5000, 3)))
    runs = []
    for with_field in (False, True):
        d, _ = to_device(nb, ic)
        c = _calc(nb, kind, 1.0, 0.01, cell=0.5, cutoff=0.5)
        integ = nb.Integrator()
        c.computeForces(d)
        for _ in range(20):
            integ.integrate(d, c, 1e-3)
            if with_field:
                c.computeField(d, pts)
                if kind == "bh":
                    c.getTree().computeField(pts, 0.5, 1.0, 0.01)
                if kind == "hash":
                    c.getGrid().computeField(pts, 0.5, 1.0, 0.01)
        torch.cuda.synchronize()
        runs.append(_state(d))
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


# 9. Gradient: central differences of the field's own phi, h = 1e-3
def _gradient_setup(cutoff, half=2.0, rmin=0.2):
    """64 bodies and 64 points in a box of side 2 half: no point within rmin of a body, no point-body distance within
    3e-3 of the cutoff (a pair must not enter or leave the sum between x - h and x + h)"""
    rng = np.random.default_rng(91)
    bodies = rng.uniform(-half, half, (64, 3)).astype(np.float32)
    pts = []
    while len(pts) < 64:
        p = rng.uniform(-half, half, 3).astype(np.float32)
        r = np.linalg.norm(bodies.astype(np.float64) - p, axis=1)
        if r.min() > rmin and np.abs(r - cutoff).min() > 3e-3:
            pts.append(p)
    return bodies, np.array(pts, np.float32)


def _gradient_check(tag, fn, pts, h=1e-3):
    stencil = [pts]
    for ax in range(3):
        for s in (+1, -1):
            q = pts.copy()
            q[:, ax] = (q[:, ax] + np.float32(s * h)).astype(np.float32)
            stencil.append(q)
    a, phi = _field(fn, np.concatenate(stencil))
    k = len(pts)
    worst = 0.0
    for i in range(k):
        grad, ulp = np.zeros(3), 0.0
        for ax in range(3):
            ip, im = (1 + 2 * ax) * k + i, (2 + 2 * ax) * k + i
            dx = float(stencil[1 + 2 * ax][i, ax]) - float(stencil[2 + 2 * ax][i, ax])
            grad[ax] = (phi[ip] - phi[im]) / dx
            # phi is rounded to fp32 once: each difference quotient carries up to ulp(phi) / 2h
            ulp = max(ulp, float(np.spacing(np.float32(abs(phi[ip]) + abs(phi[im])))))
        e = np.linalg.norm(grad + a[i])
        worst = max(worst, e / np.linalg.norm(a[i]))
        assert e <= 1e-3 * np.linalg.norm(a[i]) + np.sqrt(3) * ulp / (2 * h), (tag, i, grad, a[i])
    print(f"{tag}: worst |grad phi + a| / |a| = {worst:.3e}")


def _bodies(nb, pos, m):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    ic = {"pos_x": pos[:, 0].copy(), "pos_y": pos[:, 1].copy(), "pos_z": pos[:, 2].copy(),
          "mass": np.asarray(m, np.float32)}
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k] = np.zeros(len(ic["mass"]), np.float32)
    return to_device(nb, ic)[0], ic


def test_gradient_of_the_field_phi_is_minus_its_a(nb, ctx):
    G, eps, cell, cutoff = 1.0, 0.01, 1.5, 1.5
    bodies, pts = _gradient_setup(cutoff)
    m = np.random.default_rng(5).uniform(0.5, 2.0, 64).astype(np.float32)
    d, _ = _bodies(nb, bodies, m)
    _gradient_check("direct", lambda p: _calc(nb, "direct", G, eps).computeField(d, p), pts)
    _gradient_check("hash", lambda p: _calc(nb, "hash", G, eps, cell=cell, cutoff=cutoff).computeField(d, p), pts)
    for order in (1, 2):  # theta = 0: every point's list is all the bodies
        _gradient_check(f"tree theta 0 order {order}",
                        lambda p: _calc(nb, "bh", G, eps, theta=0.0, order=order).computeField(d, p), pts)
    # accepted nodes: from 5 to 6 root half-sizes away the root cube is accepted at theta = 0.5 (2 half < 0.5 dist) at the
    # point and at its six neighbours alike, so phi and a are those of ONE node, multipoles included
    half = 0.5 * float((bodies.max(0) - bodies.min(0)).max()) + 0.001
    far = _shell_points(np.random.default_rng(92), 64, 0.5 * (bodies.max(0) + bodies.min(0)), 5.0 * half, 6.0 * half)
    for order in (1, 2):
        _gradient_check(f"tree theta 0.5 order {order}, root accepted",
                        lambda p: _calc(nb, "bh", G, eps, theta=0.5, order=order).computeField(d, p), far)


# 10. Errors and edges
def test_field_errors_and_edges(nb, ctx):
    lib = nb._lib.load()
    d, ic = _bodies(nb, np.random.default_rng(2).uniform(-1, 1, (100, 3)), np.ones(100))
    pts = _dev(np.random.default_rng(3).uniform(-1.5, 1.5, (65, 3)))
    p4 = torch.nn.functional.pad(pts, (0, 1)).contiguous()
    out = torch.empty((65, 4), dtype=torch.float32, device="cuda")
    tree, grid = nb.BarnesHutTree(100), nb.SpatialHashGrid(100, 0.5)
    direct = _calc(nb, "direct", 1.0, 0.1)
    # not built
    with pytest.raises(nb.StateException):
        tree.computeField(pts, 0.5, 1.0, 0.1)
    with pytest.raises(nb.StateException):
        grid.computeField(pts, 0.5, 1.0, 0.1)
    tree.build(d)
    grid.build(d)
    # the order changed since the build
    tree.setMultipoleOrder(2)
    with pytest.raises(nb.StateException):
        tree.computeField(pts, 0.5, 1.0, 0.1)
    tree.setMultipoleOrder(1)
    # theta, cutoff
    for theta in (-0.1, 2.5, float("nan")):
        with pytest.raises(nb.ValidationException):
            tree.computeField(pts, theta, 1.0, 0.1)
    for cutoff in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(nb.ValidationException):
            grid.computeField(pts, cutoff, 1.0, 0.1)
    # null points / out (the C ABI; the Python layer never passes one)
    s = d.struct()
    import ctypes as C
    V, R = nb._lib.ERR_VALIDATION, nb._lib.ERR_RESOURCE
    assert lib.nbody_hip_direct_field(ctx.handle, C.byref(s), None, 65, 1.0, 0.1, out.data_ptr()) == V
    assert lib.nbody_hip_direct_field(ctx.handle, C.byref(s), p4.data_ptr(), 65, 1.0, 0.1, None) == V
    assert lib.nbody_hip_tree_field(tree._h, None, 65, 0.5, 1.0, 0.1, out.data_ptr()) == V
    assert lib.nbody_hip_tree_field(tree._h, p4.data_ptr(), 65, 0.5, 1.0, 0.1, None) == V
    assert lib.nbody_hip_grid_field(grid._h, None, 65, 0.5, 1.0, 0.1, out.data_ptr()) == V
    assert lib.nbody_hip_grid_field(grid._h, p4.data_ptr(), 65, 0.5, 1.0, 0.1, None) == V
    # more points than the kernels index: refused before anything is touched
    big = (1 << 30) + 1
    assert lib.nbody_hip_direct_field(ctx.handle, C.byref(s), p4.data_ptr(), big, 1.0, 0.1, out.data_ptr()) == R
    assert lib.nbody_hip_tree_field(tree._h, p4.data_ptr(), big, 0.5, 1.0, 0.1, out.data_ptr()) == R
    assert lib.nbody_hip_grid_field(grid._h, p4.data_ptr(), big, 0.5, 1.0, 0.1, out.data_ptr()) == R
    # the Python layer's argument checks
    for bad in (pts.double(), pts.cpu(), pts[:, :2], pts.reshape(-1)):
        with pytest.raises(nb.ValidationException):
            direct.computeField(d, bad)
    with pytest.raises(nb.ValidationException):
        direct.computeField(d, pts, torch.empty((64, 4), dtype=torch.float32, device="cuda"))
    # not capturable
    with pytest.raises(nb.StateException):
        with ctx.capture():
            tree.computeField(pts, 0.5, 1.0, 0.1)
    calls = {"direct": lambda p, o=None: direct.computeField(d, p, o), "tree": lambda p, o=None: tree.computeField(p, 0.5, 1.0, 0.1, o),
             "grid": lambda p, o=None: grid.computeField(p, 0.5, 1.0, 0.1, o)}
    for name, fn in calls.items():
        # no points: succeeds, returns an empty [0, 4] tensor, touches nothing
        assert tuple(fn(pts[:0]).shape) == (0, 4), name
        # 65 points (a ragged wave), [M, 3] and [M, 4] input, `out` filled in place
        full = fn(pts)
        assert full.shape == (65, 4) and torch.isfinite(full).all(), name
        got = fn(p4, out)
        assert got is out and torch.equal(out, full), name
        # a single point is the first row
        assert torch.equal(fn(pts[:1]), full[:1]), name
        # a non-finite point: its row alone is not finite
        q = pts.clone()
        q[7, 1] = float("nan")
        q[40, 0] = float("inf")
        bad = fn(q)
        keep = torch.ones(65, dtype=torch.bool, device="cuda")
        keep[[7, 40]] = False
        assert torch.equal(bad[keep], full[keep]) and not torch.isfinite(bad[~keep]).any(), name
    # eps = 0, a point on a body: finite, and the guard convention holds -- the coincident body contributes nothing
    on = _dev(_pos(ic)[:10])
    for name, kind in (("direct", "direct"), ("tree", "bh"), ("grid", "hash")):
        c0 = _calc(nb, kind, 1.0, 0.0, theta=0.0, cell=4.0, cutoff=4.0)  # (the hash: every body inside the cutoff)
        got = c0.computeField(d, on).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), name
        a_ref, phi_ref, S = fr.direct_field(_pos(ic)[:10], _pos(ic), ic["mass"], 1.0, 0.0)
        if kind == "hash":
            phi_ref = phi_ref + 1.0 * 99.0 / 4.0  # 99 partners, each shifted by 1 / cutoff
        assert np.all(np.linalg.norm(got[:, :3] - a_ref, axis=1) <= 1e-5 * S), name
        assert np.all(np.abs(got[:, 3] - phi_ref) <= 1e-5 * np.abs(phi_ref)), name


def test_particle_system_field(nb, ctx):
    n = 2048
    ic = nb.ic.plummer(n, seed=4)
    pts = np.random.default_rng(6).uniform(-2, 2, (1000, 3)).astype(np.float32)
    for method in (nb.ForceMethod.DIRECT_N2, nb.ForceMethod.BARNES_HUT, nb.ForceMethod.SPATIAL_HASH):
        ps = nb.ParticleSystem()
        ps.initialize(nb.SimulationConfig(particle_count=n, force_method=method, G=1.0, softening=0.05,
                                          barnes_hut_theta=0.5, spatial_hash_cell_size=1.0, spatial_hash_cutoff=1.0),
                      initial_conditions=ic)
        ps.update(1e-3)
        d = ps.getDeviceData()
        before = _state(d)
        calc = {nb.ForceMethod.DIRECT_N2: _calc(nb, "direct", 1.0, 0.05),
                nb.ForceMethod.BARNES_HUT: _calc(nb, "bh", 1.0, 0.05, theta=0.5),
                nb.ForceMethod.SPATIAL_HASH: _calc(nb, "hash", 1.0, 0.05, cell=1.0, cutoff=1.0)}[method]
        want = calc.computeField(d, _dev(pts))
        assert torch.equal(ps.computeFieldAt(pts), want), method            # a host array is uploaded
        assert torch.equal(ps.computeFieldAt(_dev(pts)), want), method
        after = _state(d)
        for k in before:
            assert np.array_equal(before[k], after[k]), (method, k)


# 11. The facade's program: its known answers, and its numbers against the Python API on the same case
def test_facade_field_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "field_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r"^field (\S+) (\S+)$", r.stdout, re.M)}
    d, _ = _bodies(nb, [0.0, 0.0, 0.0], [2.0])
    p = _dev([[0.5, 0.0, 0.0]])
    want = {"direct": _calc(nb, "direct", 1.5, 0.1), "bh_theta0": _calc(nb, "bh", 1.5, 0.1, theta=0.0),
            "bh_theta0.5": _calc(nb, "bh", 1.5, 0.1, theta=0.5),
            "hash_cell2_cutoff2": _calc(nb, "hash", 1.5, 0.1, cell=2.0, cutoff=2.0)}
    assert set(got) == set(want)
    for k, c in want.items():
        v = float(c.computeField(d, p)[0, 3].item())
        assert abs(got[k] - v) <= 1e-6 * abs(v), (k, got[k], v)
