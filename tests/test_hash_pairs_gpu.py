"""The cutoff decision of the spatial-hash kernels, pair by pair at its exact edges: every force kernel of the grid
(nbody_hip_grid_tuning 0, 1, 2, 3, 4, 6, 7, 8, 9, 10), both eps regimes (eps = 0.05 cutoff: the compare-free forms;
eps = 0: the GUARD instantiations), both sides of the switch at the ends of the compare-free range, the two-grid form
and the field, on the lattice populations of tests/hash_pair_ref.py -- pairs with d2 == cutoff2 by the thousand, and
planted pairs 2, 1 and 0 floats below and above it.

Every comparison is against the grid-free restatement hash_pair_ref.reference (checked on the CPU in
tests/test_hash_pairs_cpu.py), never against another run of the code under test, except where a scaled population is
compared bit for bit with the unscaled one.  Asserted per body: tier 1 of tests/gpu_util.py (err_i <= max(1e-5, C u
kappa_i), C of the "gold" kind and of the kernel that ran -- derived, not fitted); bodies whose reference is 0 are +0
bit for bit.  Tier 2 is printed (hash_stats), not asserted: its limits were measured on other populations.  One pair on
the wrong side of the decision moves a body by hundreds of bounds (test_hash_pairs_cpu.py asserts that of the inputs).

Every case asserts that its grid has a start array (without one the kernels 8 to 10 would fall back to the cell-run
kernel) and that the cells exported by the build are the intended ones, so that every accepted pair lies in
neighbouring cells.

nbody_hip_grid_potential is left out on purpose: the shifted potential is 0 at the cutoff by design, so a pair on the
wrong side of the decision changes phi by a rounding error only -- phi cannot show a wrong tie.  For the same reason the
field's phi is held only to the 1e-5 of its scale that tests/test_field_gpu.py uses.

Scaled populations (everything x 2^k, masses x 4^k): where HashParams::guard() picks the same instantiation on both
sides, the accelerations are asserted EQUAL BIT FOR BIT to the unscaled ones (a factor 4^k leaves the mantissa of d2 +
eps2 and the parity of its exponent alone, which is all v_rsq_f32 looks at).  Measured on an MI355X: it holds for all ten
kernel settings, both eps regimes and both populations.
"""
import ctypes as C

import numpy as np
import pytest

import hash_pair_ref as hp
import sort_ref as sr
from gpu_util import C_SUM, hash_bound, hash_stats, rel_err

pytestmark = pytest.mark.gpu
F = np.float32
KERNELS = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)
FRACTIONS = (hp.EPS_FRACTION, 0.0)
G = 1.0


def build(nb, pop, members=None, slab=None):
    """a packed build of the population (or of its bodies `members`) with its explicit bounds -> (grid, device bodies).
    Asserts the grid's dimensions, the exported cells and the start array."""
    import torch
    lib = nb._lib.load()
    posm = pop.posm if members is None else np.ascontiguousarray(pop.posm[members])
    n = posm.shape[0]
    grid = nb.SpatialHashGrid(n, float(pop.cell))
    nb._lib.check(lib.nbody_hip_grid_set_slab(grid._h, *(slab if slab is not None else (0, 0))))
    dev = torch.from_numpy(posm).cuda()
    nb._lib.check(lib.nbody_hip_grid_build_packed(grid._h, dev.data_ptr(), n, (C.c_float * 6)(*[float(b) for b in pop.bounds])))
    assert tuple(grid._info()[0]) == pop.dims(), f"{pop.name}: grid {grid._info()[0]} against {pop.dims()}"
    _, _, pc, _ = sr.grid_cell_data(nb, grid, n)
    want = pop.cells() if members is None else pop.cells()[members]
    assert np.array_equal(pc, want), f"{pop.name}: particle_cells against the intended cells"
    assert grid.copyCellStartArray() is not None, f"{pop.name}: no start array"
    return grid, dev


def pairs_in_neighbouring_cells(pop, pc, ref):
    d = pop.dims()
    xyz = np.stack([pc % d[0], (pc // d[0]) % d[1], pc // (d[0] * d[1])], 1).astype(np.int64)
    i, j = ref["pairs"]
    assert float(pop.cell) >= 1.01 * float(pop.cutoff) and np.abs(xyz[i] - xyz[j]).max() <= 1


def forces(nb, grid, pop, eps, kern, n=None):
    import torch
    n = pop.n if n is None else n
    acc = torch.full((n, 4), 7.0, device="cuda")
    grid.tuning(kern)
    nb._lib.check(nb._lib.load().nbody_hip_grid_compute_forces_packed(grid._h, float(pop.cutoff), G, float(eps), acc.data_ptr()))
    torch.cuda.synchronize()
    grid.tuning(0)
    a = acc.cpu().numpy()
    assert np.all(a[:, 3].view(np.uint32) == 0)
    return np.ascontiguousarray(a[:, :3])


def check(tag, a, acc_ref, kappa, kern):
    """tier 1 on every body with a non-zero reference, +0 bit for bit on the others; prints the statistics of tier 2"""
    nz = np.linalg.norm(acc_ref, axis=1) > 0
    assert np.all(np.ascontiguousarray(a[~nz]).view(np.uint32) == 0), f"{tag}: a body without an accepted partner is not +0"
    assert np.all(np.isfinite(a)), tag
    err, kap = rel_err(a[nz], acc_ref[nz]), kappa[nz]
    bound = hash_bound(kap, "gold", kern)
    st = hash_stats(err, kap, a.shape[0])
    worst = int(np.argmax(err / bound)) if err.size else 0
    print(f"hash pairs {tag} [gold, kernel {kern}]: " + ", ".join(f"{k} {v:.3g}" for k, v in st.items())
          + (f"; worst vs bound: err {err[worst]:.3e} bound {bound[worst]:.3e} (body {np.flatnonzero(nz)[worst]})"
             if err.size else ""), flush=True)
    assert np.all(err <= bound), f"{tag}: {int((err > bound).sum())} bodies outside tier 1, worst {err[worst]:.3e} against {bound[worst]:.3e}"


def centre_terms(pop, ref, eps):
    """[(centre, None: no accepted partner / the single term of its one accepted partner)] of a star population"""
    eps2 = F(F(eps) * F(eps))
    out = []
    for ctr, _, _ in pop.planted:
        mine = ref["pairs"][1][ref["pairs"][0] == ctr]
        if len(mine) == 0:
            out.append((ctr, None))
        elif len(mine) == 1:
            d = pop.ints[int(mine[0])] - pop.ints[ctr]
            h = float(F(F(float(hp.dist2_fp32(*d)) * pop.unit * pop.unit) + eps2))
            out.append((ctr, G * float(pop.mass[int(mine[0])]) * d.astype(np.float64) * pop.unit * h ** -1.5))
    assert any(t is None for _, t in out) and any(t is not None for _, t in out)
    return out


def check_centres(tag, a, terms, kern):
    """a star's centre: the sum over exactly its accepted satellites -- none: +0; one: that single term, to tier 1"""
    for ctr, term in terms:
        if term is None:
            assert np.all(a[ctr].view(np.uint32) == 0), f"{tag}: centre {ctr} has no accepted partner"
        else:
            e = np.linalg.norm(a[ctr] - term) / np.linalg.norm(term)
            assert e <= hash_bound(1.0, "gold", kern), f"{tag}: centre {ctr}, one partner: {e:.3e}"


def guard_of(pop, eps):
    lo, hi, g = hp.limits()
    return bool(F(F(eps) * F(eps)) < g or not (lo <= pop.cutoff2 <= hi))


# ---- every kernel on every population ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("key", hp.KEYS, ids=str)
def test_pairs_on_the_edge(nb, ctx, monkeypatch, key, fraction):
    """ties by the thousand (dense: windows of several LDS batches, the filtered form, the later passes of the two-phase
    form; sparse: light cells beside crowded ones) and the planted pairs of the stars, through all ten kernel settings;
    the dense populations once more on a grid that always takes the unit-list forms"""
    pop = hp.population(key)
    eps = pop.eps(fraction)
    ref = hp.reference_of(key, fraction)
    assert guard_of(pop, eps) == (fraction == 0.0)
    terms = centre_terms(pop, ref, eps) if pop.planted else None
    for units in (None, "2") if key in hp.TIES else (None,):
        if units:
            monkeypatch.setenv("NBH_HASH_UNITS", units)
        grid, keep = build(nb, pop)
        pairs_in_neighbouring_cells(pop, sr.grid_cell_data(nb, grid, pop.n)[2], ref)
        for kern in KERNELS if units is None else (2, 3, 4, 6, 7):
            tag = f"{pop.name} eps {eps}{' unit lists' if units else ''}"
            a = forces(nb, grid, pop, eps, kern)
            check(tag, a, ref["acc"], ref["kappa"], kern)
            if pop.planted:
                check_centres(tag, a, terms, kern)
        del keep
        grid.close()


# ---- both sides of the switch at the ends of the compare-free range -----------------------------------------------------------
@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("key", hp.SCALED, ids=str)
def test_scaled_populations(nb, ctx, key, fraction):
    """x 2^k for the largest k whose cutoff2 the compare-free decision still takes, the smallest k for which GUARD takes
    over, and a negative k that takes eps2 below the GUARD threshold.  Against the restatement of the scaled population
    (tier 1, the same exact zeros) on both sides of a switch; bit for bit against the unscaled run where the
    instantiation is the same."""
    base = hp.population(key)
    k_in, k_out, k_neg = hp.scale_exponents(base)
    grid, keep = build(nb, base)
    a0 = {kern: forces(nb, grid, base, base.eps(fraction), kern) for kern in KERNELS}
    del keep
    grid.close()
    g0 = guard_of(base, base.eps(fraction))
    same = []
    for k in (k_in, k_out, k_neg):
        pop = hp.population(key, k)
        eps = pop.eps(fraction)
        ref = hp.reference_of(key, fraction, k)
        gk = guard_of(pop, eps)
        assert gk == (fraction == 0.0 or k != k_in)
        grid, keep = build(nb, pop)
        for kern in KERNELS:
            tag = f"{pop.name} eps {eps} ({'GUARD' if gk else 'compare-free'})"
            a = forces(nb, grid, pop, eps, kern)
            check(tag, a, ref["acc"], ref["kappa"], kern)
            if gk == g0:
                bad = np.flatnonzero((a.view(np.uint32) != a0[kern].view(np.uint32)).any(axis=1))
                assert bad.size == 0, (f"{tag} kernel {kern}: {bad.size} bodies differ from the unscaled run, first {bad[0]}: "
                                       f"{a[bad[0]]} against {a0[kern][bad[0]]}")
        same.append(gk == g0)
        del keep
        grid.close()
    assert same == ([True, False, False] if fraction else [True, True, True])


# ---- the two-grid form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("key", hp.FIELD, ids=str)
def test_two_grid_form(nb, ctx, key, fraction):
    """nbody_hip_grid_forces_pair_packed on a ties population cut along z into two slabs, built as
    test_packed_slabs_equal_whole builds them: own x own on the slab's grid, then the slab's boundary layers against a grid
    of the halo layer, accumulated.  Ties straddle the cut."""
    import torch
    pop = hp.population(key)
    eps = pop.eps(fraction)
    ref = hp.reference_of(key, fraction)
    lib = nb._lib.load()
    gz = pop.dims()[2]
    cz = pop.cells_xyz()[:, 2]
    cut = int(np.median(cz)) + 1 if key[2] == "off" else 2
    i, j = hp.reference_of(key, hp.EPS_FRACTION, le=True)["pairs"]
    tie = hp.pair_d2(pop, (i, j)) == pop.c2_units
    assert ((cz[i] < cut) & (cz[j] >= cut) & tie).sum() > 100, "ties across the cut"
    for z0, z1 in ((0, cut), (cut, gz)):
        own = np.flatnonzero((cz >= z0) & (cz < z1))
        halo = np.flatnonzero((cz == z0 - 1) | (cz == z1))
        assert own.size > 500 and halo.size > 100
        h0 = max(z0 - 1, 0)
        g_own, keep_own = build(nb, pop, own, (z0, z1 - z0))
        g_halo, keep_halo = build(nb, pop, halo, (h0, min(z1 + 1, gz) - h0))
        for kern in KERNELS:
            g_own.tuning(kern)
            acc = torch.full((own.size, 4), 7.0, device="cuda")
            nb._lib.check(lib.nbody_hip_grid_forces_pair_packed(g_own._h, g_own._h, z0, z1 - z0, float(pop.cutoff), G, float(eps),
                                                                acc.data_ptr(), 0))
            for z in sorted({z0, z1 - 1}):
                nb._lib.check(lib.nbody_hip_grid_forces_pair_packed(g_own._h, g_halo._h, z, 1, float(pop.cutoff), G, float(eps),
                                                                    acc.data_ptr(), 1))
            torch.cuda.synchronize()
            a = acc.cpu().numpy()
            assert np.all(a[:, 3] == 0)
            check(f"{pop.name} eps {eps} two grids, layers [{z0}, {z1})", np.ascontiguousarray(a[:, :3]), ref["acc"][own],
                  ref["kappa"][own], kern)
        g_own.tuning(0)
        del keep_own, keep_halo
        g_own.close()
        g_halo.close()


# ---- the field ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("key", hp.FIELD, ids=str)
def test_field_on_lattice_sites(nb, ctx, key, fraction):
    """SpatialHashGrid.computeField at every site of the lattice, occupied (a coincident pair) or not: nearly every one is
    exactly at the cutoff from several bodies.  The force part under the checks of the force kernels (partial sums of
    at most 32 entries: the C_SUM of kernels 2 to 4), phi to 1e-5 of its scale as in tests/test_field_gpu.py."""
    import torch
    pop = hp.population(key)
    eps = pop.eps(fraction)
    sites = hp.field_sites()
    ref = hp.reference(pop, eps, targets=sites)
    grid, keep = build(nb, pop)
    pts = torch.from_numpy((sites.astype(np.float64) * pop.unit).astype(F)).cuda()
    out = grid.computeField(pts, float(pop.cutoff), G, float(eps)).cpu().numpy()
    assert C_SUM[2] == 32
    check(f"{pop.name} eps {eps} field", np.ascontiguousarray(out[:, :3]), ref["acc"], ref["kappa"], 2)
    some = ref["phi_scale"] > 0
    assert not out[~some, 3].any()
    ephi = np.abs(out[some, 3].astype(np.float64) - ref["phi"][some]) / ref["phi_scale"][some]
    print(f"{pop.name} eps {eps} field: |dphi| / scale max {ephi.max():.3e}")
    assert ephi.max() <= 1e-5
    del keep
    grid.close()
