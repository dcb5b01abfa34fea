"""The reductions of csrc/energy.hip at their edge shapes against tests/energy_ref.py, the plain fp64 restatement:
nbody_hip_kinetic_energy_f64 / nbody_hip_potential_energy_f64 (the triangular sweep), their float forms,
nbody_hip_direct_potential (the per-body sweep, potential_combine_kernel, term_sum_kernel) and nbody_hip_energies_packed.
Every energy-conservation figure of the project is read off these kernels.

The bodies (energy_ref.bodies) have UNEQUAL masses -- a mass taken from the wrong side of a pair or from the wrong index
cannot show with the equal masses of ic.plummer -- and heavy sentinels at 0, 255, 256, n - 1 (262143, 262144): the loss of
one of them moves the reference by at least 100 x the tolerance (tests/test_energy_cpu.py).  The shapes are the regimes of
the launch plan (energy_ref.plan: one split / one tile per split / a short last split / exact splits) and both sides of
their boundaries, last tiles of 1 and 255 bodies, and the first sizes at which the grid-stride kernels take a second turn.

Bounds: 1e-6 relative on KE and PE, 1e-5 relative per body on phi (the project's own); "bit-equal" and "== 0.0" exact.
Every case prints what it measured ("energy: ..." lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import energy_ref as er
from gpu_util import to_device

pytestmark = pytest.mark.gpu

G, TOL, TOL_PHI = er.G, er.TOL, er.TOL_PHI
GUARD = 16
PHI_CASES = [(n, 0.01) for n in er.PHI_SIZES] + [(n, 0.0) for n in er.PHI_SIZES if n <= 2049]

_memo = {}


def memo(key, make):
    """inputs, their device copies and their references are made once and shared by the cases that need them"""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def rel(got, want):
    """relative error; of a reference that is exactly 0 (one body, no sources, a target of mass 0) only 0 is no error"""
    if want == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - want) / abs(want)


def on_device(nb, n):
    return memo(("device", n), lambda: to_device(nb, er.as_ic(*er.bodies(n)))[0])


def pack(pos, m, vel):
    """(posm [n, 4], vel [n, 4]) on the device; the w lane of the velocities holds a value that must not enter"""
    posm = np.concatenate([pos, np.asarray(m)[:, None]], 1).astype(np.float32)
    vel4 = np.concatenate([vel, np.full((len(vel), 1), 7.0)], 1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(posm)).cuda(), torch.from_numpy(np.ascontiguousarray(vel4)).cuda()


def ref_energies(n, eps):
    pos, vel, m = er.bodies(n)
    return memo(("ke", n), lambda: er.kinetic(vel, m)), memo(("pe", n, eps), lambda: er.potential(pos, m, G, eps))


def backend(nb, ctx):
    from nbody_amd.distributed import HipBackend
    return memo(("backend", id(ctx)), lambda: HipBackend(ctx))


# ---- KE + PE of one body set: kinetic_kernel, potential_kernel<TRI> ---------------------------------------------------------------
@pytest.mark.parametrize("eps", er.EPS)
@pytest.mark.parametrize("n", er.ENERGY_SIZES)
def test_energies_f64(nb, ctx, n, eps):
    ke, pe = nb.Integrator().computeEnergiesF64(on_device(nb, n), G, eps)
    ke_ref, pe_ref = ref_energies(n, eps)
    e_ke, e_pe = rel(ke, ke_ref), rel(pe, pe_ref)
    print(f"energy: f64 n={n} eps={eps} [{er.regime(n)}]: KE rel err {e_ke:.3e}, PE rel err {e_pe:.3e}")
    assert e_ke <= TOL
    if n == 1:
        assert pe == 0.0 and pe_ref == 0.0
    else:
        assert e_pe <= TOL


def test_energies_of_no_bodies(nb, ctx):
    """count = 0 with every array NULL: zeros, nothing dereferenced"""
    d = nb.ParticleData()
    integ = nb.Integrator()
    assert integ.computeEnergiesF64(d, G, 0.01) == (0.0, 0.0)
    assert integ.computeKineticEnergy(d) == 0.0 and integ.computePotentialEnergy(d, G, 0.01) == 0.0
    assert nb.DirectForceCalculator().computePotential(d) == 0.0
    out = (C.c_double * 2)(1.0, 1.0)
    nb._lib.check(nb._lib.load().nbody_hip_energies_packed(ctx.handle, None, None, 0, 0, None, 0, G, 0.01, out))
    assert (out[0], out[1]) == (0.0, 0.0)


@pytest.mark.parametrize("n", er.FLOAT_SIZES)
def test_float_api_is_the_rounded_f64_value(nb, ctx, n):
    d, integ = on_device(nb, n), nb.Integrator()
    ke, pe = integ.computeEnergiesF64(d, G, 0.01)
    assert integ.computeKineticEnergy(d) == np.float32(ke)
    assert integ.computePotentialEnergy(d, G, 0.01) == np.float32(pe)
    assert integ.computeKineticEnergyF64(d) == ke


# ---- KE above the cap of the grid: kinetic_kernel and kinetic_packed_kernel in their second and third turn ----------------------
@pytest.mark.parametrize("n", er.KINETIC_SIZES)
def test_kinetic_energy_above_the_grid_cap(nb, ctx, n):
    """1024 blocks of 256 lanes: 262144 bodies is the last size of one turn.  Through nbody_hip_kinetic_energy_f64, and
    through nbody_hip_energies_packed against 300 sources that are none of the targets (more than 1024 target blocks: the kb
    cap; one source split of two tiles)"""
    pos, vel, m = er.bodies(n)
    spos, _, sm = er.bodies(300, seed=5)
    ke_ref, pe_ref = memo(("shard300", n), lambda: er.shard(pos, m, vel, -n, spos, sm, G, 0.01))
    ke = nb.Integrator().computeKineticEnergyF64(on_device(nb, n))
    posm, vel4 = pack(pos, m, vel)
    src, _ = pack(spos, sm, np.zeros((300, 3)))
    ke_p, pe_p = backend(nb, ctx).energies(posm, vel4, -n, src, G, 0.01)
    print(f"energy: KE n={n}: f64 rel err {rel(ke, ke_ref):.3e}, packed rel err {rel(ke_p, ke_ref):.3e}, "
          f"packed PE against 300 sources rel err {rel(pe_p, pe_ref):.3e}")
    assert rel(ke, ke_ref) <= TOL
    assert rel(ke_p, ke_ref) <= TOL
    assert rel(pe_p, pe_ref) <= TOL


# ---- per-body Direct potential: potential_kernel<PER>, potential_combine_kernel, term_sum_kernel --------------------------------
def run_potential(nb, d, eps, ctx=None):
    """-> (phi as fp64, PE with a phi buffer, PE without); the words behind phi must keep what they held"""
    c = nb.DirectForceCalculator(ctx=ctx)
    c.setGravitationalConstant(G)
    c.setSofteningParameter(eps)
    buf = torch.full((d.count + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    pe = c.computePotential(d, buf[:d.count])
    pe_alone = c.computePotential(d)
    buf = buf.cpu().numpy()
    assert np.isnan(buf[d.count:]).all(), "the words behind phi were written"
    return buf[:d.count].astype(np.float64), pe, pe_alone


def check_potential(tag, phi, pe, pe_alone, pos, m, phi_ref, pe_ref):
    n = len(m)
    assert pe_alone.hex() == pe.hex(), f"{tag}: PE without a phi buffer {pe_alone!r}, with one {pe!r}"
    if n == 1:
        assert phi[0] == 0.0 and pe == 0.0 and pe_ref == 0.0
        return
    e_phi = np.abs(phi - phi_ref) / np.abs(phi_ref)
    half = 0.5 * float((m.astype(np.float64) * phi).sum())
    print(f"energy: potential {tag}: phi max rel err {e_phi.max():.3e} (body {int(e_phi.argmax())}), PE rel err "
          f"{rel(pe, pe_ref):.3e}, 1/2 sum m phi against PE {rel(half, pe):.3e}")
    assert e_phi.max() <= TOL_PHI
    assert rel(pe, pe_ref) <= TOL
    # phi_i = fl32(-G s_i), PE = -G/2 sum m_i s_i in fp64, every m_i s_i >= 0: the roundings of phi move the sum by at most
    # 2^-24 of itself (5.96e-8; the fp64 sums of both sides are seven orders below).  With unequal masses this holds only
    # if body i's term carries body i's mass: the check store_potential depends on.
    assert rel(half, pe) <= 6e-8


@pytest.mark.parametrize("n,eps", PHI_CASES)
def test_direct_potential(nb, ctx, n, eps):
    pos, vel, m = er.bodies(n)
    phi, pe, pe_alone = run_potential(nb, on_device(nb, n), eps)
    check_potential(f"n={n} eps={eps}", phi, pe, pe_alone, pos, m, memo(("phi", n, eps), lambda: er.phi(pos, m, G, eps)),
                    ref_energies(n, eps)[1])


# ---- nbody_hip_energies_packed against energy_ref.shard ----------------------------------------------------------------------------
def packed_cases():
    return memo(("packed cases",), _packed_cases)


def _packed_cases():
    """name -> (targets, self_offset, sources), each body set (pos, vel, m).  The sources: N_PACKED bodies, a short last
    tile of 245.  Targets that alias sources are the SAME bodies (r = 0: with softening a self pair that is not excluded
    adds m^2 / eps); the others are fresh bodies."""
    ns = er.N_PACKED
    S = er.bodies(ns)
    fresh = er.bodies(40, seed=9)
    cut = lambda b, lo, hi: tuple(a[lo:hi] for a in b)                              # noqa: E731
    cat = lambda *bs: tuple(np.concatenate(parts) for parts in zip(*bs))           # noqa: E731
    return {
        "shard_from_0": (cut(S, 0, 300), 0, S),
        "shard_at_255_of_2": (cut(S, 255, 257), 255, S),
        "shard_768_to_the_end": (cut(S, 768, ns), 768, S),                         # its self indices: the short last tile
        "offset_minus_3": (cat(cut(fresh, 0, 3), cut(S, 0, 7)), -3, S),            # targets 3..9 are sources 0..6
        "offset_ns_minus_2": (cat(cut(S, ns - 2, ns), cut(fresh, 3, 6)), ns - 2, S),   # only the first two alias
        "disjoint_at_ns": (cut(fresh, 0, 5), ns, S),
        "disjoint_at_minus_nt": (cut(fresh, 0, 5), -5, S),
        "disjoint_far_above": (cut(fresh, 0, 5), 1 << 40, S),
        "disjoint_far_below": (cut(fresh, 0, 5), -(1 << 40), S),
        "one_target": (cut(S, 500, 501), 500, S),
        "one_target_of_mass_0": (cut(S, 900, 901), 900, S),                        # KE and PE share exactly 0
        "one_target_in_the_last_slot": (cut(S, ns - 1, ns), ns - 1, S),
        "one_fresh_target": (cut(fresh, 7, 8), ns, S),
        "no_sources": (cut(S, 0, 300), 0, cut(S, 0, 0)),
        "more_targets_than_sources": (S, 0, cut(S, 0, 100)),                       # targets 0..99 alias, the others do not
        "piece_0_301": (cut(S, 0, 301), 0, S),
        "piece_301_777": (cut(S, 301, 777), 301, S),
        "piece_777_end": (cut(S, 777, ns), 777, S),
    }


def run_packed(nb, ctx, name, eps):
    (tpos, tvel, tm), off, (spos, svel, sm) = packed_cases()[name]
    posm, vel4 = pack(tpos, tm, tvel)
    src, _ = pack(spos, sm, svel)
    got = backend(nb, ctx).energies(posm, vel4, off, src, G, eps)
    want = memo(("packed", name, eps), lambda: er.shard(tpos, tm, tvel, off, spos, sm, G, eps))
    return got, want


@pytest.mark.parametrize("eps", er.EPS)
@pytest.mark.parametrize("name", list(packed_cases()))
def test_energies_packed(nb, ctx, name, eps):
    (ke, pe), (ke_ref, pe_ref) = run_packed(nb, ctx, name, eps)
    print(f"energy: packed {name} eps={eps}: KE rel err {rel(ke, ke_ref):.3e}, PE rel err {rel(pe, pe_ref):.3e}")
    if name == "no_sources":
        assert pe == 0.0 and pe_ref == 0.0
    if name == "one_target_of_mass_0":
        assert (ke, pe) == (0.0, 0.0) and (ke_ref, pe_ref) == (0.0, 0.0)
    assert rel(ke, ke_ref) <= TOL
    assert rel(pe, pe_ref) <= TOL


@pytest.mark.parametrize("eps", er.EPS)
def test_energies_packed_pieces_sum_to_the_whole(nb, ctx, eps):
    """cuts at 301 and 777, off the tile grid: the three shares against the PE of the whole set"""
    got = [run_packed(nb, ctx, name, eps)[0] for name in ("piece_0_301", "piece_301_777", "piece_777_end")]
    ke_ref, pe_ref = ref_energies(er.N_PACKED, eps)
    ke, pe = sum(g[0] for g in got), sum(g[1] for g in got)
    print(f"energy: packed three pieces eps={eps}: KE rel err {rel(ke, ke_ref):.3e}, PE rel err {rel(pe, pe_ref):.3e}")
    assert rel(ke, ke_ref) <= TOL and rel(pe, pe_ref) <= TOL


# ---- the workspace: ctx->reduce is reused and only grows ---------------------------------------------------------------------------
def entry_points(nb):
    def energies(c, n):
        return nb.Integrator(ctx=c).computeEnergiesF64(on_device(nb, n), G, 0.01)

    def potential(c, n):
        phi, pe, pe_alone = run_potential(nb, on_device(nb, n), 0.01, ctx=c)
        return pe, pe_alone, phi.tobytes()

    def packed(c, n):
        posm, vel4 = memo(("packed whole", n), lambda: pack(*(er.bodies(n)[k] for k in (0, 2, 1))))
        return backend(nb, c).energies(posm, vel4, 0, posm, G, 0.01)
    return {"energies_f64": energies, "direct_potential": potential, "energies_packed": packed}


def test_workspace_reuse_large_small_large(nb, ctx):
    """one context through 12288, 3, 257, 11777, 1 bodies with each entry point in turn: every value bit for bit what a
    context of its own gives (a final sum that read one partial too many would add what the larger call left behind)"""
    calls = entry_points(nb)
    own = nb.Context()
    got = {(name, n): call(own, n) for name, call in calls.items() for n in er.REUSE_SIZES}
    for (name, n), value in got.items():
        fresh = nb.Context()
        want = calls[name](fresh, n)
        _memo.pop(("backend", id(fresh)), None)
        fresh.close()
        assert value == want, f"{name}, n={n}: {value[:2]} on the reused context, {want[:2]} on a fresh one"
    _memo.pop(("backend", id(own)), None)
    own.close()
    for n in er.REUSE_SIZES:      # and they are the right values
        ke_ref, pe_ref = ref_energies(n, 0.01)
        for name in calls:
            ke, pe = (None, got[name, n][0]) if name == "direct_potential" else got[name, n]
            assert ke is None or rel(ke, ke_ref) <= TOL
            assert (pe == 0.0 and pe_ref == 0.0) if n == 1 else rel(pe, pe_ref) <= TOL


# ---- a denormal r^2 between a padded target lane and a real source --------------------------------------------------------------
def test_a_source_within_a_denormal_r2_of_the_padded_lanes(nb, ctx):
    """eps = 0, 257 bodies, the last one at (1e-20, 0, 0): the 255 padded lanes of the second block (at the origin, mass 0)
    see it at r^2 = 1e-40.  The reference is finite (no real pair is closer than 1); a reciprocal square root that returns
    inf there must not reach the block sum through 0 x inf."""
    pos, vel, m = er.denormal_case()
    n = len(m)
    sep = np.linalg.norm(pos[:-1].astype(np.float64) - pos[-1], axis=1)
    assert pos[-1, 0] == np.float32(1e-20) > 0 and sep.min() >= 1.0 and np.linalg.norm(pos[:-1], axis=1).min() >= 1.0
    assert 0 < float(pos[-1, 0]) ** 2 < float(np.finfo(np.float32).tiny)
    ke_ref, pe_ref = er.kinetic(vel, m), er.potential(pos, m, G, 0.0)
    assert np.isfinite(pe_ref)
    d = to_device(nb, er.as_ic(pos, vel, m))[0]
    ke, pe = nb.Integrator().computeEnergiesF64(d, G, 0.0)
    phi, pe_phi, pe_alone = run_potential(nb, d, 0.0)
    posm, vel4 = pack(pos, m, vel)
    ke_p, pe_p = backend(nb, ctx).energies(posm, vel4, 0, posm, G, 0.0)
    print(f"energy: denormal case: PE {pe!r} (triangular), {pe_phi!r} (per body), {pe_p!r} (packed), reference {pe_ref!r}")
    assert np.isfinite([pe, pe_phi, pe_p]).all()
    assert rel(ke, ke_ref) <= TOL and rel(ke_p, ke_ref) <= TOL
    assert rel(pe, pe_ref) <= TOL and rel(pe_p, pe_ref) <= TOL
    check_potential("denormal case", phi, pe_phi, pe_alone, pos, m, er.phi(pos, m, G, 0.0), pe_ref)
