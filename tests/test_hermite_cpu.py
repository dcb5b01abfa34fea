"""Direct force-and-jerk and the fourth-order Hermite integrator (nbody_hip_hermite_*, nbody_hip_direct_acc_jerk): the
declarations of every layer, the fp64 restatements the GPU tests compare against (tests/hermite_ref.py) pinned to closed
forms and to the order of the scheme, and ParticleSystem's scheme switching.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import hermite_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nbody_hip_hermite_create", "nbody_hip_hermite_destroy", "nbody_hip_hermite_prime",
         "nbody_hip_hermite_invalidate", "nbody_hip_hermite_step", "nbody_hip_hermite_jerk",
         "nbody_hip_hermite_suggest_dt", "nbody_hip_direct_acc_jerk")


# ---- declarations (these fail without the feature) ---------------------------------------------------------------------
def test_header_declares_and_prototypes_bind_the_eight_entry_points(nb):
    src = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    nargs = {}
    for name in NAMES:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        args = " ".join(m.group(1).split())
        nargs[name] = len(args.split(","))
        assert "eps2" not in args, args  # eps, like the potential and field calls
    assert "typedef struct nbody_hip_hermite nbody_hip_hermite;" in src
    assert "float dt, int steps" in " ".join(re.search(r"nbody_hip_hermite_step\s*\(([^)]*)\)", src).group(1).split())
    assert "nbody_float4* acc_out_or_null, nbody_float4* jerk_out" in " ".join(
        re.search(r"nbody_hip_direct_acc_jerk\s*\(([^)]*)\)", src).group(1).split())
    # the header says what continuation after a checkpoint is, and does not claim more
    doc = src[src.index("FOURTH-ORDER HERMITE"):src.index("typedef struct nbody_hip_hermite")]
    assert "truncation order" in doc and "NOT bit for bit" in doc and "no reference counterpart" in src[
        src.index("FOURTH-ORDER HERMITE") - 120:src.index("FOURTH-ORDER HERMITE")]
    for name in NAMES:
        res, args = nb._lib.PROTOTYPES[name]
        assert res is not None and len(args) == nargs[name], name
    assert "hermite" in nb._lib.CLOSE_ORDER  # registered with the atexit registry, before the contexts
    assert nb._lib.CLOSE_ORDER.index("hermite") < nb._lib.CLOSE_ORDER.index("context")
    assert re.search(r"#define NBODY_HIP_ABI_VERSION 1\b", src)
    mk = open(os.path.join(ROOT, "n-body_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bhermite\.hip\b", mk, re.M)


def test_python_signatures_as_documented(nb):
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    H = nb.HermiteIntegrator
    assert sig(H.__init__) == ["self", "block_size", "ctx"]
    assert inspect.signature(H.__init__).parameters["block_size"].default == 256
    assert sig(H.integrate) == ["self", "d_particles", "force_calc", "dt"]
    assert sig(H.integrate_steps) == ["self", "d_particles", "force_calc", "dt", "steps"]
    assert sig(H.prime) == ["self", "d_particles", "force_calc"]
    assert sig(H.invalidate) == ["self"] and sig(H.getJerk) == ["self"]
    assert sig(H.suggestTimeStep) == ["self", "eta"]
    assert inspect.signature(H.suggestTimeStep).parameters["eta"].default == 0.02
    for name in ("computeKineticEnergy", "computePotentialEnergy", "computeTotalEnergy", "computeKineticEnergyF64",
                 "computeEnergiesF64"):
        assert sig(getattr(H, name)) == sig(getattr(nb.Integrator, name)), name
    assert sig(nb.direct_acc_jerk)[:4] == ["ctx", "d_particles", "G", "eps"]
    assert sig(nb.ParticleSystem.setIntegrationScheme) == ["self", "scheme"]
    assert sig(nb.ParticleSystem.getIntegrationScheme) == ["self"]
    assert not issubclass(H, nb.Integrator)  # Integrator itself is not touched: a class of its own


def test_facade_declares_the_class():
    hpp = open(os.path.join(ROOT, "n-body_amd", "facade", "include", "nbody_facade.hpp")).read()
    body = hpp[hpp.index("class HermiteIntegrator {"):]
    body = body[:body.index("};")]
    for decl in ("void integrate(ParticleData* d_particles, ForceCalculator* force_calc, float dt);",
                 "void integrateSteps(ParticleData* d_particles, ForceCalculator* force_calc, float dt, int steps);",
                 "void prime(ParticleData* d_particles, ForceCalculator* force_calc);", "void invalidate();",
                 "void getJerk(float4* d_out) const;", "float suggestTimeStep(float eta = 0.02f) const;",
                 "float computeKineticEnergy(", "float computePotentialEnergy(", "float computeTotalEnergy("):
        assert decl in body, decl
    cpp = open(os.path.join(ROOT, "n-body_amd", "facade", "src", "facade_device.cpp")).read()
    assert "typeid(*fc) != typeid(DirectForceCalculator)" in cpp
    mk = open(os.path.join(ROOT, "n-body_amd", "facade", "Makefile")).read()
    assert "tests/hermite_tests.cpp" in mk and "$(LIBDIR)/hermite_tests" in mk.split("\n\n")[1]


def test_refusals_name_the_method_and_say_direct_only(nb):
    class Sub(nb.DirectForceCalculator):
        pass

    h = nb.HermiteIntegrator()
    for calc in (nb.BarnesHutCalculator(0.5), nb.SpatialHashCalculator(1.0, 2.0), Sub()):
        for method, call in (("integrate", lambda c: h.integrate(None, c, 1e-3)),
                             ("integrate_steps", lambda c: h.integrate_steps(None, c, 1e-3, 2)),
                             ("prime", lambda c: h.prime(None, c))):
            with pytest.raises(ValueError) as e:
                call(calc)
            assert f"HermiteIntegrator.{method}" in str(e.value) and "Direct-only" in str(e.value)
            assert type(calc).__name__ in str(e.value)
    with pytest.raises(nb.StateException):
        h.getJerk()
    with pytest.raises(nb.StateException):
        h.suggestTimeStep()
    h.invalidate()  # nothing to invalidate yet: no error


# ---- ParticleSystem: scheme switching without a device -----------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.invalidated = 0

    def invalidate(self):
        self.invalidated += 1


def test_particle_system_scheme_switching(nb):
    ps = nb.ParticleSystem()
    assert ps.getIntegrationScheme() == "velocity-verlet"
    ps.setIntegrationScheme("hermite4")
    assert ps.getIntegrationScheme() == "hermite4"
    for method in (nb.ForceMethod.BARNES_HUT, nb.ForceMethod.SPATIAL_HASH):
        with pytest.raises(nb.ValidationException) as e:
            ps.setForceMethod(method)  # switching away from Direct while it is selected
        assert "hermite4" in str(e.value) and "Direct-only" in str(e.value) and method.name in str(e.value)
        assert ps.getForceMethod() == nb.ForceMethod.DIRECT_N2
    cfg = nb.SimulationConfig(particle_count=8, force_method=nb.ForceMethod.BARNES_HUT)
    with pytest.raises(nb.ValidationException):
        ps.initialize(cfg)  # (refused before anything touches the device)
    ps.setIntegrationScheme("velocity-verlet")
    ps.setForceMethod(nb.ForceMethod.BARNES_HUT)
    with pytest.raises(nb.ValidationException) as e:
        ps.setIntegrationScheme("hermite4")  # refused at the call with another force method
    assert "Direct-only" in str(e.value) and "BARNES_HUT" in str(e.value)
    assert ps.getIntegrationScheme() == "velocity-verlet"
    with pytest.raises(nb.ValidationException):
        ps.setIntegrationScheme("leapfrog")
    ps.setForceMethod(nb.ForceMethod.DIRECT_N2)
    ps.setIntegrationScheme("hermite4")
    # every parameter change behind the integrator invalidates its handle
    ps.hermite_ = rec = _Recorder()
    ps.setGravitationalConstant(2.0)
    ps.setSofteningParameter(0.05)
    assert rec.invalidated == 2
    ps.setIntegrationScheme("velocity-verlet")
    ps.setIntegrationScheme("hermite4")
    assert rec.invalidated == 4
    # neither the configuration nor the checkpoint knows the scheme
    assert not any("scheme" in k or "hermite" in k for k in vars(nb.SimulationConfig()))
    assert not any("scheme" in k or "jerk" in k for k in vars(nb.SimulationState()))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_two_bodies_closed_form():
    G, eps = 1.7, 0.05
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, -0.25]], np.float32)
    vel = np.array([[0.0, 0.1, 0.0], [0.1, -0.2, 0.3]], np.float32)
    m = np.array([2.0, 0.75], np.float32)
    a, j, sa, sj = hr.acc_jerk(pos, vel, m, G, eps)
    d = pos[1].astype(np.float64) - pos[0]
    w = vel[1].astype(np.float64) - vel[0]
    h = d @ d + hr.eps2_of(eps)
    for i, s in ((0, G * 0.75), (1, -G * 2.0)):
        assert np.allclose(a[i], s * d * h ** -1.5, rtol=1e-14, atol=0)
        assert np.allclose(j[i], s * (w - 3.0 * (d @ w) / h * d) * h ** -1.5, rtol=1e-14, atol=0)
    assert np.allclose(sa, np.linalg.norm(a, axis=1), rtol=1e-14)  # one term: the magnitude sums are the magnitudes
    assert (sj >= np.linalg.norm(j, axis=1) * (1 - 1e-14)).all()
    # coincident bodies: nothing to a; m w / eps^3 to j -- and nothing to either under the guard convention
    pos2 = np.array([[0.25, 0.5, 1.0], [0.25, 0.5, 1.0]], np.float32)
    a, j, _, _ = hr.acc_jerk(pos2, vel, m, G, eps)
    assert not a.any() and np.allclose(j[0], G * 0.75 * w * hr.eps2_of(eps) ** -1.5, rtol=1e-14)
    a, j, sa, sj = hr.acc_jerk(pos2, vel, m, G, 0.0)
    assert not a.any() and not j.any() and not sa.any() and not sj.any()
    # `targets` selects rows
    a3, j3, _, _ = hr.acc_jerk(pos, vel, m, G, eps, targets=[1])
    a2, j2, _, _ = hr.acc_jerk(pos, vel, m, G, eps)
    assert np.array_equal(a3[0], a2[1]) and np.array_equal(j3[0], j2[1])


def _plummer(nb, n):
    ic = nb.ic.plummer(n, seed=42)
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)
    vel = np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1)
    return pos, vel, ic["mass"]


@pytest.mark.parametrize("n, eps", [(64, 0.1), (64, 0.01), (256, 0.05)])
def test_jerk_is_the_time_derivative_of_the_acceleration(nb, n, eps):
    """j = the central difference of a along x +- v h in fp64; h = 1e-4, relative <= 1e-5, G = 1.7"""
    pos, vel, m = _plummer(nb, n)
    pos, vel = pos.astype(np.float64), vel.astype(np.float64)
    G, h = 1.7, 1e-4
    _, j, _, _ = hr.acc_jerk(pos, vel, m, G, eps)
    ap = hr.acc_jerk(pos + vel * h, vel, m, G, eps)[0]
    am = hr.acc_jerk(pos - vel * h, vel, m, G, eps)[0]
    rel = np.linalg.norm((ap - am) / (2 * h) - j, axis=1) / np.linalg.norm(j, axis=1)
    print(f"n={n} eps={eps}: max relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-5


def test_momentum_sums_vanish(nb):
    pos, vel, m = _plummer(nb, 256)
    rng = np.random.default_rng(3)
    m = (m * rng.uniform(0.5, 2.0, len(m))).astype(np.float32)  # general masses
    a, j, sa, sj = hr.acc_jerk(pos, vel, m, 1.7, 0.05)
    m64 = m.astype(np.float64)
    assert np.abs((m64[:, None] * a).sum(0)).max() <= 1e-13 * (m64 * sa).sum()
    assert np.abs((m64[:, None] * j).sum(0)).max() <= 1e-13 * (m64 * sj).sum()


@pytest.fixture(scope="module")
def binary_errors():
    """max |dx| after one period (T = 6.25) of the e = 0.5 binary against an fp64 Hermite run of 65,536 steps"""
    pos, vel, m = hr.binary()
    T, eps = 6.25, 0.01
    ref = hr.hermite_steps(pos, vel, m, 1.0, eps, T / 65536, 65536, np.float64)["pos"]
    out = {}
    for n in (50, 100, 200):
        out["h64", n] = np.abs(hr.hermite_steps(pos, vel, m, 1.0, eps, T / n, n, np.float64)["pos"] - ref).max()
        out["vv", n] = np.abs(hr.vv_steps(pos, vel, m, 1.0, eps, T / n, n, np.float64)["pos"] - ref).max()
    out["h32", 50] = np.abs(hr.hermite_steps(pos, vel, m, 1.0, eps, T / 50, 50, np.float32)["pos"] - ref).max()
    out["h32", 100] = np.abs(hr.hermite_steps(pos, vel, m, 1.0, eps, T / 100, 100, np.float32)["pos"] - ref).max()
    return out


def test_order_of_the_scheme_on_the_binary(binary_errors):
    e = binary_errors
    print({k: f"{v:.3e}" for k, v in e.items()})
    assert 12 <= e["h64", 50] / e["h64", 100] <= 20     # fourth order: 16
    assert 12 <= e["h64", 100] / e["h64", 200] <= 20
    assert 3.5 <= e["vv", 100] / e["vv", 200] <= 4.5    # the comparison scheme is second order
    assert e["h64", 200] <= e["vv", 200] / 16


def test_order_survives_fp32_state(binary_errors):
    e = binary_errors
    assert e["h32", 50] / e["h32", 100] >= 8


def test_suggest_dt():
    a = np.array([[3.0, 0.0, 4.0], [1.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    j = np.array([[0.0, 10.0, 0.0], [0.0, 0.0, 4.0], [0.0, 0.0, 0.0]])  # the third body has no jerk: not counted
    assert hr.suggest_dt(a, j, 0.02) == pytest.approx(0.02 * 0.25)
    assert hr.suggest_dt(a, np.zeros_like(j)) == float("inf")
