"""The Hermite integrator with individual block time steps (nbody_hip_hermite_block_*): the declarations of every layer,
the restatement the GPU tests compare against (tests/hermite_block_ref.py) pinned to the shared-step restatement, to its
own invariants, to hand-made cases of the level rule and to the two accuracy conditions of DESIGN.md section 4.10, and
ParticleSystem's scheme switching.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import hermite_block_ref as br
import hermite_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nbody_hip_hermite_block_create", "nbody_hip_hermite_block_destroy", "nbody_hip_hermite_block_set_params",
         "nbody_hip_hermite_block_prime", "nbody_hip_hermite_block_invalidate", "nbody_hip_hermite_block_step",
         "nbody_hip_hermite_block_advance", "nbody_hip_hermite_block_state", "nbody_hip_hermite_block_set_levels",
         "nbody_hip_hermite_block_tuning", "nbody_hip_hermite_block_info")


# ---- declarations (these fail without the feature) ---------------------------------------------------------------------
def test_header_declares_and_prototypes_bind_the_entry_points(nb):
    src = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for name in NAMES:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        args = " ".join(m.group(1).split())
        res, argtypes = nb._lib.PROTOTYPES[name]
        assert res is not None and len(argtypes) == len(args.split(",")), name
        assert "eps2" not in args, args
    assert "typedef struct nbody_hip_hermite_block nbody_hip_hermite_block;" in src
    one = lambda name: " ".join(re.search(name + r"\s*\(([^)]*)\)", src).group(1).split())  # noqa: E731
    assert "float dt_max, int block_steps" in one("nbody_hip_hermite_block_step")
    assert "float dt_max, int macro_steps" in one("nbody_hip_hermite_block_advance")
    assert "float eta, float eta_start, int max_level" in one("nbody_hip_hermite_block_set_params")
    assert "int* levels, unsigned int* ticks, float* want, nbody_float4* jerk" in one("nbody_hip_hermite_block_state")
    doc = src[src.index("INDIVIDUAL BLOCK TIME STEPS"):src.index("typedef struct nbody_hip_hermite_block ")]
    for phrase in ("no reference counterpart", "MACRO STEPS", "AT tick_i", "NONE of its arrays written", "FLOOR HIT",
                   "bit for bit", "no floating-point atomics", "ERR_STATE in the middle of a macro step"):
        assert phrase in doc or phrase in src[src.index("INDIVIDUAL BLOCK TIME STEPS") - 200:], phrase
    # the info struct of the header and its ctypes mirror agree field by field
    body = src[src.index("typedef struct nbody_hip_hermite_block_info_t {"):src.index("} nbody_hip_hermite_block_info_t;")]
    fields = re.findall(r"(?:unsigned long long|unsigned int|int)\s+(\w+)(?:\[\d+\])?;", body)
    assert fields == [f for f, _ in nb._lib.HermiteBlockInfoStruct._fields_]
    assert "hermite_block" in nb._lib.CLOSE_ORDER
    assert nb._lib.CLOSE_ORDER.index("hermite_block") < nb._lib.CLOSE_ORDER.index("context")
    assert re.search(r"#define NBODY_HIP_ABI_VERSION 1\b", src)
    mk = open(os.path.join(ROOT, "n-body_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bhermite_block\.hip\b", mk, re.M)
    tool = open(os.path.join(ROOT, "tools", "disasm_diff.py")).read()
    assert '"hermite_block.hip"' in tool
    # the pair bodies live in one header both translation units include
    for f in ("hermite.hip", "hermite_block.hip"):
        text = open(os.path.join(ROOT, "n-body_amd", "csrc", f)).read()
        assert '#include "hermite_common.h"' in text and "void jerk_pk(" not in text, f
    common = open(os.path.join(ROOT, "n-body_amd", "csrc", "hermite_common.h")).read()
    for piece in ("void jerk_pk(", "void jerk_guard(", "float rsq(", "constexpr int TS = 256;", "typedef float f2"):
        assert piece in common, piece


def test_python_signatures_as_documented(nb):
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    B = nb.BlockHermiteIntegrator
    assert sig(B.__init__) == ["self", "block_size", "ctx"]
    assert sig(B.integrate) == ["self", "d_particles", "force_calc", "dt_max"]
    assert sig(B.advance) == ["self", "d_particles", "force_calc", "dt_max", "macro_steps"]
    assert sig(B.block_step) == ["self", "d_particles", "force_calc", "dt_max", "block_steps"]
    assert sig(B.prime) == ["self", "d_particles", "force_calc", "dt_max"]
    assert sig(B.setParameters) == ["self", "eta", "eta_start", "max_level"]
    p = inspect.signature(B.setParameters).parameters
    assert (p["eta"].default, p["eta_start"].default, p["max_level"].default) == (0.02, 0.01, 16)
    for name in ("invalidate", "getLevels", "getState", "getJerk", "info", "close"):
        assert sig(getattr(B, name)) == ["self"], name
    for name in ("computeKineticEnergy", "computePotentialEnergy", "computeTotalEnergy", "computeKineticEnergyF64",
                 "computeEnergiesF64"):
        assert sig(getattr(B, name)) == sig(getattr(nb.Integrator, name)), name
    assert not issubclass(B, nb.Integrator) and not issubclass(B, nb.HermiteIntegrator)  # a class of its own
    from nbody_amd import system
    assert system.INTEGRATION_SCHEMES == ("velocity-verlet", "hermite4", "hermite4-block")


def test_facade_declares_the_class():
    hpp = open(os.path.join(ROOT, "n-body_amd", "facade", "include", "nbody_facade.hpp")).read()
    body = hpp[hpp.index("class BlockHermiteIntegrator {"):]
    body = body[:body.index("};")]
    for decl in ("void integrate(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max);",
                 "void advance(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max, int macro_steps);",
                 "void blockStep(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max, int block_steps = 1);",
                 "void prime(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max);", "void invalidate();",
                 "void setParameters(float eta = 0.02f, float eta_start = 0.01f, int max_level = 16);",
                 "void getLevels(int* h_out) const;", "BlockHermiteInfo info() const;", "float computeKineticEnergy(",
                 "float computePotentialEnergy(", "float computeTotalEnergy("):
        assert decl in body, decl
    cpp = open(os.path.join(ROOT, "n-body_amd", "facade", "src", "facade_device.cpp")).read()
    impl = cpp[cpp.index("BlockHermiteIntegrator::handleFor"):]
    # (the exact-type rule is the file's one requireDirect, which handleFor calls first)
    assert 'requireDirect("BlockHermiteIntegrator", method, fc, d);' in impl[:400]
    rule = cpp[cpp.index("void requireDirect("):]
    assert "typeid(*fc) != typeid(DirectForceCalculator)" in rule[:400]
    mk = open(os.path.join(ROOT, "n-body_amd", "facade", "Makefile")).read()
    assert "tests/hermite_block_tests.cpp" in mk and "$(LIBDIR)/hermite_block_tests" in mk.split("\n\n")[1]


def test_refusals_name_the_method_and_say_direct_only(nb):
    class Sub(nb.DirectForceCalculator):
        pass

    b = nb.BlockHermiteIntegrator()
    for calc in (nb.BarnesHutCalculator(0.5), nb.SpatialHashCalculator(1.0, 2.0), Sub()):
        for method, call in (("integrate", lambda c: b.integrate(None, c, 1e-3)),
                             ("advance", lambda c: b.advance(None, c, 1e-3, 2)),
                             ("block_step", lambda c: b.block_step(None, c, 1e-3, 1)),
                             ("prime", lambda c: b.prime(None, c, 1e-3))):
            with pytest.raises(ValueError) as e:
                call(calc)
            assert f"BlockHermiteIntegrator.{method}" in str(e.value) and "Direct-only" in str(e.value)
            assert type(calc).__name__ in str(e.value)
    for call in (b.getLevels, b.getState, b.getJerk, b.info):
        with pytest.raises(nb.StateException):
            call()
    with pytest.raises(nb.ValidationException):
        b.setParameters(max_level=21)
    with pytest.raises(nb.ValidationException):
        b.setParameters(eta=0.0)
    b.invalidate()  # nothing to invalidate yet: no error


# ---- ParticleSystem: scheme switching without a device -----------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.invalidated = 0

    def invalidate(self):
        self.invalidated += 1


def test_particle_system_scheme_switching(nb):
    ps = nb.ParticleSystem()
    ps.setIntegrationScheme("hermite4-block")
    assert ps.getIntegrationScheme() == "hermite4-block"
    for method in (nb.ForceMethod.BARNES_HUT, nb.ForceMethod.SPATIAL_HASH):
        with pytest.raises(nb.ValidationException) as e:
            ps.setForceMethod(method)  # switching away from Direct while it is selected
        assert "hermite4-block" in str(e.value) and "Direct-only" in str(e.value) and method.name in str(e.value)
        assert ps.getForceMethod() == nb.ForceMethod.DIRECT_N2
    cfg = nb.SimulationConfig(particle_count=8, force_method=nb.ForceMethod.BARNES_HUT)
    with pytest.raises(nb.ValidationException):
        ps.initialize(cfg)  # (refused before anything touches the device)
    ps.setIntegrationScheme("velocity-verlet")
    ps.setForceMethod(nb.ForceMethod.BARNES_HUT)
    with pytest.raises(nb.ValidationException) as e:
        ps.setIntegrationScheme("hermite4-block")  # refused at the call with another force method
    assert "Direct-only" in str(e.value) and "BARNES_HUT" in str(e.value)
    assert ps.getIntegrationScheme() == "velocity-verlet"
    ps.setForceMethod(nb.ForceMethod.DIRECT_N2)
    ps.setIntegrationScheme("hermite4-block")
    # every path that invalidates the shared-step handle invalidates this one
    ps.hermite_ = shared = _Recorder()
    ps.hermite_block_ = rec = _Recorder()
    ps.setGravitationalConstant(2.0)
    ps.setSofteningParameter(0.05)
    assert rec.invalidated == 2
    ps.setIntegrationScheme("hermite4")
    ps.setIntegrationScheme("hermite4-block")
    ps.setIntegrationScheme("velocity-verlet")
    assert rec.invalidated == 5 and shared.invalidated == rec.invalidated
    # neither the configuration nor the checkpoint knows the scheme
    assert not any("scheme" in k or "hermite" in k or "level" in k for k in vars(nb.SimulationConfig()))
    assert not any("scheme" in k or "jerk" in k or "level" in k for k in vars(nb.SimulationState()))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _plummer(nb, n, seed=42):
    return br.plummer_case(nb.ic.plummer(n, seed=seed))


def test_level_zero_is_the_shared_step_restatement(nb):
    pos, vel, m = _plummer(nb, 64, seed=3)
    a = br.block_steps(pos, vel, m, 1.7, 0.05, 1 / 64, 3, max_level=0)
    b = hr.hermite_steps(pos, vel, m, 1.7, 0.05, 1 / 64, 3)
    for k in ("pos", "vel", "acc", "acc_old", "jerk"):
        assert np.array_equal(a[k], b[k]), k
    assert a["body_steps"] == 3 * 64 and a["block_steps"] == 3 and a["level_steps"][0] == 3 * 64
    assert not a["ticks"].any() and not a["levels"].any() and a["macro_steps"] == 3


def test_invariants_after_every_block_step(nb):
    pos, vel, m = _plummer(nb, 96, seed=5)
    L = 10
    run = br.BlockHermite(pos, vel, m, 1.0, 0.01, 1 / 8, max_level=L)
    assert len(set(run.level)) > 2  # (the case has a spread of levels)
    arrays = ("x", "v", "a", "a_old", "j", "level", "tick", "want")
    steps = 0
    for macro in range(2):
        while True:
            before = {k: getattr(run, k).copy() for k in arrays}
            t, A = run.schedule()
            assert np.array_equal(A, np.flatnonzero(before["tick"] + 2 ** (L - before["level"]) == t))
            assert (before["tick"] + 2 ** (L - before["level"]) >= t).all() and len(A) >= 1
            t2, A2 = run.step()
            steps += 1
            assert (t2, list(A2)) == (t, list(A))
            rest = np.setdiff1d(np.arange(len(pos)), A)
            wrapped = t == 2 ** L
            for k in arrays:
                if k == "tick" and wrapped:
                    continue
                assert np.array_equal(getattr(run, k)[rest], before[k][rest], equal_nan=True), k
            if wrapped:
                assert not run.tick.any() and len(A) == len(pos)
                break
            assert (run.tick <= t).all() and (run.tick[A] == t).all()
            assert (run.tick % 2 ** (L - run.level) == 0).all()  # alignment, after the level moves
            assert ((run.level >= 0) & (run.level <= L)).all()
        assert run.macro_steps == macro + 1  # every macro step completes
    assert run.block_steps == steps and run.level_steps.sum() == run.body_steps


def test_level_rule_on_hand_made_cases():
    L, dt_max, eta = 8, 1.0, 0.02
    z = np.zeros((1, 3))
    ex = np.array([[1.0, 0.0, 0.0]])

    def rule(a0, j0, a1, j1, k, t):
        h = dt_max / 2.0 ** k
        new, want, floor = br.new_level(a0, j0, a1, j1, [h], dt_max, eta, [k], L, [t])
        return int(new[0]), float(want[0]), bool(floor[0])

    # a constant acceleration with no jerk: a2 = a3 = 0, the denominator is 0 -> +inf; one doubling, only when aligned
    assert rule(ex, z, ex, z, 3, 2 * 2 ** (L - 3)) == (2, np.inf, False)
    assert rule(ex, z, ex, z, 3, 3 * 2 ** (L - 3)) == (3, np.inf, False)  # t is not a multiple of 2 * 2^(L-k)
    assert rule(ex, z, ex, z, 0, 2 ** L) == (0, np.inf, False)             # level 0 stays
    # a0 = a1, j0 = -j1 = (s, 0, 0): a2 = -2 s / h, a3 = 0, a2 + h a3 = -2 s / h -> want = sqrt(eta (2 s / h + s^2)) h / (2 s)
    k, s = 2, 4.0
    h = dt_max / 2 ** k
    want = np.sqrt(float(np.float32(eta)) * (1.0 * (2 * s / h) + s * s) / ((2 * s / h) ** 2))  # (eta is an fp32 number)
    new, got, floor = rule(ex, s * ex, ex, -s * ex, k, 2 ** (L - k))
    assert got == pytest.approx(want, rel=1e-14) and want < h
    expect = k
    while expect < L and want < dt_max / 2 ** expect:
        expect += 1
    assert new == expect and new - k >= 2 and not floor  # several halvings in one go
    # the same case one level above the floor (want ~ 0.07 h whatever h is): the level stops at L, the hit is counted
    new, got, floor = rule(ex, 1e6 * ex, ex, -1e6 * ex, L - 1, 2)
    assert new == L and floor and got < dt_max / 2 ** L
    new, got, floor = rule(ex, 1e6 * ex, ex, -1e6 * ex, L, 1)
    assert new == L and floor
    # want in [dt, 2 dt): the level stays (no doubling below the factor 2, no halving above dt)
    k = 2
    h = dt_max / 2 ** k
    s = eta / (4.5 * h)  # want ~ sqrt(eta h / (2 s)) = 1.5 h
    new, got, floor = rule(ex, s * ex, ex, -s * ex, k, 2 ** L)
    assert h <= got < 2 * h and new == k and not floor
    # priming: the smallest level whose step is not longer than eta_start |a| / |j|, clamped; +inf without a jerk
    lv, want = br.prime_levels(np.array([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]]),
                               np.array([[0.0, 0, 0], [0.03, 0, 0], [1e9, 0, 0], [1.0, 0, 0]]), 0.01, 1.0, L)
    assert want[0] == np.inf and want[1] == pytest.approx(1.0 / 3.0) and want[3] == 0.0
    assert list(lv) == [0, 2, L, L]


@pytest.fixture(scope="module")
def refs():
    return br.references()


def test_recorded_references_are_the_shared_step_runs(refs):
    """the golden file holds what hermite_block_ref.compute_references computes: spot check of the binary case at a
    coarser reference (fourth order: 8,192 steps are within 4e-6 of 32,768)"""
    pos, vel, m = br.binary_case()
    c = br.BINARY
    coarse = hr.hermite_steps(pos, vel, m, 1.0, c["eps"], c["T"] / 8192, 8192, np.float64)["pos"]
    assert np.abs(coarse - refs["binary_ref"]).max() <= 4e-6
    assert refs["plummer_ref"].shape == (256, 3) and 1.5e-5 < refs["plummer_shared_err"] < 2e-5
    assert 3e-5 < refs["binary_shared_err"] < 4e-5


def test_plummer_condition(nb, refs):
    """block steps at eta = 0.02 on ic.plummer(256, seed=42), eps = 0.01, T = 1: max |dx| against the fp64 reference not
    above that of the shared fp32 run of 512 steps (1.70e-5) AND at most a quarter of its 131,072 body steps.
    Restatement: 9.2e-6 with 16,478 body steps in 816 block steps."""
    c = br.PLUMMER
    pos, vel, m = _plummer(nb, c["n"], c["seed"])
    r = br.block_steps(pos, vel, m, 1.0, c["eps"], c["dt_max"], c["macro"], eta=0.02, eta_start=0.01, max_level=c["L"])
    err = np.abs(r["pos"] - refs["plummer_ref"]).max()
    print(f"plummer: max |dx| {err:.3e} (shared 512 steps: {refs['plummer_shared_err']:.3e}), {r['body_steps']} body "
          f"steps in {r['block_steps']} block steps, floor hits {r['floor_hits']}")
    assert err <= refs["plummer_shared_err"]
    assert r["body_steps"] <= c["shared_steps"] * c["n"] // 4
    assert r["floor_hits"] == 0 and r["macro_steps"] == c["macro"]


def test_binary_condition(refs):
    """the e = 0.9 binary with a light third body, eps = 1e-4, one period, dt_max = T / 16, L = 16: error not above the
    shared fp32 run of 4,096 steps and at most an eighth of its 12,288 body steps.  Restatement: 6.7e-6 with 502 body
    steps in 243 block steps, levels 0-8."""
    c = br.BINARY
    pos, vel, m = br.binary_case()
    r = br.block_steps(pos, vel, m, 1.0, c["eps"], c["T"] / c["macro"], c["macro"], eta=0.02, eta_start=0.01,
                       max_level=c["L"])
    err = np.abs(r["pos"] - refs["binary_ref"]).max()
    print(f"binary: max |dx| {err:.3e} (shared 4,096 steps: {refs['binary_shared_err']:.3e}), {r['body_steps']} body "
          f"steps in {r['block_steps']} block steps, levels {np.flatnonzero(r['level_steps'])}")
    assert err <= refs["binary_shared_err"]
    assert r["body_steps"] <= c["shared_steps"] * 3 // 8
    assert r["floor_hits"] == 0
    shallow = br.block_steps(pos, vel, m, 1.0, c["eps"], c["T"] / c["macro"], c["macro"], max_level=2)
    assert shallow["floor_hits"] > 0 and shallow["level_steps"][3:].sum() == 0
