"""Extended state precision of the two Hermite integrators: the declarations of every layer, the restatement the GPU
tests compare against (tests/hermite_ext_ref.py) held to fp64 on displaced clusters and to the accuracy conditions of
DESIGN.md section 4.11, host-side validation and ParticleSystem's handling of the mode.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import hermite_block_ref as br
import hermite_ext_ref as xr
import hermite_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NAMES = ("nbody_hip_hermite_set_precision", "nbody_hip_hermite_get_precision", "nbody_hip_hermite_set_state_f64",
         "nbody_hip_hermite_get_state_f64", "nbody_hip_hermite_block_set_precision", "nbody_hip_hermite_block_get_precision",
         "nbody_hip_hermite_block_set_state_f64", "nbody_hip_hermite_block_get_state_f64", "nbody_hip_direct_acc_jerk_ext")
# the a-priori constant of the jerk criterion in extended mode: derived in tests/test_hermite_ext_gpu.py from section 4.9's
# C = 480.1 and the two extra roundings of d
C_JERK_EXT = 41 + np.sqrt(3.0) * 257 + 1


# ---- 3. interface ------------------------------------------------------------------------------------------------------
def test_header_declares_and_prototypes_bind_the_entry_points(nb):
    src = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for name in NAMES:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        args = " ".join(m.group(1).split())
        res, argtypes = nb._lib.PROTOTYPES[name]
        assert res is not None and len(argtypes) == len(args.split(",")), name
        assert "eps2" not in args, args
    assert re.search(r"#define NBODY_HIP_ABI_VERSION 1\b", src)
    one = lambda name: " ".join(re.search(name + r"\s*\(([^)]*)\)", src).group(1).split())  # noqa: E731
    assert "const nbody_float4* pos_lo_device, float G, float eps" in one("nbody_hip_direct_acc_jerk_ext")
    assert "const double* pos_host, const double* vel_host" in one("nbody_hip_hermite_set_state_f64")
    doc = src[src.index("EXTENDED STATE PRECISION"):src.index("nbody_hip_hermite_set_precision(")]
    for phrase in ("X = pos + pos_lo", "hi = (float)X, lo = (float)(X - hi)", "(x_j,hi - x_i,hi) + (x_j,lo - x_i,lo)",
                   "DISTINCT", "bitwise reproducible", "ALSO zeroes the residuals", "checkpoint"):
        assert phrase in doc, phrase
    # every exported entry point of the library source is declared (the library itself is checked by the ABI test)
    for f, prefix in (("hermite.hip", "nbody_hip_hermite_"), ("hermite_block.hip", "nbody_hip_hermite_block_")):
        text = open(os.path.join(ROOT, "n-body_amd", "csrc", f)).read()
        for tail in ("set_precision", "get_precision", "set_state_f64", "get_state_f64"):
            assert f'extern "C" int {prefix}{tail}(' in text, (f, tail)
    common = open(os.path.join(ROOT, "n-body_amd", "csrc", "hermite_common.h")).read()
    # one text per body, the precision a template flag: the extended forms are instantiations, not copies
    for piece in ("void jerk_pk(", "void jerk_guard(", "void hermite_predict(", "void hermite_correct(", "struct HermiteLo",
                  "if constexpr (EXT)"):
        assert piece in common, piece
    for gone in ("jerk_pk_ext", "jerk_guard_ext", "hermite_predict_ext", "hermite_correct_ext"):
        assert gone not in common, gone


def test_the_loaded_library_exports_the_entry_points(nb):
    lib = nb._lib.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    assert lib.nbody_hip_abi_version() == 1


def test_python_signatures_and_mode_strings(nb):
    for cls in (nb.HermiteIntegrator, nb.BlockHermiteIntegrator):
        assert list(inspect.signature(cls.setStatePrecision).parameters) == ["self", "precision"]
        assert list(inspect.signature(cls.setExtendedState).parameters)[:4] == ["self", "d_particles", "pos64", "vel64"]
        assert list(inspect.signature(cls.getExtendedState).parameters) == ["self", "d_particles"]
        h = cls()
        assert h.getStatePrecision() == "fp32"          # the default keeps today's behaviour
        h.setStatePrecision("extended")                  # (no handle yet: recorded for its creation)
        assert h.getStatePrecision() == "extended"
        h.setStatePrecision("fp32")
        for bad in ("fp64", "Extended", "", None, 1):
            with pytest.raises(nb.ValidationException, match="state precision must be one of"):
                h.setStatePrecision(bad)
        assert h.getStatePrecision() == "fp32"
    assert list(inspect.signature(nb.direct_acc_jerk_ext).parameters)[:5] == ["ctx", "d_particles", "pos_lo", "G", "eps"]
    assert nb.api.STATE_PRECISIONS == ("fp32", "extended")


def test_facade_declares_the_methods():
    hpp = open(os.path.join(ROOT, "n-body_amd", "facade", "include", "nbody_facade.hpp")).read()
    assert "enum class StatePrecision { Fp32 = 0, Extended = 1 };" in hpp
    for cls in ("class HermiteIntegrator {", "class BlockHermiteIntegrator {"):
        body = hpp[hpp.index(cls):]
        body = body[:body.index("\n};")]
        for m in ("void setStatePrecision(StatePrecision p);", "StatePrecision getStatePrecision() const",
                  "void setExtendedState(", "void getExtendedState("):
            assert m in body, (cls, m)
    mk = open(os.path.join(ROOT, "n-body_amd", "facade", "Makefile")).read()
    assert "tests/hermite_ext_tests.cpp" in mk


def test_particle_system_mode_handling(nb):
    ps = nb.ParticleSystem()
    assert ps.getHermiteStatePrecision() == "fp32"
    for bad in ("fp64", "double", None):
        with pytest.raises(nb.ValidationException, match="state precision must be one of"):
            ps.setHermiteStatePrecision(bad)
    ps.setHermiteStatePrecision("extended")
    assert ps.getHermiteStatePrecision() == "extended"
    # the refusals of setIntegrationScheme are untouched by the mode: a Hermite scheme stays Direct-only
    ps.setIntegrationScheme("hermite4")
    with pytest.raises(nb.ValidationException, match="Direct-only"):
        ps.setForceMethod(nb.ForceMethod.BARNES_HUT)
    with pytest.raises(nb.StateException):
        ps.getExtendedState()  # (not initialized)

    # who invalidates (residuals lost) and who only re-primes (residuals kept), without a device: counted on a stand-in
    class Probe:
        def __init__(self):
            self.invalidated, self.precision = 0, None

        def invalidate(self):
            self.invalidated += 1

        def setStatePrecision(self, p):
            self.precision = p

    for mode, expected in (("extended", 0), ("fp32", 2)):
        ps = nb.ParticleSystem()
        ps.setHermiteStatePrecision(mode)
        ps.hermite_, ps.hermite_block_ = Probe(), Probe()
        ps.setGravitationalConstant(1.5)
        ps.setSofteningParameter(0.02)
        ps.setTimeStep(1e-3)
        assert ps.hermite_.invalidated == ps.hermite_block_.invalidated == expected, mode
        ps.setIntegrationScheme("hermite4-block")  # a switch of the scheme loses them
        assert ps.hermite_.invalidated == expected + 1
        ps.setHermiteStatePrecision("fp32" if mode == "extended" else "extended")  # and so does a switch of the mode
        assert ps.hermite_.precision == ps.hermite_block_.precision == ps.getHermiteStatePrecision()
        assert ps.hermite_.invalidated == expected + 2


# ---- 1. the arithmetic model of the pair sweep against fp64 ------------------------------------------------------------
@pytest.fixture(scope="module")
def plummer257(nb):
    ic = nb.ic.plummer(257, seed=42)
    return (np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1), np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1),
            ic["mass"])


@pytest.mark.parametrize("geometry", list(xr.GEOMETRIES))
def test_model_sweep_against_fp64_on_displaced_clusters(plummer257, geometry):
    """257 bodies; the softening shrinks with the cluster (0.01 x scale).  Measured with this model: max |da| / |a| 4.5e-7 /
    5.5e-7 / 6.2e-7 with the residuals, 4.5e-7 / 6.6e-3 / 0.15 from the rounded positions; jerk margins 3.2 / 3.3 / 4.2."""
    scale, centre = xr.GEOMETRIES[geometry]
    X, V, m = xr.displaced_cluster(*plummer257, scale, centre)
    eps = 0.01 * scale
    hi, lo = xr.split(X)
    assert np.array_equal(hi + lo, xr.rnd2(X)) and np.abs(hi + lo - X).max() <= 2.0 ** -49 * np.abs(X).max()
    vh = V.astype(np.float32).astype(np.float64)
    a_ref, j_ref, _, sj = hr.acc_jerk(hi + lo, vh, m, 1.0, eps)
    a, j = xr.acc_jerk_ext(hi, lo, vh, m, 1.0, eps)
    ea = np.linalg.norm(a - a_ref, axis=1) / np.linalg.norm(a_ref, axis=1)
    ej = np.linalg.norm(j - j_ref, axis=1)
    print(f"{geometry}: max |da| / |a| {ea.max():.3e}, jerk margin {(ej / (U * sj)).max():.2f}")
    assert ea.max() <= 1e-5
    assert np.all(ej <= np.maximum(1e-5 * np.linalg.norm(j_ref, axis=1), C_JERK_EXT * U * sj))
    # the same bodies from the rounded positions
    a32, _ = xr.acc_jerk_ext(hi, lo, vh, m, 1.0, eps, use_lo=False)
    e32 = np.linalg.norm(a32 - a_ref, axis=1) / np.linalg.norm(a_ref, axis=1)
    print(f"{geometry}: from the rounded positions max |da| / |a| {e32.max():.3e}")
    if geometry == "centred":
        # scale 1 at the origin is fp32-representable: every residual is zero and the two evaluations are one
        assert not lo.any() and np.array_equal(a32, a)
    else:
        assert e32.max() >= 100 * 1e-5  # the inputs discriminate


def test_model_sweep_conventions():
    """self pair, a coincident pair with and without the guard, a pair split by the residuals only"""
    def jerk_ok(j, ref):  # (the jerk of the third body is a difference of two terms: held by the criterion, not relatively)
        err = np.linalg.norm(j - ref[1], axis=1)
        return np.all(err <= np.maximum(1e-5 * np.linalg.norm(ref[1], axis=1), C_JERK_EXT * U * ref[3]))

    hi = np.array([[64.0, 0, 0], [64.0, 0, 0], [64.5, 0, 0]])
    lo = np.array([[0.0, 0, 0], [0.0, 0, 0], [0.0, 0, 0]])
    v = np.array([[0.0, 1, 0], [0.0, -1, 0], [0.0, 0, 0]])
    m = np.array([1.0, 1.0, 1.0], np.float32)
    a, j = xr.acc_jerk_ext(hi, lo, v, m, 1.0, 0.0)           # guard: the coincident pair adds nothing
    ref = hr.acc_jerk(hi + lo, v, m, 1.0, 0.0)
    assert np.allclose(a, ref[0], rtol=1e-6) and jerk_ok(j, ref) and np.isfinite(j).all()
    a, j = xr.acc_jerk_ext(hi, lo, v, m, 1.0, 0.1)           # softened: m w / eps^3 to the jerk, nothing to a
    ref = hr.acc_jerk(hi + lo, v, m, 1.0, 0.1)
    assert np.allclose(a, ref[0], rtol=1e-6) and jerk_ok(j, ref)
    e2 = hr.eps2_of(0.1)  # body 0: w = (0, -2, 0) from its twin at d = 0, w = (0, -1, 0) from the third body at d = 0.5
    assert abs(j[0, 1] - (-2.0 / e2 ** 1.5 - 1.0 / (0.25 + e2) ** 1.5)) < 1e-5 * abs(j[0, 1])
    lo[1, 0] = 2e-6                                          # hi parts coincide, lo parts differ: a distinct pair
    lo = lo.astype(np.float32).astype(np.float64)
    a, j = xr.acc_jerk_ext(hi, lo, v, m, 1.0, 0.0)
    ref = hr.acc_jerk(hi + lo, v, m, 1.0, 0.0)
    assert a[0, 0] > 1e11 and np.allclose(a, ref[0], rtol=1e-6) and jerk_ok(j, ref)
    a32, _ = xr.acc_jerk_ext(hi, lo, v, m, 1.0, 0.0, use_lo=False)
    assert abs(a32[0, 0]) < 10.0                             # (the fp32 mode does not see it)


# ---- the restatement of the steps --------------------------------------------------------------------------------------
def test_extended_steps_are_the_shared_restatement_in_the_limits(plummer257):
    pos, vel, m = plummer257
    X, V, _ = xr.displaced_cluster(pos, vel, m, 0.05, (64.0, -32.0, 16.0))
    ev = lambda x, v: hr.acc_jerk(x, v, m, 1.0, 0.0005)  # noqa: E731
    ext = xr.hermite_steps_ext(X, V, m, 1.0, 0.0005, 1e-4, 3, evaluate=ev)
    f64 = hr.hermite_steps(X, V, m, 1.0, 0.0005, 1e-4, 3, np.float64)
    f32 = hr.hermite_steps(X, V, m, 1.0, 0.0005, 1e-4, 3, np.float32)
    e_ext, e_32 = np.abs(ext["pos"] - f64["pos"]).max(), np.abs(f32["pos"] - f64["pos"]).max()
    assert e_ext < 1e-9 and e_32 > 1e-6, (e_ext, e_32)       # the extended state follows fp64, the fp32 state cannot
    # the invariant: the state is exactly hi + lo
    assert np.array_equal(xr.rnd2(ext["pos"]), ext["pos"]) and np.array_equal(xr.rnd2(ext["vel"]), ext["vel"])
    # the block restatement at max_level 0 is the shared extended step
    blk = xr.block_steps_ext(X, V, m, 1.0, 0.0005, 1e-4, 3, max_level=0,
                             evaluate=lambda x, v, t: hr.acc_jerk(x, v, m, 1.0, 0.0005, targets=t)[:2])
    for k in ("pos", "vel", "acc", "acc_old", "jerk"):
        assert np.array_equal(blk[k], ext[k]), k


@pytest.fixture(scope="module")
def refs():
    return xr.references()


def test_recorded_references_are_fp64_runs(refs):
    c = xr.BINARY
    X, V, m = xr.binary_state(True)
    short = hr.hermite_steps(X, V, m, 1.0, c["eps"], c["T"] / c["ref_steps"], 64, np.float64)["pos"]
    assert np.abs(short - X).max() < 1e-2  # (64 of 102,400 steps: the bodies have barely moved)
    assert refs["binary_centred_ref"].shape == (2, 3) and refs["block_displaced_ref"].shape == (3, 3)
    # translation invariance of the fp64 run: the displaced reference is the centred one moved
    assert np.abs(refs["binary_displaced_ref"] - xr.CENTRE - refs["binary_centred_ref"]).max() < 1e-10


# ---- 2. the steps: the accuracy the mode is for ------------------------------------------------------------------------
@pytest.mark.parametrize("displaced,ratio", [(False, 10), (True, 100)])
def test_binary_one_period_in_the_restatement(refs, displaced, ratio):
    """e = 0.9, eps 1e-4, 25,600 steps over one period, fp32 pair arithmetic in both runs.  Measured with this model:
    centred 1.1e-7 against 7.1e-6 (1 / 64), at (20, 10, 0) 1.1e-7 against 9.3e-4 (1 / 8,400)."""
    c = xr.BINARY
    X, V, m = xr.binary_state(displaced)
    ref = refs["binary_displaced_ref" if displaced else "binary_centred_ref"]
    dt = c["T"] / c["steps"]
    ext = xr.hermite_steps_ext(X, V, m, 1.0, c["eps"], dt, c["steps"])["pos"]
    f32 = hr.hermite_steps(X, V, m, 1.0, c["eps"], dt, c["steps"], np.float32,
                           evaluate=xr.model_evaluate(m, 1.0, c["eps"], use_lo=False))["pos"]
    e_ext, e_32 = np.abs(ext - ref).max(), np.abs(f32 - ref).max()
    print(f"binary {'displaced' if displaced else 'centred'}: extended {e_ext:.3e}, fp32 state {e_32:.3e}, 1 / {e_32 / e_ext:.0f}")
    assert e_ext <= e_32 / ratio


def test_block_scheme_eta_pair_in_the_restatement(refs):
    """section 4.10's binary case at (20, 10, 0): eta 0.02 -> 0.005 must help in extended mode and must not help (by
    more than 2 x) with the fp32 state.  Measured with this model: extended 5.8e-6 -> 2.8e-7, fp32 9.7e-4 -> 3.2e-3."""
    c = xr.BLOCK
    X, V, m = xr.block_state()
    err = {}
    for eta in c["etas"]:
        kw = dict(eta=eta, max_level=c["L"])
        ext = xr.block_steps_ext(X, V, m, 1.0, c["eps"], c["T"] / c["macro"], c["macro"], **kw)
        f32 = br.block_steps(X, V, m, 1.0, c["eps"], c["T"] / c["macro"], c["macro"], **kw)
        err["extended", eta] = np.abs(ext["pos"] - refs["block_displaced_ref"]).max()
        err["fp32", eta] = np.abs(f32["pos"] - refs["block_displaced_ref"]).max()
    print({f"{k[0]} eta {k[1]}": f"{v:.3e}" for k, v in err.items()})
    e1, e2 = c["etas"]
    assert err["extended", e2] < err["extended", e1]
    assert err["fp32", e2] >= err["fp32", e1] / 2
