"""The three Hermite handles (nbody_hip_hermite_*, _block_*, _batch_*) without a GPU: what every entry point answers to a
null handle, the public surface of the three Python classes, the CPU check of the carve arithmetic (make handle_check:
hermite_carve.h under AddressSanitizer and UBSan against the written-out up256 chain) and where the shared host code
lives."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
FILES = ("hermite.hip", "hermite_block.hip", "hermite_batch.hip")


def _noun(name):
    if name.startswith("nbody_hip_hermite_batch_"):
        return b"null block-step Hermite ensemble"
    if name.startswith("nbody_hip_hermite_block_"):
        return b"null block-step Hermite integrator"
    return b"null Hermite integrator"


def _zero(argtype):
    """a null pointer, or the zero of a scalar type"""
    if argtype is C.c_void_p or issubclass(argtype, C._Pointer):
        return None
    return argtype(0)


# ---- 1. the null-handle contract ---------------------------------------------------------------------------------------
def test_every_entry_point_answers_a_null_handle(nb):
    lib = nb._lib.load()
    names = sorted(n for n in nb._lib.PROTOTYPES if n.startswith("nbody_hip_hermite_"))
    assert len(names) == 46 and sum(n.endswith("_create") for n in names) == 3, names
    for name in names:
        fn, argtypes = getattr(lib, name), nb._lib.PROTOTYPES[name][1]
        if name.endswith("_destroy"):
            assert fn(None) == nb._lib.OK, name
        elif name.endswith("_create"):
            out = C.c_void_p(0x1)
            assert fn(*[_zero(t) for t in argtypes[:-1]], C.byref(out)) == nb._lib.ERR_STATE, name
            assert lib.nbody_hip_last_error().startswith(b"null context"), name
            assert out.value is None, name  # (the out pointer is cleared before anything is refused)
            assert fn(*[_zero(t) for t in argtypes]) == nb._lib.ERR_STATE, name
            assert lib.nbody_hip_last_error().startswith(b"null output pointer"), name
        else:
            assert fn(*[_zero(t) for t in argtypes]) == nb._lib.ERR_STATE, name
            assert lib.nbody_hip_last_error().startswith(_noun(name)), (name, lib.nbody_hip_last_error())


# ---- 2. the public surface of the three classes (generated from the tree before the handle core, pasted) ----------------
CTOR = "(block_size: 'int' = 256, ctx: 'Context | None' = None)"
STATE = {
    "close": "(self)",
    "ctx": "property",
    "getBlockSize": "(self)",
    "getExtendedState": "(self, d_particles: 'ParticleData')",
    "getJerk": "(self) -> 'torch.Tensor'",
    "getStatePrecision": "(self) -> 'str'",
    "invalidate": "(self)",
    "setBlockSize": "(self, size)",
    "setExtendedState": "(self, d_particles: 'ParticleData', pos64, vel64, force_calc=None)",
    "setStatePrecision": "(self, precision: 'str')",
}
ENERGIES = {
    "computeEnergiesF64": "(self, d_particles, G, eps)",
    "computeKineticEnergy": "(self, d_particles) -> 'float'",
    "computeKineticEnergyF64": "(self, d_particles) -> 'float'",
    "computePotentialEnergy": "(self, d_particles, G, eps) -> 'float'",
    "computeTotalEnergy": "(self, d_particles, G, eps) -> 'float'",
}
BLOCK = {
    "getState": "(self) -> 'dict'",
    "setParameters": "(self, eta: 'float' = 0.02, eta_start: 'float' = 0.01, max_level: 'int' = 16)",
}
SURFACE = {
    "HermiteIntegrator": {
        **STATE, **ENERGIES,
        "integrate": "(self, d_particles: 'ParticleData', force_calc, dt: 'float')",
        "integrate_steps": "(self, d_particles: 'ParticleData', force_calc, dt: 'float', steps: 'int')",
        "prime": "(self, d_particles: 'ParticleData', force_calc)",
        "suggestTimeStep": "(self, eta: 'float' = 0.02) -> 'float'",
    },
    "BlockHermiteIntegrator": {
        **STATE, **ENERGIES, **BLOCK,
        "advance": "(self, d_particles: 'ParticleData', force_calc, dt_max: 'float', macro_steps: 'int')",
        "block_step": "(self, d_particles: 'ParticleData', force_calc, dt_max: 'float', block_steps: 'int' = 1)",
        "diagnostics": "(self, d_particles: 'ParticleData', force_calc) -> 'np.ndarray'",
        "diagnostics_into": "(self, d_particles: 'ParticleData', force_calc, out: 'torch.Tensor')",
        "getLevels": "(self) -> 'np.ndarray'",
        "getScheduling": "(self)",
        "info": "(self) -> 'dict'",
        "integrate": "(self, d_particles: 'ParticleData', force_calc, dt_max: 'float')",
        "prime": "(self, d_particles: 'ParticleData', force_calc, dt_max: 'float')",
        "setLevels": "(self, levels)",
        "setScheduling": "(self, scheduling: 'str')",
        "setTuning": "(self, narrow_below: 'int' = 0)",
    },
    "BlockHermiteEnsemble": {
        **STATE, **BLOCK,
        "advance": "(self, d_particles: 'ParticleData', macro_steps: 'int' = 1)",
        "diagnostics": "(self, d_particles: 'ParticleData') -> 'np.ndarray'",
        "diagnostics_into": "(self, d_particles: 'ParticleData', out: 'torch.Tensor')",
        "events": "(self) -> 'np.ndarray'",
        "info": "(self, system=None) -> 'dict'",
        "prime": "(self, d_particles: 'ParticleData', force_calc, dt_max)",
        "running": "(self) -> 'int'",
        "setEvents": "(self, radii=None, max_macro_steps=None, track_closest: 'bool' = False, stop_on_contact: 'bool' = False)",
        "setLayout": "(self, offsets)",
    },
}


def test_public_surface_of_the_three_classes(nb):
    for cls_name, want in SURFACE.items():
        cls = getattr(nb, cls_name)
        assert str(inspect.signature(cls)) == CTOR, cls_name
        got = {}
        for name in sorted(n for n in dir(cls) if not n.startswith("_")):
            attr = inspect.getattr_static(cls, name)
            got[name] = "property" if isinstance(attr, property) else str(inspect.signature(getattr(cls, name)))
        assert sorted(got) == sorted(want), cls_name  # (the ensemble has no energy methods)
        assert got == want, cls_name
    # the wording of the refusals follows the class
    for cls_name, noun in (("HermiteIntegrator", "Hermite integrator"), ("BlockHermiteIntegrator", "block-step Hermite integrator"),
                           ("BlockHermiteEnsemble", "block-step Hermite ensemble")):
        h = getattr(nb, cls_name)()
        try:
            h.getJerk()
        except nb.StateException as e:
            assert str(e) == f"the {noun} is not primed"
        else:
            raise AssertionError(cls_name)
        try:
            h._direct(object(), "prime")
        except ValueError as e:
            assert str(e).startswith(f"{cls_name}.prime: the Hermite scheme is Direct-only -- it needs exactly a "
                                     f"DirectForceCalculator (the tree and the grid have no jerk), got object")
        else:
            raise AssertionError(cls_name)
        assert h.getBlockSize() == 256 and h._h is None and h._capacity == 0 and h._count == 0 and h._precision == 0


# ---- the carve arithmetic under the sanitizers --------------------------------------------------------------------------
def test_handle_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "handle_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hermite_handle_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/hermite_handle_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    carve = re.sub(r"//.*", "", open(os.path.join(CSRC, "hermite_carve.h")).read())
    for word in ("hip", "__global__", "__device__", "float4"):  # plain C++: no device, no HIP header
        assert word not in carve, word


# ---- 3. where the shared host code lives (this part cannot pass before the handle core: the tree before it has no
# hermite_handle.h, two copies of up256 and the four launch macros) ------------------------------------------------------
def test_the_three_files_share_the_handle_core():
    core = open(os.path.join(CSRC, "hermite_handle.h")).read()
    for piece in ("struct HermiteHandleCore", "const char* noun", "struct BlockParams", "hermite_arrays(", "with_flags(",
                  '#include "hermite_carve.h"'):
        assert piece in core, piece
    for f in FILES:
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "hermite_handle.h"' in text, f
        assert "static size_t up256" not in text, f
        assert not re.search(r"#\s*define\s+NBH_", text), f
        assert "HermiteArrays{d->pos_x" not in text, f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^hermite\.o hermite_block\.o hermite_batch\.o:.*\bhermite_handle\.h\b.*\bhermite_carve\.h\b", mk, re.M)
