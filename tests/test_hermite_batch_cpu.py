"""The block-step Hermite ensemble (nbody_hip_hermite_batch_*, BlockHermiteEnsemble), the parts that need no GPU: ic.concat,
the Python-side argument checks, the null-handle answers, the prototypes against the header, and the property of the
300-system case that tests/test_hermite_batch_gpu.py relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hermite_batch_cases as bc
import hermite_block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("create", "destroy", "set_params", "set_precision", "get_precision", "set_layout", "prime", "invalidate",
         "advance", "state", "info", "set_state_f64", "get_state_f64")


def test_concat_offsets_and_contents(nb):
    parts = [nb.ic.plummer(n, seed=7 + n) for n in (3, 257, 1)]
    ic, off = nb.ic.concat(parts)
    assert off.dtype == np.uint64 and off.tolist() == [0, 3, 260, 261]
    assert sorted(ic) == sorted(("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass"))
    for s, p in enumerate(parts):
        for k, v in ic.items():
            assert v.dtype == np.float32 and v.shape == (261,)
            assert np.array_equal(v[int(off[s]):int(off[s + 1])], p[k]), (s, k)
    one, off1 = nb.ic.concat([parts[1]])
    assert off1.tolist() == [0, 257] and all(np.array_equal(one[k], parts[1][k]) for k in one)
    with pytest.raises(ValueError, match="at least one system"):
        nb.ic.concat([])
    short = dict(parts[0])
    short["vel_z"] = short["vel_z"][:2]
    with pytest.raises(ValueError, match="system 1"):
        nb.ic.concat([parts[1], short])
    empty = {k: v[:0] for k, v in parts[0].items()}
    with pytest.raises(ValueError, match="system 0"):
        nb.ic.concat([empty])


def test_python_side_argument_checks(nb):
    e = nb.BlockHermiteEnsemble()
    assert e.getStatePrecision() == "fp32" and e._offsets is None
    for bad in ((0.0, 0.01, 16), (float("nan"), 0.01, 16), (0.02, -1.0, 16), (0.02, float("inf"), 16), (0.02, 0.01, 21),
                (0.02, 0.01, -1)):
        with pytest.raises(nb.ValidationException):
            e.setParameters(*bad)
    e.setParameters(0.03, 0.02, 10)
    assert e._params == (0.03, 0.02, 10)
    with pytest.raises(nb.ValidationException, match="state precision must be one of"):
        e.setStatePrecision("fp64")
    e.setStatePrecision("extended")
    assert e.getStatePrecision() == "extended"
    # offsets: dtype and shape
    for bad, what in (([0.0, 4.0], "must be integers"), (np.zeros((2, 2), np.int64), "one-dimensional"), ([0], "B \\+ 1 >= 2"),
                      ([], "B \\+ 1 >= 2"), ([0, -4], "must not be negative"), (np.array([0, 4], np.float32), "must be integers")):
        with pytest.raises(nb.ValidationException, match=what):
            e.setLayout(bad)
    assert e._offsets is None
    e.setLayout(np.array([0, 4, 16], np.int32))
    assert e._offsets.dtype == np.uint64 and e._offsets.tolist() == [0, 4, 16]
    # the length of a dt_max array, and the calculator, are checked before any handle exists
    d = nb.ParticleData()
    fc = nb.DirectForceCalculator.__new__(nb.DirectForceCalculator)  # (no context: the checks come first)
    for bad in ([0.1], [0.1, 0.1, 0.1], np.zeros((2, 1), np.float32)):
        with pytest.raises(nb.ValidationException, match="dt_max must be a scalar or an array of 2 values"):
            e.prime(d, fc, bad)
    with pytest.raises(ValueError, match="Direct-only"):
        e.prime(d, object(), 0.1)
    with pytest.raises(nb.StateException, match="no layout"):
        nb.BlockHermiteEnsemble().prime(d, fc, 0.1)
    with pytest.raises(nb.StateException, match="not primed"):
        e.advance(d, 1)
    for call in (e.getState, e.getJerk, e.info):
        with pytest.raises(nb.StateException, match="not primed"):
            call()
    e.advance(d, 0)  # (macro_steps <= 0 does nothing)
    e.invalidate()
    assert e._h is None
    e.close()
    assert "hermite_batch" in nb._lib.CLOSE_ORDER
    assert nb._lib.CLOSE_ORDER.index("hermite_batch") < nb._lib.CLOSE_ORDER.index("context")


def test_null_handle_is_a_state_error(nb):
    lib = nb._lib.load()
    mode = C.c_int(7)
    off = np.array([0, 4], np.uint64)
    s = nb._lib.ParticleDataStruct()
    dt = np.array([0.1], np.float32)
    info = nb._lib.HermiteBlockInfoStruct()
    calls = (lambda: lib.nbody_hip_hermite_batch_set_params(None, 0.02, 0.01, 16),
             lambda: lib.nbody_hip_hermite_batch_set_precision(None, 1),
             lambda: lib.nbody_hip_hermite_batch_get_precision(None, C.byref(mode)),
             lambda: lib.nbody_hip_hermite_batch_set_layout(None, off.ctypes.data, 1),
             lambda: lib.nbody_hip_hermite_batch_prime(None, C.byref(s), 1.0, 0.1, dt.ctypes.data),
             lambda: lib.nbody_hip_hermite_batch_invalidate(None),
             lambda: lib.nbody_hip_hermite_batch_advance(None, C.byref(s), 1),
             lambda: lib.nbody_hip_hermite_batch_state(None, None, None, None, None),
             lambda: lib.nbody_hip_hermite_batch_info(None, -1, C.byref(info)),
             lambda: lib.nbody_hip_hermite_batch_set_state_f64(None, C.byref(s), None, None),
             lambda: lib.nbody_hip_hermite_batch_get_state_f64(None, C.byref(s), None, None))
    for call in calls:
        assert call() == nb._lib.ERR_STATE
        assert b"null block-step Hermite ensemble" in lib.nbody_hip_last_error()
    assert mode.value == 7
    h = C.c_void_p(1)
    assert lib.nbody_hip_hermite_batch_create(None, 16, 2, C.byref(h)) == nb._lib.ERR_STATE and not h.value
    assert b"null context" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_hermite_batch_destroy(None) == nb._lib.OK


def test_prototypes_are_bound_and_declared(nb):
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    lib = nb._lib.load()
    for name in NAMES:
        sym = "nbody_hip_hermite_batch_" + name
        assert sym in nb._lib.PROTOTYPES, sym
        assert getattr(lib, sym).argtypes == nb._lib.PROTOTYPES[sym][1]
        assert len(re.findall(rf"^NBODY_HIP_API int {sym}\(", header, re.M)) == 1, sym
    declared = set(re.findall(r"\b(nbody_hip_hermite_batch_\w+)\(", header))
    assert declared == {"nbody_hip_hermite_batch_" + n for n in NAMES}
    assert "typedef struct nbody_hip_hermite_batch nbody_hip_hermite_batch;" in header
    assert len(re.findall(r"^#define NBODY_HIP_ABI_VERSION 1\s*$", header, re.M)) == 1
    assert nb.BlockHermiteEnsemble is nb.api.BlockHermiteEnsemble and callable(nb.ic.concat)


def test_the_triple_ensemble_has_many_schedules():
    """the property tests/test_hermite_batch_gpu.py asserts of its 300 systems, on the inputs: by the restatement of the
    scheme the systems do not share one schedule"""
    c = bc.TRIPLE
    steps = set()
    for ic in bc.triples(c["systems"]):
        pos, vel, m = bc.arrays_of(ic)
        assert pos.shape == (3, 3) and pos.dtype == np.float32 and m.shape == (3,)
        steps.add(br.block_steps(pos, vel, m, c["G"], c["eps"], c["dt_max"], 2, max_level=c["max_level"])["block_steps"])
    assert len(steps) >= 5, sorted(steps)
    # seeded: the same systems every time
    a, b = bc.triples(3), bc.triples(3)
    assert all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in x)
