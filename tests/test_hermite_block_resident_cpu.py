"""Resident scheduling of the block-step Hermite integrator, the parts that need no GPU: the names the two Python setters
take, the null-handle answers of the two entry points, and the constants of include/nbody_hip.h against the module's."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    src = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    got = re.findall(rf"^#define {name} (\d+)\s*$", src, re.M)
    assert len(got) == 1, name
    return int(got[0])


def test_integrator_scheduling_names(nb):
    b = nb.BlockHermiteIntegrator()
    assert b.getScheduling() == ("host", None)
    for name in ("host", "resident", "auto"):
        b.setScheduling(name)  # remembered before the handle exists, like setTuning
        assert b.getScheduling() == (name, None)
    for bad in ("Resident", "device", "", None, 1, b"host"):
        with pytest.raises(nb.ValidationException, match="scheduling must be one of"):
            b.setScheduling(bad)
    assert b.getScheduling() == ("auto", None) and b._h is None


def test_particle_system_scheduling_names(nb):
    ps = nb.ParticleSystem()
    assert ps.getHermiteBlockScheduling() == "host"
    for name in ("resident", "auto", "host"):
        ps.setHermiteBlockScheduling(name)
        assert ps.getHermiteBlockScheduling() == name
    for bad in ("HOST", "gpu", None, 2):
        with pytest.raises(nb.ValidationException, match="scheduling must be one of"):
            ps.setHermiteBlockScheduling(bad)
    assert ps.getHermiteBlockScheduling() == "host" and ps.hermite_block_ is None
    # like the state precision: not a field of the configuration
    assert not any("sched" in f for f in vars(nb.SimulationConfig()))


def test_null_handle_is_a_state_error(nb):
    lib = nb._lib.load()
    mode, form = C.c_int(7), C.c_int(7)
    assert lib.nbody_hip_hermite_block_set_scheduling(None, 1) == nb._lib.ERR_STATE
    assert b"null block-step Hermite integrator" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_hermite_block_get_scheduling(None, C.byref(mode), C.byref(form)) == nb._lib.ERR_STATE
    assert b"null block-step Hermite integrator" in lib.nbody_hip_last_error()
    assert (mode.value, form.value) == (7, 7)


def test_header_constants_match_the_module(nb):
    from nbody_amd import api
    assert _header_constant("NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX") == api.HERMITE_BLOCK_RESIDENT_MAX == 4096
    below = _header_constant("NBODY_HIP_HERMITE_BLOCK_RESIDENT_BELOW")
    assert below == api.HERMITE_BLOCK_RESIDENT_BELOW
    assert 0 <= below <= api.HERMITE_BLOCK_RESIDENT_MAX + 1  # (0: the automatic choice never takes the resident form)
