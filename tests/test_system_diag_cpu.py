"""The ensemble diagnostics without a GPU: the CPU check of the shared arithmetic (make diag_check: system_diag_common.h
under AddressSanitizer and UBSan against a long double restatement, and the kernel's pair enumeration at every size class),
the layout of the struct in ctypes and numpy, the declarations, the null-handle answers and the Python-side argument checks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import system_diag_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
NAMES = ("nbody_hip_systems_diagnostics", "nbody_hip_hermite_batch_diagnostics", "nbody_hip_hermite_block_diagnostics")


def test_diag_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "diag_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "system_diag_check: ok" in r.stdout and "FAIL" not in r.stdout
    assert "-fsanitize=address,undefined" in r.stdout or os.path.exists(os.path.join(ROOT, "n-body_amd", "lib", "system_diag_check"))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/system_diag_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert "system_diag.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)


def test_the_shared_header_is_plain_cxx_and_the_kernel_uses_it():
    common = open(os.path.join(CSRC, "system_diag_common.h")).read()
    code = re.sub(r"//.*", "", common)
    for word in ("__shfl", "__builtin_amdgcn", "threadIdx", "__shared__", "__syncthreads", "hip_runtime", "float2", "rsq"):
        assert word not in code, word
    kernel = open(os.path.join(CSRC, "system_diag.hip")).read()
    for fn in ("diag_body(", "diag_body_add(", "diag_pair(", "diag_min_take(", "diag_row_runs(", "diag_finish("):
        assert fn in common and fn in kernel + open(os.path.join(CSRC, "system_diag_check.cpp")).read(), fn
    assert "atomic" not in re.sub(r"//.*", "", kernel)        # no atomics (the comments say so too)
    assert "readfirstlane" in kernel


def test_struct_layout(nb):
    S = nb._lib.SystemDiagStruct
    assert C.sizeof(S) == 152 == nb.SYSTEM_DIAG_BYTES == nb.SYSTEM_DIAG_DTYPE.itemsize
    want = dict(mass=0, com=8, momentum=32, ang_mom=56, kinetic=80, potential=88, min_sep=96, bind_energy=104, bind_a=112,
                bind_e=120, min_i=128, min_j=132, bind_i=136, bind_j=140, n=144, status=148)
    assert [f for f, _ in S._fields_] == list(want)
    for name, off in want.items():
        assert getattr(S, name).offset == off, name
        assert nb.SYSTEM_DIAG_DTYPE.fields[name][1] == off, name
    # the header states the same struct, field for field and in this order
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    body = header[header.index("typedef struct nbody_hip_system_diag {"):header.index("} nbody_hip_system_diag;")]
    decl = re.findall(r"^\s*(?:double|int)\s+([^;]+);", body, re.M)
    names = [n.strip().split("[")[0] for d in decl for n in d.split(",")]
    assert names == list(want)


def test_header_declares_and_prototypes_bind_the_entry_points(nb):
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    # (the model, the struct and the generic call are in nbody_hip.h, the two calls on integrator handles in nbody_hip_diag.h)
    handles = open(os.path.join(ROOT, "include", "nbody_hip_diag.h")).read()
    assert '#include "nbody_hip.h"' in handles and "#define NBODY_HIP_ABI_VERSION" not in handles
    assert NAMES[0] + "(" in header and all(n + "(" in handles and n + "(" not in header for n in NAMES[1:])
    header = header + handles
    lib = nb._lib.load()
    for name in NAMES:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, name
        args = " ".join(m.group(1).split())
        res, argtypes = nb._lib.PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == len(args.split(",")), name
        assert "eps2" not in args
        assert getattr(lib, name).argtypes == argtypes
    one = lambda name: " ".join(re.search(name + r"\s*\(([^)]*)\)", header).group(1).split())  # noqa: E731
    assert ("const nbody_float4* pos_lo_or_null, const nbody_float4* vel_lo_or_null, const unsigned long long* offsets_device, "
            "size_t n_systems, float G, float eps, nbody_hip_system_diag* out_device") in one(NAMES[0])
    assert re.search(r"#define NBODY_HIP_ABI_VERSION 1\b", header)
    doc = header[header.index("ensemble DIAGNOSTICS"):header.index("NBODY_HIP_API int nbody_hip_systems_diagnostics")]
    for phrase in ("exact fp64 sums", "eps2 = (double)(eps * eps)", "correctly rounded sqrt and /", "UNSOFTENED",
                   "lexicographically smallest (i, j)", "There are no atomics", "bitwise reproducible", "/* 152 bytes */"):
        assert phrase in doc, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.14" in design and "system_diag_kernel" in design


def test_null_handles_are_answered_without_a_device(nb):
    lib = nb._lib.load()
    s = nb._lib.ParticleDataStruct()
    out = (C.c_char * 152)()
    off = (C.c_ulonglong * 2)(0, 1)
    ST = nb._lib.ERR_STATE
    assert lib.nbody_hip_systems_diagnostics(None, C.byref(s), None, None, off, 1, 1.0, 0.1, out) == ST
    assert b"null context" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_hermite_batch_diagnostics(None, C.byref(s), out) == ST
    assert b"null block-step Hermite ensemble" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_hermite_block_diagnostics(None, C.byref(s), 1.0, 0.1, out) == ST
    assert b"null block-step Hermite integrator" in lib.nbody_hip_last_error()
    assert not any(out.raw)


def test_python_signatures_and_argument_checks(nb):
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(nb.systems_diagnostics) == ["ctx", "d_particles", "offsets", "G", "eps", "pos_lo", "vel_lo"]
    assert sig(nb.systems_diagnostics_into)[:6] == ["ctx", "d_particles", "offsets", "G", "eps", "out"]
    assert sig(nb.BlockHermiteEnsemble.diagnostics) == ["self", "d_particles"]
    assert sig(nb.BlockHermiteEnsemble.diagnostics_into) == ["self", "d_particles", "out"]
    assert sig(nb.BlockHermiteIntegrator.diagnostics) == ["self", "d_particles", "force_calc"]
    assert sig(nb.BlockHermiteIntegrator.diagnostics_into) == ["self", "d_particles", "force_calc", "out"]
    import torch
    cpu = torch.device("cpu")
    api = nb.api
    with pytest.raises(nb.ValidationException, match="one-dimensional"):
        api._diag_offsets([[0, 1]], cpu)
    with pytest.raises(nb.ValidationException, match="integers"):
        api._diag_offsets([0.0, 1.0], cpu)
    with pytest.raises(nb.ValidationException, match=r"\[0, 2\^62\]"):
        api._diag_offsets([0, -1], cpu)
    with pytest.raises(nb.ValidationException, match="int64"):
        api._diag_offsets(torch.zeros(3, dtype=torch.int32), cpu)
    assert api._diag_offsets(np.array([0, 3, 7], np.uint64), cpu).tolist() == [0, 3, 7]
    good = nb.system_diag_tensor(3, cpu)
    assert good.shape == (3, 152) and api._diag_out(good, 3, cpu) is good
    with pytest.raises(nb.ValidationException, match="hold 2 x 152 bytes"):
        api._diag_out(good, 2, cpu)
    with pytest.raises(nb.ValidationException, match="torch tensor"):
        api._diag_out(np.zeros(152, np.uint8), 1, cpu)
    with pytest.raises(nb.ValidationException, match="contiguous float32 tensor of shape \\(5, 4\\)"):
        api._diag_lo("pos_lo", torch.zeros((5, 3)), 5, cpu)
    assert api._diag_lo("pos_lo", None, 5, cpu) is None
    rows = nb.system_diag_array(good)
    assert rows.dtype == nb.SYSTEM_DIAG_DTYPE and rows.shape == (3,)
    with pytest.raises(nb.StateException, match="not primed"):
        nb.BlockHermiteEnsemble().diagnostics(None)
    facade = open(os.path.join(ROOT, "n-body_amd", "facade", "include", "nbody_facade.hpp")).read()
    assert "void diagnostics(ParticleData* d_particles, SystemDiag* h_out);" in facade
    assert "void diagnostics(ParticleData* d_particles, ForceCalculator* force_calc, SystemDiag* h_out);" in facade
    mk = open(os.path.join(ROOT, "n-body_amd", "facade", "Makefile")).read()
    assert "$(LIBDIR)/system_diag_tests: tests/system_diag_tests.cpp $(LIB)" in mk


def test_the_reference_and_the_chain_lengths():
    # the restatement against closed forms: an equal-mass circular binary of separation 1 (G = 1, m = 1/2 each, relative
    # speed sqrt(G M / r) = 1)
    X = np.array([[-0.5, 0, 0], [0.5, 0, 0]])
    V = np.array([[0, -0.5, 0], [0, 0.5, 0]])
    r = sr.reference(X, V, [0.5, 0.5], 1.0, 0.0)
    assert r["potential"] == -0.25 and r["kinetic"] == 0.125 and (r["min_i"], r["min_j"], r["min_sep"]) == (0, 1, 1.0)
    assert (r["bind_i"], r["bind_j"], r["bind_energy"], r["bind_a"], r["bind_e"]) == (0, 1, -0.125, 1.0, 0.0)
    assert list(r["ang_mom"]) == [0, 0, 0.25] and list(r["com"]) == [0, 0, 0] and r["mass"] == 1.0
    # ... and with the speeds halved it falls from apocentre: E_b = 1/32 - 1/4, a = 4/7, e = r / a - 1 = 3/4
    r = sr.reference(X, 0.5 * V, [0.5, 0.5], 1.0, 0.0)
    assert r["bind_energy"] == 1 / 32 - 1 / 4 and abs(r["bind_a"] - 4 / 7) < 1e-15 and abs(r["bind_e"] - 0.75) < 1e-15
    # L(n) stays inside the cap the design states, at every size
    for n in range(1, 4097):
        assert sr.chain_pairs(n) <= n * n / 512 + 64 and sr.chain_bodies(n) <= 25
    assert sr.chain_pairs(4096) == 32769 and sr.chain_pairs(64) == 17 and sr.chain_pairs(1) == 9
