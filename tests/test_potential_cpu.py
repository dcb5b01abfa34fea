"""Per-body potential (nbody_hip_{direct,tree,grid}_potential): the declarations of every layer and the fp64
restatement the GPU tests compare against.  No GPU needed."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import potential_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("nbody_hip_direct_potential", "nbody_hip_tree_potential", "nbody_hip_grid_potential")


def test_header_declares_and_prototypes_bind_the_potential_calls(nb):
    src = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for name in NAMES:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        args = m.group(1)
        assert "float* phi" in args and "double* pe" in args and "float eps" in args, args
    for name in NAMES:
        res, args = nb._lib.PROTOTYPES[name]
        assert res is not None and len(args) == (6 if name == "nbody_hip_direct_potential" else 7)
    assert re.search(r"#define NBODY_HIP_ABI_VERSION 1\b", src)


def test_python_methods_have_the_documented_signatures(nb):
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(nb.ForceCalculator.computePotential) == ["self", "d_particles", "phi"]
    assert sig(nb.BarnesHutTree.computePotential) == ["self", "d_particles", "theta", "G", "eps", "phi"]
    assert sig(nb.SpatialHashGrid.computePotential) == ["self", "d_particles", "cutoff", "G", "eps", "phi"]
    for cls in (nb.DirectForceCalculator, nb.BarnesHutCalculator, nb.SpatialHashCalculator):
        assert sig(cls.computePotential) == ["self", "d_particles", "phi"]
    assert nb.BarnesHutCalculator.computePotential is not nb.ForceCalculator.computePotential
    assert nb.SpatialHashCalculator.computePotential is not nb.ForceCalculator.computePotential
    for name in ("computeMethodPotentialEnergy", "computeMethodTotalEnergy", "getPotential"):
        assert callable(getattr(nb.ParticleSystem, name))


def test_fp64_restatement_reproduces_the_fixture_pe():
    z = np.load(os.path.join(GOLDEN, "plummer4096_direct.npz"))
    pos = np.stack([z["pos_x"], z["pos_y"], z["pos_z"]], 1)
    phi = pr.direct_phi(pos, z["mass"], float(z["G"]), float(z["eps"]))
    pe = 0.5 * (z["mass"].astype(np.float64) * phi).sum()
    assert float(z["pe"]) == -0.30456890846407947
    assert abs(pe - float(z["pe"])) <= 1e-12 * abs(float(z["pe"]))


def test_shifted_pair_term_is_continuous_at_the_cutoff():
    for rc, eps in ((1.0, 0.01), (2.0, 0.0), (0.5, 0.1)):
        rc2 = float(np.float32(rc) * np.float32(rc))
        inside = pr.shifted_term(np.nextafter(rc2, 0.0), rc, eps)
        at = pr.shifted_term(rc2, rc, eps)
        assert at == 0.0
        assert 0.0 <= inside < 1e-12
        # and it decreases towards the cutoff
        r2 = np.linspace(0.25, 1.0, 50) * rc2
        assert np.all(np.diff(pr.shifted_term(r2, rc, eps)) < 0)


def test_hash_restatement_on_two_bodies():
    pos = np.array([[0.0, 0.0, 0.0], [0.6, 0.0, 0.0]], np.float32)
    m = np.array([1.0, 2.0], np.float32)
    phi, scale = pr.hash_phi(pos, m, 1.0, 0.01, 1.0, cell_of=[0, 0], dims=(2, 2, 2))
    r2 = float(pr.fp32_dist2(np.float32(0.6), np.float32(0), np.float32(0)))
    assert phi[0] == pytest.approx(-2.0 * pr.shifted_term(r2, 1.0, 0.01), rel=1e-15)
    assert scale[0] == pytest.approx(2.0 / np.sqrt(r2 + float(np.float32(0.01) ** 2)), rel=1e-15)
    phi, _ = pr.hash_phi(pos, m, 1.0, 0.01, 0.5, cell_of=[0, 0], dims=(2, 2, 2))  # outside the cutoff
    assert phi[0] == 0.0


def test_facade_header_declares_the_potential_entry_points():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    inc = os.path.join(ROOT, "n-body_amd", "facade", "include")
    src = ("#include \"nbody_facade.hpp\"\n"
           "double (nbody::BarnesHutTree::*t)(const nbody::ParticleData*, float, float, float, float*) = "
           "&nbody::BarnesHutTree::computePotential;\n"
           "double (nbody::SpatialHashGrid::*g)(const nbody::ParticleData*, float, float, float, float*) = "
           "&nbody::SpatialHashGrid::computePotential;\n"
           "double (*f)(nbody::ForceCalculator&, nbody::ParticleData*, float*) = &nbody::computePotential;\n"
           "static_assert(sizeof(nbody::BarnesHutTree) == 96 && sizeof(nbody::SpatialHashGrid) == 96, \"layout\");\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
