"""Field at arbitrary points (nbody_hip_{direct,tree,grid}_field): the declarations of every layer and the fp64
restatements the GPU tests compare against (tests/field_ref.py).  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import field_ref as fr
import quadrupole_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nbody_hip_direct_field", "nbody_hip_tree_field", "nbody_hip_grid_field")


def test_header_declares_and_prototypes_bind_the_field_calls(nb):
    src = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for name in NAMES:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        args = " ".join(m.group(1).split())
        assert "const nbody_float4* points" in args and "size_t n_points" in args and "nbody_float4* out" in args, args
        assert "float eps" in args and "eps2" not in args, args
    assert "no reference counterpart" in src[src.index("ARBITRARY POINTS") - 80:src.index("ARBITRARY POINTS")]
    for name in NAMES:
        res, args = nb._lib.PROTOTYPES[name]
        assert res is not None and len(args) == 7
    assert re.search(r"#define NBODY_HIP_ABI_VERSION 1\b", src)


def test_python_methods_have_the_documented_signatures(nb):
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(nb.ForceCalculator.computeField) == ["self", "d_particles", "points", "out"]
    assert sig(nb.BarnesHutTree.computeField) == ["self", "points", "theta", "G", "eps", "out"]
    assert sig(nb.SpatialHashGrid.computeField) == ["self", "points", "cutoff", "G", "eps", "out"]
    for cls in (nb.DirectForceCalculator, nb.BarnesHutCalculator, nb.SpatialHashCalculator):
        assert sig(cls.computeField) == ["self", "d_particles", "points", "out"]
    assert nb.DirectForceCalculator.computeField is nb.ForceCalculator.computeField
    assert nb.BarnesHutCalculator.computeField is not nb.ForceCalculator.computeField
    assert nb.SpatialHashCalculator.computeField is not nb.ForceCalculator.computeField
    assert sig(nb.ParticleSystem.computeFieldAt) == ["self", "points", "out"]


def test_facade_declares_the_field_calls():
    hpp = open(os.path.join(ROOT, "n-body_amd", "facade", "include", "nbody_facade.hpp")).read()
    assert len(re.findall(r"void computeField\(const float4\* d_points, size_t n, float \w+, float G, float eps, "
                          r"float4\* d_out\);", hpp)) == 2
    assert re.search(r"^void computeField\(ForceCalculator& force_calc, ParticleData\* d_particles, const float4\* d_points, "
                     r"size_t n,\s*float4\* d_out\);", hpp, re.M)
    mk = open(os.path.join(ROOT, "n-body_amd", "facade", "Makefile")).read()
    assert "tests/field_tests.cpp" in mk and "$(LIBDIR)/field_tests" in mk.split("\n\n")[1]


# ---- known answers of the restatements ------------------------------------------------------------------------------
def test_one_body_known_answer():
    G, M, eps = 1.5, 2.0, 0.1
    x = np.array([[0.5, 0.0, 0.0], [0.0, -1.25, 0.0], [0.3, 0.4, 1.2], [0.0, 0.0, 0.0]], np.float32)
    a, phi, S = fr.direct_field(x, [[0.0, 0.0, 0.0]], [M], G, eps)
    x64 = x.astype(np.float64)
    r2 = (x64 ** 2).sum(1)
    e2 = float(np.float32(eps) ** 2)
    assert np.allclose(a, -G * M * x64 * ((r2 + e2) ** -1.5)[:, None], rtol=1e-14, atol=0)
    assert np.allclose(phi, -G * M * (r2 + e2) ** -0.5, rtol=1e-14, atol=0)
    assert np.allclose(S, np.linalg.norm(a, axis=1), rtol=1e-12)
    # the coincident body: no force, -G M / eps in phi; nothing of either under the guard convention
    assert not a[3].any() and phi[3] == pytest.approx(-G * M / np.sqrt(e2), rel=1e-14)
    a0, phi0, _ = fr.direct_field(x[3:], [[0.0, 0.0, 0.0]], [M], G, 0.0)
    assert not a0.any() and phi0[0] == 0.0
    # the hash: the same force inside the cutoff, phi shifted to zero at it, nothing beyond
    ah, ph, _, _ = fr.hash_field_all(x, [[0.0, 0.0, 0.0]], [M], G, eps, 1.0)
    inside = r2 < 1.0
    assert np.allclose(ah[inside], a[inside], rtol=1e-14) and not ah[~inside].any() and not ph[~inside].any()
    assert np.allclose(ph[inside], phi[inside] + G * M / np.sqrt(1.0 + e2), rtol=1e-13)


def test_two_equal_bodies_cancel_at_the_midpoint():
    pos = np.array([[-0.5, 0.25, 1.0], [0.5, -0.25, -1.0]], np.float32)
    a, phi, S = fr.direct_field(np.zeros((1, 3), np.float32), pos, [2.0, 2.0], 1.0, 0.1)
    assert np.abs(a).max() <= 1e-15 * S[0] and S[0] > 0
    assert phi[0] == pytest.approx(-4.0 / np.sqrt(1.3125 + float(np.float32(0.1) ** 2)), rel=1e-14)


def _central_gradient(f, x, h=1e-5):
    g = np.zeros(3)
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        g[a] = (f(x + e) - f(x - e)) / (2 * h)
    return g


def test_direct_restatement_gradient():
    rng = np.random.default_rng(1)
    pos = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    m = rng.uniform(0.5, 2.0, 40)
    for x in rng.uniform(-1.5, 1.5, (8, 3)):
        # (the restatement takes fp32 points: evaluate the fp64 formula it states at unrounded positions)
        def phi_at(y):
            d = pos.astype(np.float64) - y[None, :]
            return -1.3 * (m / np.sqrt((d * d).sum(1) + float(np.float32(0.05) ** 2))).sum()
        x32 = x.astype(np.float32).astype(np.float64)
        a, phi, _ = fr.direct_field(x32[None, :], pos, m, 1.3, 0.05)
        assert phi[0] == pytest.approx(phi_at(x32), rel=1e-14)
        g = _central_gradient(phi_at, x32)
        assert np.linalg.norm(g + a[0]) <= 1e-7 * np.linalg.norm(a[0])


@pytest.mark.parametrize("order", [1, 2])
def test_accepted_node_gradient(order):
    """node_eval (what tree_field evaluates an accepted node with): grad phi = -a by fp64 central differences"""
    rng = np.random.default_rng(2)
    bodies = rng.normal(0, 0.2, (30, 3))
    m = rng.uniform(0.5, 2.0, 30)
    M, c, S = qr.moments_of(bodies, m)
    eps = 0.05
    for x in rng.normal(0, 1, (8, 3)) + 2.0:
        def phi_at(y):
            _, p = qr.single_node((c - y)[None, :], eps, M, S, order)
            return float(p[0])
        a, _ = qr.single_node((c - x)[None, :], eps, M, S, order)
        g = _central_gradient(phi_at, x)
        assert np.linalg.norm(g + a[0]) <= 1e-7 * np.linalg.norm(a[0])


def test_hash_window_equals_the_truncated_sum_when_cutoff_fits_the_cell():
    rng = np.random.default_rng(3)
    n, cell, G, eps = 600, 1.0, 1.0, 0.01
    pos = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    m = rng.uniform(0.5, 2.0, n)
    lo = pos.min(0) - np.float32(0.001)
    hi = pos.max(0) + np.float32(0.001)
    dims = [int(np.ceil(np.float32(hi[a] - lo[a]) / np.float32(cell))) + 1 for a in range(3)]
    cell_of = fr.hash_cells(pos, lo, cell, dims)
    inside = rng.uniform(-3, 3, (150, 3))
    faces = rng.uniform(-3, 3, (60, 3))
    fa = rng.integers(0, 3, 60)  # one coordinate ON a face of the grid's box
    faces[np.arange(60), fa] = np.where(rng.random(60) < 0.5, lo[fa], hi[fa])
    lattice = lo[None, :].astype(np.float64) + cell * rng.integers(0, 6, (40, 3))  # on cell boundaries
    outside = rng.uniform(-3, 3, (100, 3))
    ax = rng.integers(0, 3, 100)
    outside[np.arange(100), ax] = np.where(rng.random(100) < 0.5, -3.0 - rng.uniform(0, 1.5, 100), 3.0 + rng.uniform(0, 1.5, 100))
    pts = np.concatenate([inside, faces, lattice, outside]).astype(np.float32)
    for cutoff in (1.0, 0.6):
        pc = fr.hash_cells(pts, lo, cell, dims)
        aw, pw, Sw, _ = fr.hash_field(pts, pc, pos, m, G, eps, cutoff, cell_of, dims)
        aa, pa, Sa, _ = fr.hash_field_all(pts, pos, m, G, eps, cutoff)
        assert np.array_equal(aw != 0, aa != 0)
        assert np.allclose(aw, aa, rtol=1e-12, atol=1e-12 * Sa.max())
        assert np.allclose(pw, pa, rtol=1e-12, atol=1e-12)
        assert (Sa[: len(inside)] > 0).sum() > 100  # the comparison is not empty
    # the bodies' own cells: a body is in the cell the grid put it in
    assert np.array_equal(fr.hash_cells(pos, lo, cell, dims), cell_of)
    # non-finite and far points clamp into the grid
    far = np.array([[1e30, -1e30, 0.0], [np.inf, 0.0, 0.0], [np.nan, 0.0, 0.0]], np.float32)
    pc = fr.hash_cells(far, lo, cell, dims)
    assert ((pc >= 0) & (pc < dims[0] * dims[1] * dims[2])).all()
