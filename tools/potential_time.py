"""Per-body potential calls against the force call and the O(N^2) Direct PE, ms per call (median of 5, host clock
around work that ends in a device synchronise).

  bh    config 4 (two galaxies, 2^20 bodies, theta 0.5, eps 0.1) and 8,388,608 bodies
  hash  config 5 (uniform box at 16 bodies per unit volume, 4,194,304 bodies, cell = cutoff = 1, eps 0.01) and 16,777,216
  crossover  Barnes-Hut phi walk (tree built) against the Direct phi at 10^4 and 10^5 bodies (Plummer, theta 0.5)

The tree / grid is built once per size; "force" is the force call on it, "potential" the potential call on it (phi and
PE), "direct pe" nbody_hip_potential_energy_f64 (the triangular O(N^2) sweep).
usage: python tools/potential_time.py [--small] [--no-direct]
  --small      configs 4 and 5 and the crossover only (the rocprofv3 run)
  --no-direct  skip the Direct PE (it takes ~8 s at 8 M bodies and ~32 s at 16 M)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbody_amd as nb  # noqa: E402
from gpu_util import to_device  # noqa: E402


def ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def case(kind, n, direct):
    if kind == "bh":
        ic, G, eps, theta = nb.ic.two_galaxies(n, seed=42), 1.0, 0.1, 0.5
        d, _ = to_device(nb, ic)
        s = nb.BarnesHutTree(n)
        s.build(d)
        force = lambda: s.computeForces(d, theta, G, eps)  # noqa: E731
        pot = lambda phi: s.computePotential(d, theta, G, eps, phi)  # noqa: E731
        what = f"Barnes-Hut two galaxies theta {theta} eps {eps}"
    else:
        half = 0.5 * (n / 16.0) ** (1.0 / 3.0)
        ic, G, eps, cutoff = nb.ic.uniform_box(n, seed=42, lo=-half, hi=half), 1.0, 0.01, 1.0
        d, _ = to_device(nb, ic)
        s = nb.SpatialHashGrid(n, 1.0)
        s.build(d)
        force = lambda: s.computeForces(d, cutoff, G, eps)  # noqa: E731
        pot = lambda phi: s.computePotential(d, cutoff, G, eps, phi)  # noqa: E731
        what = f"spatial hash uniform box cell 1 cutoff {cutoff} eps {eps}"
    phi = torch.empty(n, dtype=torch.float32, device="cuda")
    t_force = ms(force)
    t_pot = ms(lambda: pot(phi))
    t_pe_only = ms(lambda: pot(None))
    line = (f"{what}, N={n}: force {t_force:.3f} ms, potential (phi + PE) {t_pot:.3f} ms, PE only {t_pe_only:.3f} ms, "
            f"PE {pot(None):.9e}")
    if direct:
        integ = nb.Integrator()
        t0 = time.perf_counter()
        _, pe = integ.computeEnergiesF64(d, G, eps)
        t_direct = 1e3 * (time.perf_counter() - t0)
        line += f"; direct PE (one call) {t_direct:.1f} ms = {t_direct / t_pot:.0f} x the potential call (PE {pe:.9e})"
    print(line, flush=True)


def crossover():
    for n in (10000, 100000):
        d, _ = to_device(nb, nb.ic.plummer(n, seed=1))
        tree = nb.BarnesHutTree(n)
        tree.build(d)
        fc = nb.DirectForceCalculator()
        fc.setSofteningParameter(0.01)
        phi = torch.empty(n, dtype=torch.float32, device="cuda")
        t_bh = ms(lambda: tree.computePotential(d, 0.5, 1.0, 0.01, phi))
        t_dir = ms(lambda: fc.computePotential(d, phi))
        t_force = ms(lambda: tree.computeForces(d, 0.5, 1.0, 0.01))
        print(f"crossover N={n}: Barnes-Hut phi (theta 0.5, tree built) {t_bh:.3f} ms, Direct phi {t_dir:.3f} ms, "
              f"Barnes-Hut force walk {t_force:.3f} ms", flush=True)
    d, _ = to_device(nb, nb.ic.plummer(1 << 20, seed=1))
    fc = nb.DirectForceCalculator()
    fc.setSofteningParameter(0.01)
    phi = torch.empty(1 << 20, dtype=torch.float32, device="cuda")
    print(f"Direct phi N={1 << 20}: {ms(lambda: fc.computePotential(d, phi), reps=3):.1f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-direct", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    case("bh", 1 << 20, not a.no_direct)
    case("hash", 4194304, not a.no_direct)
    crossover()
    if not a.small:
        case("bh", 8388608, not a.no_direct)
        case("hash", 16777216, not a.no_direct)


if __name__ == "__main__":
    main()
