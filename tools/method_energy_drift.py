"""Energy drift with the force method's own PE at a size the O(N^2) PE cannot reach in useful time: Barnes-Hut, two
galaxies (unit total mass), 8,388,608 bodies, theta 0.5, eps 0.1, dt 1e-3, 2,000 Velocity-Verlet steps, KE (fp64) +
BarnesHutCalculator.computePotential sampled every 100 steps.  Prints per sample the energies, |E - E0| / |E0|,
|E - E0| / |PE0| and the time of the PE sample (host clock; the call blocks).
usage: python tools/method_energy_drift.py [n] [steps] [every]
"""
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8388608
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    G, eps, theta, dt = 1.0, 0.1, 0.5, 1e-3
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    ic = nb.ic.two_galaxies(n, seed=42)
    ic["mass"] = (ic["mass"] / np.float32(n)).astype(np.float32)  # unit total mass
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(theta)
    calc.setGravitationalConstant(G)
    calc.setSofteningParameter(eps)
    integ = nb.Integrator()
    calc.computeForces(d)

    def sample():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pe = calc.computePotential(d)
        t_pe = 1e3 * (time.perf_counter() - t0)
        return integ.computeKineticEnergyF64(d), pe, t_pe

    ke0, pe0, t_pe = sample()
    e0 = ke0 + pe0
    print(f"Barnes-Hut two galaxies N={n} theta {theta} eps {eps} dt {dt}: method PE sampled every {every} steps", flush=True)
    print(f"step {0:5d}  KE {ke0:.10e}  PE {pe0:.10e}  E {e0:.10e}  PE sample {t_pe:.2f} ms (tree build + walk + sum)",
          flush=True)
    worst, t_steps = 0.0, 0.0
    for s in range(every, steps + 1, every):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        integ.integrate_steps(d, calc, dt, every)
        torch.cuda.synchronize()
        t_steps += time.perf_counter() - t0
        ke, pe, t_pe = sample()
        e = ke + pe
        worst = max(worst, abs(e - e0) / abs(pe0))
        print(f"step {s:5d}  KE {ke:.10e}  PE {pe:.10e}  E {e:.10e}  |dE|/|E0| {abs(e - e0) / abs(e0):.3e}  "
              f"|dE|/|PE0| {abs(e - e0) / abs(pe0):.3e}  PE sample {t_pe:.2f} ms", flush=True)
    print(f"max |E - E0| / |PE0| over {steps} steps: {worst:.3e}; {1e3 * t_steps / steps:.3f} ms per step", flush=True)


if __name__ == "__main__":
    main()
