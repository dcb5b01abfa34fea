"""Barnes-Hut multipole order 1 against order 2 (nbody_hip_tree_set_multipole_order): accuracy against Direct and cost.

  table  (default) config 4 (two galaxies, 2^20 bodies, eps 0.1) and a 2^20 Plummer (eps 0.01), theta in {0.3, 0.5,
         0.7, 0.9}, both orders: build ms, walk ms and full step ms (torch device events on the stream the library
         uses, warm, mean of `iters`), force relative error against Direct (median / p99 / rms), phi rms relative error
         and |dPE| / |PE|
  drift  energy drift of both orders: config-4 ICs (unit total mass) at 2^17 bodies, theta 0.5, eps 0.1, dt 1e-3,
         2,000 steps, KE + the exact fp64 pair PE (Integrator.computeEnergiesF64) every 100 steps
  step   one warm order-2 config-4 step (build + walk + kick / drift), for a kernel trace:
         rocprofv3 --kernel-trace --stats -d DIR -o step -- python tools/bh_quadrupole_sweep.py step [order] --out -
  stats  the kernel statistics of such a trace from rocprofv3's database (DIR/step_results.db): per kernel the
         dispatches, mean and total us, VGPRs / SGPRs / scratch; and whether the trace holds an order-2 kernel
Every line printed is also appended to --out (default profiles/r05_bh_quadrupole.txt; '-' = stdout only).
usage: python tools/bh_quadrupole_sweep.py [table|drift|step [order]|stats DB [label]] [--out FILE] [--iters K]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbody_amd as nb  # noqa: E402
from gpu_util import acc_of, rel_err, to_device  # noqa: E402

OUT = [None]


def say(line):
    print(line, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(line + "\n")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms


def population(which):
    if which == "config4":
        return nb.ic.two_galaxies(1 << 20, seed=42), 1.0, 0.1
    return nb.ic.plummer(1 << 20, seed=42), 1.0, 0.01


def table(iters):
    say("# theta x multipole order, 2^20 bodies (MI355X): times in ms (device events, warm, mean of %d); errors against "
        "Direct (per-body |a - a_D| / |a_D|; phi: rms of (phi - phi_D) / |phi_D|)" % iters)
    say(f"{'population':<10} {'theta':>5} {'order':>5} {'build':>7} {'walk':>7} {'step':>7} {'median':>10} {'p99':>10} "
        f"{'rms':>10} {'phi_rms':>10} {'dPE/PE':>10}")
    for which in ("config4", "plummer"):
        ic, G, eps = population(which)
        d, _ = to_device(nb, ic)
        direct = nb.DirectForceCalculator()
        direct.setGravitationalConstant(G)
        direct.setSofteningParameter(eps)
        direct.computeForces(d)
        ref = acc_of(d).astype(np.float64)
        phi_ref = torch.empty(d.count, dtype=torch.float32, device="cuda")
        pe_ref = direct.computePotential(d, phi_ref)
        phi_ref = phi_ref.cpu().numpy().astype(np.float64)
        for theta in (0.3, 0.5, 0.7, 0.9):
            for order in (1, 2):
                tree = nb.BarnesHutTree(d.count)
                tree.setMultipoleOrder(order)
                tree.build(d)
                tree.computeForces(d, theta, G, eps)
                e = rel_err(acc_of(d), ref)
                phi = torch.empty(d.count, dtype=torch.float32, device="cuda")
                pe = tree.computePotential(d, theta, G, eps, phi)
                ep = (phi.cpu().numpy().astype(np.float64) - phi_ref) / np.abs(phi_ref)
                t_build = timed(lambda: tree.build(d), iters)
                t_walk = timed(lambda: tree.computeForces(d, theta, G, eps), iters)
                t_step = timed(lambda: (tree.build(d), tree.computeForces(d, theta, G, eps)), iters)
                say(f"{which:<10} {theta:>5.1f} {order:>5d} {t_build:>7.3f} {t_walk:>7.3f} {t_step:>7.3f} "
                    f"{np.median(e):>10.3e} {np.percentile(e, 99):>10.3e} {np.sqrt((e * e).mean()):>10.3e} "
                    f"{np.sqrt((ep * ep).mean()):>10.3e} {abs(pe - pe_ref) / abs(pe_ref):>10.3e}")
                tree.close()
        del d


def drift():
    n, G, eps, theta, dt, steps, every = 1 << 17, 1.0, 0.1, 0.5, 1e-3, 2000, 100
    ic = nb.ic.two_galaxies(n, seed=42)
    ic["mass"] = (ic["mass"] / np.float32(n)).astype(np.float32)  # unit total mass
    say(f"# energy drift: two galaxies (unit total mass) N={n}, theta {theta}, eps {eps}, dt {dt}, {steps} steps; "
        f"E = fp64 KE + exact fp64 pair PE every {every} steps")
    for order in (1, 2):
        d, _ = to_device(nb, ic)
        calc = nb.BarnesHutCalculator(theta)
        calc.setGravitationalConstant(G)
        calc.setSofteningParameter(eps)
        calc.setMultipoleOrder(order)
        integ = nb.Integrator()
        calc.computeForces(d)
        ke0, pe0 = integ.computeEnergiesF64(d, G, eps)
        e0 = ke0 + pe0
        worst_e = worst_pe = 0.0
        for s in range(every, steps + 1, every):
            integ.integrate_steps(d, calc, dt, every)
            ke, pe = integ.computeEnergiesF64(d, G, eps)
            worst_e = max(worst_e, abs(ke + pe - e0) / abs(e0))
            worst_pe = max(worst_pe, abs(ke + pe - e0) / abs(pe0))
        say(f"order {order}: E0 {e0:.10e} PE0 {pe0:.10e}; final |E - E0| / |E0| {abs(ke + pe - e0) / abs(e0):.3e}, "
            f"max |E - E0| / |E0| {worst_e:.3e}, max |E - E0| / |PE0| {worst_pe:.3e}")


def step(order):
    ic, G, eps = population("config4")
    d, _ = to_device(nb, ic)
    calc = nb.BarnesHutCalculator(0.5)
    calc.setGravitationalConstant(G)
    calc.setSofteningParameter(eps)
    calc.setMultipoleOrder(order)
    integ = nb.Integrator()
    calc.computeForces(d)
    for _ in range(3):
        integ.integrate(d, calc, 1e-3)
    torch.cuda.synchronize()
    say(f"# one warm config-4 step at order {order} (three steps run; the trace shows all of them)")


def stats(db, label):
    import sqlite3
    con = sqlite3.connect(db)
    rows = con.execute("select name, count(*), sum(duration), max(vgpr_count), max(sgpr_count), max(scratch_size) "
                       "from kernels group by name order by sum(duration) desc").fetchall()
    say(f"# kernel trace {label}: rocprofv3 --kernel-trace --stats, the whole run (ICs, first forces, three steps)")
    say(f"{'calls':>6} {'total_us':>10} {'mean_us':>9} {'vgpr':>5} {'sgpr':>5} {'scratch':>7}  kernel")
    order2 = []
    for name, calls, total, vgpr, sgpr, scratch in rows:
        short = name.split("(")[0]
        if "quad_kernel" in short or "const* restrict>" in short:
            order2.append(short)
        say(f"{calls:>6d} {total / 1e3:>10.1f} {total / 1e3 / calls:>9.1f} {vgpr:>5d} {sgpr:>5d} {scratch:>7d}  {short}")
    say(f"order-2 kernels in this trace: {', '.join(sorted(set(order2))) if order2 else 'none'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="table", choices=("table", "drift", "step", "stats"))
    ap.add_argument("arg", nargs="?", default=None, help="step: the order (2); stats: the trace database")
    ap.add_argument("label", nargs="?", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_bh_quadrupole.txt"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    OUT[0] = None if a.out == "-" else a.out
    if a.what == "stats":
        stats(a.arg, a.label)
        return
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    {"table": lambda: table(a.iters), "drift": drift, "step": lambda: step(int(a.arg or 2))}[a.what]()


if __name__ == "__main__":
    main()
