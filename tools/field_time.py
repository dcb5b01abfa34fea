"""Field calls (nbody_hip_{direct,tree,grid}_field), ms per call: median of 5 after a warm-up call, host clock around
work that ends in a device synchronise; the tree / grid is built once per case.

  config 4 tree   two galaxies, 2^20 bodies, theta 0.5, eps 0.1, multipole orders 1 and 2: 2^18 and 2^20 points, a random
                  cloud in the bodies' box and a raster in the orbital plane (row-major caller order), with the points
                  Morton-sorted by the call (default) and in caller order (NBH_FIELD_SORT=0); the Direct field at the same
                  point counts (the O(N M) comparison); small point counts (no replicas: what a small M costs)
  config 5 grid   uniform box at 16 bodies per unit volume, 2^22 bodies, cell = cutoff = 1, eps 0.01: 2^22 random points,
                  sorted by cell and in caller order
  own positions   the field walk over the bodies' own positions against the force walk plus the potential walk on the
                  same tree -- one pass against two
usage: python tools/field_time.py [--out profiles/r06_field.txt] [--small]
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

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(min(t)), float(max(t))


def fmt(t):
    return f"{t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def sorted_and_not(fn):
    """(sorted by the call, caller order) timings of fn"""
    os.environ.pop("NBH_FIELD_SORT", None)
    a = ms(fn)
    os.environ["NBH_FIELD_SORT"] = "0"
    try:
        b = ms(fn)
    finally:
        os.environ.pop("NBH_FIELD_SORT", None)
    return a, b


def clouds(pos, m):
    lo, hi = pos.min(0), pos.max(0)
    side = int(round(np.sqrt(m)))
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[1], hi[1], side), indexing="ij")
    raster = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1).astype(np.float32)
    cloud = np.random.default_rng(1).uniform(lo, hi, (m, 3)).astype(np.float32)
    return {"random cloud": cloud, "raster": raster}


def tree_config4(small):
    n, G, eps, theta = 1 << 20, 1.0, 0.1, 0.5
    ic = nb.ic.two_galaxies(n, seed=42)
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)
    d, _ = to_device(nb, ic)
    direct = nb.DirectForceCalculator()
    direct.setGravitationalConstant(G)
    direct.setSofteningParameter(eps)
    sizes = (1 << 18,) if small else (1 << 18, 1 << 20)
    for order in (1, 2):
        t = nb.BarnesHutTree(n)
        t.setMultipoleOrder(order)
        t.build(d)
        for m in sizes:
            for name, pts in clouds(pos, m).items():
                p = torch.from_numpy(pts).cuda()
                out = torch.empty((len(pts), 4), dtype=torch.float32, device="cuda")
                a, b = sorted_and_not(lambda: t.computeField(p, theta, G, eps, out))
                say(f"config 4 tree field, order {order}, {len(pts)} points, {name}: sorted {fmt(a)}, caller order {fmt(b)}")
                if order == 1:
                    say(f"  Direct field, {n} bodies x {len(pts)} points, {name}: {fmt(ms(lambda: direct.computeField(d, p, out), reps=3))}")
        # the bodies' own positions: one pass against the force walk + the potential walk
        p = torch.from_numpy(pos.astype(np.float32)).cuda()
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        phi = torch.empty(n, dtype=torch.float32, device="cuda")
        a, b = sorted_and_not(lambda: t.computeField(p, theta, G, eps, out))
        f = ms(lambda: t.computeForces(d, theta, G, eps))
        ph = ms(lambda: t.computePotential(d, theta, G, eps, phi))
        line = (f"own positions, order {order}, {n} bodies: field walk sorted {fmt(a)}, caller order {fmt(b)}; force walk "
                f"(automatic form) {fmt(f)}, potential walk (phi + PE) {fmt(ph)}")
        if order == 1:
            t.walkForm(1)
            line += f", force walk (plain form) {fmt(ms(lambda: t.computeForces(d, theta, G, eps)))}"
            t.walkForm(0)
        say(line)
        if order == 1:  # small point counts: no replicas, a handful of waves on 256 CUs
            for m in (64, 1024, 16384, 65536):
                p = torch.from_numpy(clouds(pos, m)["random cloud"]).cuda()
                out = torch.empty((m, 4), dtype=torch.float32, device="cuda")
                say(f"config 4 tree field, order 1, {m} points, random cloud: {fmt(ms(lambda: t.computeField(p, theta, G, eps, out)))}; "
                    f"Direct field: {fmt(ms(lambda: direct.computeField(d, p, out), reps=3))}")


def grid_config5(small):
    n = 1 << (20 if small else 22)
    half = 0.5 * (n / 16.0) ** (1.0 / 3.0)
    ic, G, eps, cutoff = nb.ic.uniform_box(n, seed=42, lo=-half, hi=half), 1.0, 0.01, 1.0
    d, _ = to_device(nb, ic)
    g = nb.SpatialHashGrid(n, 1.0)
    g.build(d)
    p = torch.from_numpy(np.random.default_rng(2).uniform(-half, half, (n, 3)).astype(np.float32)).cuda()
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    phi = torch.empty(n, dtype=torch.float32, device="cuda")
    a, b = sorted_and_not(lambda: g.computeField(p, cutoff, G, eps, out))
    f = ms(lambda: g.computeForces(d, cutoff, G, eps))
    ph = ms(lambda: g.computePotential(d, cutoff, G, eps, phi))
    say(f"config 5 grid field, {n} bodies, {n} random points: sorted {fmt(a)}, caller order {fmt(b)}; force call {fmt(f)}, "
        f"potential call (phi + PE) {fmt(ph)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_field.txt"))
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    say(f"tools/field_time.py on {torch.cuda.get_device_name(0)}: ms per call, median of 5 (min, max) after a warm-up call")
    tree_config4(a.small)
    grid_config5(a.small)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
