#!/usr/bin/env python3
"""The density-peak (HOP) groups (nbody_hip_hop_groups) measured beside the neighbour search that
feeds them, in one run:
  config-5 initial conditions (the uniform box at 16 bodies per unit volume), N = 4,194,304, grid cell 1.0;
  config 4 (two galaxies), N = 1,048,576, grid cell 0.25;
  config 5 at N = 1,048,576, where the numpy restatement of tests/hop_ref.py runs on one CPU thread beside the device.
Parameters: k = 16, n_hop = 16, n_merge = 4, delta_outer = the lower median of the densities, HOP's defaults above it.
Per workload, medians and ranges of 2 x 5 readings (two rounds of five, each after a warm-up call): neighbours(k = 16) and
the whole hop_groups call by device events around them, the six stages of the call by the events the library records
(nbody_hip_hop_stage_times), and n_peaks, n_groups, rounds and the number of directed boundary records.
usage: python tools/hop_profile.py [--out FILE] [--small]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS, REPS = 2, 5
K, N_HOP, N_MERGE = 16, 16, 4
OUT = None  # --out: every line is appended as it is said


def say(line):
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def spread(t):
    return f"{np.median(t):9.3f} ms (min {min(t):.3f}, max {max(t):.3f})"


def timed(torch, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z), out


def record_count(torch, cat, res, delta_outer):
    """directed boundary records of the call, counted as the model states them (plain torch: a tool's plumbing)"""
    live = res.rho >= delta_outer
    peak = cat.peak.to(torch.int64)
    pairs = 0
    for s in range(N_MERGE):
        j = res.index[:, s].to(torch.int64)
        jj = j.clamp(min=0)
        pairs += int((live & (j >= 0) & live[jj] & (peak != peak[jj])).sum())
    return 2 * pairs


def workload(nb, torch, ctx, name, ic, cell, host_too):
    import hop_ref as ref
    from gpu_util import to_device
    d, _ = to_device(nb, ic)
    n = d.count
    grid = nb.SpatialHashGrid(n, cell, ctx)
    grid.build(d)
    t_nb, t_hop, stages = [], [], {s: [] for s in nb.HOP_STAGES}
    cat = res = None
    for _ in range(ROUNDS):
        res = grid.neighbours(K, lists=True, density=True)  # warm-up
        delta_outer = float(torch.nanmedian(res.rho))
        nb.hop_groups(ctx, res.index, res.rho, N_HOP, N_MERGE, delta_outer)
        for _ in range(REPS):
            ms, res = timed(torch, lambda: grid.neighbours(K, lists=True, density=True))
            t_nb.append(ms)
            ms, cat = timed(torch, lambda: nb.hop_groups(ctx, res.index, res.rho, N_HOP, N_MERGE, delta_outer))
            t_hop.append(ms)
            for s, v in cat.stage_ms.items():
                stages[s].append(v)
    dims = grid.getGridDims()
    exact = float((res.status == 0).float().mean())
    say(f"{name}: N = {n}, cell {cell} (grid {dims[0]}x{dims[1]}x{dims[2]}), k = {K}, n_hop = {N_HOP}, n_merge = {N_MERGE}, "
        f"delta_outer = median density = {delta_outer:.6g}; {100 * exact:.1f} % of the lists exact")
    say(f"    n_peaks {cat.n_peaks}, n_groups {cat.n_groups}, n_members {cat.n_members}, rounds {cat.rounds}, "
        f"directed boundary records {record_count(torch, cat, res, delta_outer)}")
    say(f"    neighbours(k = {K})              {spread(t_nb)}")
    say(f"    hop_groups, whole call          {spread(t_hop)}")
    for s in nb.HOP_STAGES:
        say(f"        {s:<28}{spread(stages[s])}")
    say(f"        (the stages sum to {sum(np.median(v) for v in stages.values()):.3f} ms; records and unite-and-attach "
        f"include their read-backs)")
    if host_too:
        t0 = time.perf_counter()
        index, rho = res.index.cpu().numpy(), res.rho.cpu().numpy()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = ref.reference(index, rho, N_HOP, N_MERGE, delta_outer)
        t_numpy = time.perf_counter() - t0
        same = all(np.array_equal(want[key], getattr(cat, key).cpu().numpy()) for key in ("labels", "peak", "offsets", "members",
                                                                                           "group_peak"))
        say(f"    host path, one CPU thread: read-back of lists and densities {t_copy * 1e3:.1f} ms, the numpy restatement "
            f"{t_numpy * 1e3:.1f} ms; its five arrays equal the device's: {same}")
    grid.close()
    del d, res, cat
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 2^16 everywhere (a rehearsal)")
    a = ap.parse_args()
    global OUT
    OUT = a.out
    import torch
    import nbody_amd as nb
    torch.set_num_threads(1)
    ctx = nb.default_context(0)
    say(f"hop_groups beside neighbours(k = {K}), {ROUNDS} x {REPS} readings each, device events; {torch.cuda.get_device_name(0)}")
    n5, n4, n5s = (1 << 16,) * 3 if a.small else (1 << 22, 1 << 20, 1 << 20)
    half = lambda n: 0.5 * (n / 16.0) ** (1 / 3)
    workload(nb, torch, ctx, "config 5, uniform box", nb.ic.uniform_box(n5, seed=42, lo=-half(n5), hi=half(n5)), 1.0, False)
    workload(nb, torch, ctx, "config 4, two galaxies", nb.ic.two_galaxies(n4, seed=42), 0.25, False)
    workload(nb, torch, ctx, "config 5, uniform box", nb.ic.uniform_box(n5s, seed=42, lo=-half(n5s), hi=half(n5s)), 1.0, True)


if __name__ == "__main__":
    main()
