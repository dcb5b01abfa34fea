#!/usr/bin/env python3
"""Friends-of-friends groups (nbody_hip_grid_groups) on the config-5 initial conditions: the uniform box at 16 bodies per
unit volume, N = 2^20 and 2^22, linking length b = 0.2 and 0.9 of the mean spacing, on two grids each -- the cell the
workload's own force grid has (1.0) and the cell of ParticleSystem.findGroups (b * 2^k by the density rule).

  default     per case: the whole SpatialHashGrid.findGroups call (device events around it; it blocks for its two counts),
              computeForces with cutoff = b on the same grid (the same pair set: the yardstick), and the CPU time of the
              scipy restatement (tests/groups_ref.py) with a comparison of its labels.  Medians of REPS readings after WARM
              warm-up calls, with min and max.
  --workload  only the calls (WARM + REPS per case, in the same order): the program for a kernel trace,
              rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/groups_bench.py --workload
  --stages F  folds such a trace (run_kernel_trace.csv) into kernel time per call and stage: link (group_init_kernel,
              group_link_kernel), label (group_label_kernel), catalogue (keys, sort, head flags, scan, offsets), and the
              span of the call on the stream
usage: python tools/groups_bench.py [--out FILE] [--small] [--no-scipy] | --workload [--small] | --stages CSV [--out FILE]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, REPS = 3, 10
G, EPS = 1.0, 0.01
SPACING = 16.0 ** (-1.0 / 3.0)
OUT = None  # --out: every line is appended as it is said


def say(line):
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def cases(small):
    """(N, fraction of the mean spacing, grid name) in the order every mode walks them"""
    return [(n, frac, grid) for n in ((1 << 16,) if small else (1 << 20, 1 << 22)) for frac in (0.2, 0.9)
            for grid in ("cell 1.0", "cell by rule")]


def spread(t):
    return f"{np.median(t):9.3f} ms (min {min(t):.3f}, max {max(t):.3f})"


def bodies(nb, n):
    from gpu_util import to_device
    h = 0.5 * (n / 16.0) ** (1 / 3)
    ic = nb.ic.uniform_box(n, seed=42, lo=-h, hi=h)
    d, _ = to_device(nb, ic)
    return d, np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)


def grid_for(nb, d, pos, b, name):
    cell = 1.0 if name == "cell 1.0" else nb.ParticleSystem.groupCellSize(pos.min(0), pos.max(0), d.count, b)
    grid = nb.SpatialHashGrid(d.count, cell)
    grid.build(d)
    return grid, cell


def run(small, scipy_too, workload):
    import torch

    import nbody_amd as nb
    if not torch.cuda.is_available():
        raise SystemExit("groups_bench.py measures on a GPU: none is visible")

    def events(fn):
        t = []
        for k in range(WARM + REPS):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            if k >= WARM:
                t.append(a.elapsed_time(z))
        return t

    held = {}
    for n, frac, name in cases(small):
        if n not in held:
            held.clear()
            held[n] = bodies(nb, n)
        d, pos = held[n]
        b = float(np.float32(frac * SPACING))
        grid, cell = grid_for(nb, d, pos, b, name)
        if workload:
            for _ in range(WARM + REPS):
                grid.findGroups(b, 1)
            grid.close()
            continue
        dims = grid.getGridDims()
        cat = grid.findGroups(b, 1)
        sizes = cat.sizes()
        say(f"N = {n}, b = {frac} x mean spacing = {b:.6f}, {name} (cell {cell:.6f}, grid {dims[0]}x{dims[1]}x{dims[2]}, start array "
            f"{'yes' if grid.copyCellStartArray() is not None else 'no'}): {cat.n_groups} groups, largest {int(sizes.max())}")
        say(f"    findGroups, whole call       {spread(events(lambda: grid.findGroups(b, 1)))}")
        say(f"    computeForces, cutoff = b    {spread(events(lambda: grid.computeForces(d, b, G, EPS)))}")
        if scipy_too and name == "cell by rule":
            import groups_ref
            t0 = time.perf_counter()
            ref = groups_ref.fof_labels(pos, b)
            t1 = time.perf_counter()
            differ = int((ref != cat.labels.cpu().numpy()).sum())
            say(f"    scipy restatement (kd-tree + connected components, one CPU thread)  {t1 - t0:9.3f} s; labels differ for {differ} bodies")
        grid.close()


def stages(path, small):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    calls, cur = [], None
    for name, t0, t1 in rows:
        if "group_init_kernel" in name:
            cur = {"link": 0, "label": 0, "catalogue": 0, "start": t0, "end": t1, "kernels": 0}
        if cur is None:
            continue
        stage = "link" if ("group_init_kernel" in name or "group_link_kernel" in name) else \
            "label" if "group_label_kernel" in name else "catalogue"
        cur[stage] += t1 - t0
        cur["end"] = t1
        cur["kernels"] += 1
        if "group_offsets_kernel" in name:
            calls.append(cur)
            cur = None
    per = WARM + REPS
    todo = cases(small)
    if len(calls) != per * len(todo):
        raise SystemExit(f"{len(calls)} calls in the trace, expected {per} for each of {len(todo)} cases")
    say(f"kernel time per call by stage, from the kernel trace of the same calls (median of {REPS} after {WARM}, min - max), ms:")
    for k, (n, frac, name) in enumerate(todo):
        sel = calls[k * per + WARM:(k + 1) * per]
        col = {s: np.array([c[s] for c in sel]) / 1e6 for s in ("link", "label", "catalogue")}
        span = np.array([c["end"] - c["start"] for c in sel]) / 1e6
        text = ", ".join(f"{s} {np.median(v):.3f} ({v.min():.3f} - {v.max():.3f})" for s, v in col.items())
        say(f"    N = {n}, b = {frac}, {name}: {text}; {sel[0]['kernels']} kernels, span on the stream {np.median(span):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 2^16 only (a rehearsal)")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--stages")
    a = ap.parse_args()
    global OUT
    OUT = a.out
    if a.stages:
        stages(a.stages, a.small)
    else:
        run(a.small, not a.no_scipy, a.workload)


if __name__ == "__main__":
    main()
