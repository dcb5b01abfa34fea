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
  --properties  the group properties (nbody_hip_groups_properties) on the same cases, grid by the
              density rule, min_members 1 and 32: the findGroups call that made the catalogue, GroupCatalogue.properties
              without and with phi (asynchronous form, device events), the older route for the groups of at most 4,096
              members (GroupCatalogue.systems + systems_diagnostics), and the byte model of the pass against the HBM rate
  --properties-workload  only the properties calls with phi (WARM + REPS per case): the program for a kernel trace
  --properties-stages F  folds such a trace into kernel time per call and kernel (cases in the order of --properties)
usage: python tools/groups_bench.py [--out FILE] [--small] [--no-scipy] | --workload [--small] | --stages CSV [--out FILE]
       | --properties [--small] [--out FILE] | --properties-workload [--small]
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


HBM_TBS = 6.29  # measured copy rate of an MI355X, TB/s: what the byte model is set against


def run_properties(small, workload):
    import torch

    import nbody_amd as nb
    if not torch.cuda.is_available():
        raise SystemExit("groups_bench.py measures on a GPU: none is visible")
    ctx = nb.default_context()

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

    for n in ((1 << 16,) if small else (1 << 20, 1 << 22)):
        d, pos = bodies(nb, n)
        for frac in (0.2, 0.9):
            b = float(np.float32(frac * SPACING))
            grid, cell = grid_for(nb, d, pos, b, "cell by rule")
            phi = torch.empty(n, dtype=torch.float32, device="cuda")
            grid.computePotential(d, b, G, EPS, phi)
            for min_members in (1, 32):
                cat = grid.findGroups(b, min_members)
                if cat.n_groups == 0:
                    say(f"N = {n}, b = {frac}, min_members {min_members}: no group")
                    continue
                sizes = cat.sizes()
                out = nb.group_props_tensor(cat.n_groups, "cuda")
                with_phi = lambda: cat.properties_into(d, out, phi, ctx)  # noqa: E731
                if workload:
                    for _ in range(WARM + REPS):
                        with_phi()
                    torch.cuda.synchronize()
                    continue
                say(f"N = {n}, b = {frac} x mean spacing, min_members {min_members} (cell {cell:.6f}): {cat.n_groups} groups, "
                    f"{cat.n_members} members, largest {int(sizes.max())}")
                say(f"    findGroups, whole call                     {spread(events(lambda: grid.findGroups(b, min_members)))}")
                t_bare = events(lambda: cat.properties_into(d, out, None, ctx))
                t_phi = events(with_phi)
                say(f"    properties, no phi                         {spread(t_bare)}")
                say(f"    properties, with phi                       {spread(t_phi)}")
                for name, t, per in (("no phi", t_bare, 24), ("with phi", t_phi, 28)):
                    model = cat.n_members * ((4 + 28) + (4 + per)) + 192 * cat.n_groups
                    floor = model / (HBM_TBS * 1e12) * 1e3
                    say(f"    byte model, {name:9s} {model / 1e6:9.1f} MB = {floor:.3f} ms at {HBM_TBS} TB/s: "
                        f"{100 * floor / np.median(t):.0f} % of the measured time")
                keep = sizes <= 4096
                if int(keep.sum()) > 0:
                    kept = nb.GroupCatalogue(cat.labels, torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"),
                                                                    torch.cumsum(sizes[keep], 0).to(torch.int32)]),
                                             cat.members[torch.repeat_interleave(keep, sizes.to(torch.int64))].contiguous(),
                                             b, min_members)
                    diag = nb.system_diag_tensor(kept.n_groups, "cuda")

                    def older():
                        sub, off = kept.systems(d)
                        nb.systems_diagnostics_into(ctx, sub, off, G, EPS, diag)

                    kout = nb.group_props_tensor(kept.n_groups, "cuda")
                    say(f"    groups of at most 4,096 members only: {kept.n_groups} groups, {kept.n_members} members")
                    say(f"      systems() + systems_diagnostics          {spread(events(older))}")
                    say(f"      properties, no phi                       {spread(events(lambda: kept.properties_into(d, kout, None, ctx)))}")
            grid.close()


def properties_stages(path, small):
    """kernel time per properties call by kernel, from a kernel trace of --properties-workload"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = ("count", "scan", "small", "chunk<1>", "combine<1>", "chunk<2>", "combine<2>")
    calls, cur = [], None
    for r in rows:
        name, t = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "group_props_count_kernel" in name:
            cur = dict.fromkeys(names, 0.0)
            cur["start"], cur["open"] = int(r["Start_Timestamp"]), True
            calls.append(cur)
            cur["count"] += t
        elif cur is None:
            continue
        elif "group_props_small_kernel" in name:
            cur["small"] += t
            cur["open"] = False  # (the scan lies between the count and the small-form kernel: later scans are not ours)
        elif "group_props_" in name:
            kind = "chunk" if "chunk_kernel" in name else "combine"
            cur[f"{kind}<{1 if 'ILi1E' in name or '<1>' in name else 2}>"] += t
        elif cur["open"]:
            cur["scan"] += t
        cur["end"] = int(r["End_Timestamp"]) if "group_props_" in name or cur["open"] else cur.get("end", 0)
    per = WARM + REPS
    if len(calls) % per:
        raise SystemExit(f"{len(calls)} calls in the trace: not a multiple of {per}")
    say(f"kernel time per properties call (with phi) by kernel, from a kernel trace of the same calls (median of {REPS} after {WARM}), ms:")
    for k in range(len(calls) // per):
        sel = calls[k * per + WARM:(k + 1) * per]
        text = ", ".join(f"{s} {np.median([c[s] for c in sel]):.3f}" for s in names)
        span = np.median([(c["end"] - c["start"]) / 1e6 for c in sel])
        say(f"    case {k + 1}: {text}; sum {sum(np.median([c[s] for c in sel]) for s in names):.3f}, span on the stream {span:.3f}")


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
    ap.add_argument("--properties", action="store_true")
    ap.add_argument("--properties-workload", action="store_true")
    ap.add_argument("--properties-stages")
    a = ap.parse_args()
    global OUT
    OUT = a.out
    if a.properties_stages:
        properties_stages(a.properties_stages, a.small)
    elif a.properties or a.properties_workload:
        run_properties(a.small, a.properties_workload)
    elif a.stages:
        stages(a.stages, a.small)
    else:
        run(a.small, not a.no_scipy, a.workload)


if __name__ == "__main__":
    main()
