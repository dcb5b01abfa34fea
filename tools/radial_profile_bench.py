#!/usr/bin/env python3
"""The radial profiles (nbody_hip_groups_radial_profile) on the config-5 initial conditions: the
uniform box at 16 bodies per unit volume, N = 2^22, friends-of-friends catalogues at linking length b = 0.2 and 0.9 of the
mean spacing (the rows of profiles/r26_group_props.txt), about the groups' centres of mass and bulk velocities; and all
bodies as one group at N = 2^16 and 2^22, about the origin.

Per case, by device events, medians of REPS readings after WARM warm-up calls with (min - max):
  findGroups and properties on the same catalogue, in the same run: the yardsticks;
  the radial profile call in its three modes (six cuts), with and without the two outputs of the radial order;
  the byte model of the pass against the measured time.
Then the host path the call replaces, once, on one CPU thread: the read-back of bodies and catalogue, and the numpy
restatement (np.lexsort on (group, bits(q)), a cumulative mass, the cuts, the shell sums by np.add.reduceat).
With --workload the calls alone run (for a kernel trace); --stages CSV sums that trace per kernel of the pass.
usage: python tools/radial_profile_bench.py [--out FILE] [--small] [--no-host] [--workload] [--stages CSV]
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
SPACING = 16.0 ** (-1 / 3)
HBM_TBS = 6.29
FRACTIONS = [0.1, 0.25, 0.5, 0.75, 0.9, 1.0]
RADII = {"groups": [0.05, 0.1, 0.2, 0.5, 1.0, float("inf")], "one": [1.0, 2.0, 4.0, 8.0, 16.0, float("inf")]}
OUT = None  # --out: every line is appended as it is said

# the kernels of one call, in stream order (the two scans and the sort are rocPRIM's: whatever runs between ours)
STAGES = ("check", "scan 1", "key", "sort", "first", "terms", "small", "scan", "base", "cut", "row", "scan 2", "shell small",
          "shell chunk", "shell combine")
OURS = {"radial_check_kernel": "check", "radial_key_kernel": "key", "radial_first_kernel": "first", "radial_terms_kernel": "terms",
        "radial_small_kernel": "small", "radial_scan_kernel": "scan", "radial_base_kernel": "base", "radial_cut_kernel": "cut",
        "radial_row_kernel": "row", "radial_shell_small_kernel": "shell small", "radial_shell_chunk_kernel": "shell chunk",
        "radial_shell_combine_kernel": "shell combine"}
BETWEEN = {"check": "scan 1", "key": "sort", "row": "scan 2"}  # what rocPRIM runs after these kernels of ours


def say(line):
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def spread(t):
    return f"{np.median(t):9.3f} ms (min {min(t):.3f}, max {max(t):.3f})"


def bodies(nb, n):
    from gpu_util import to_device
    h = 0.5 * (n / 16.0) ** (1 / 3)
    ic = nb.ic.uniform_box(n, seed=42, lo=-h, hi=h)
    d, _ = to_device(nb, ic)
    return d, ic


def byte_model(n_members, n_groups, n_cuts, order_out):
    """bytes the pass has to move once: key pass (index 4, position 12, key 8 + position 4 out), the sort's pairs in and
    out per radix pass (rocPRIM: two passes over 12 bytes in and out at up to 44 key bits, a histogram read of 8), the
    head search (8), the terms pass (key 8, position 4, index 4, 28 of the body, 32 of terms out), E (8 in, 8 out), the
    shell sums (32), the structs; the optional order (4 + 4 out)"""
    per_member = (4 + 12 + 12) + (8 + 2 * 24) + 8 + (8 + 4 + 4 + 28 + 32) + 16 + 32 + (8 if order_out else 0)
    return n_members * per_member + n_groups * (32 + 64 * n_cuts + 48 + 28 * n_cuts)


def host_path(d, offsets, members, centres, vels, cuts):
    """the path the call replaces: bodies and catalogue read back, then numpy on one thread (mass mode)"""
    t0 = time.perf_counter()
    f = {k: getattr(d, k).cpu().numpy() for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
    off = offsets.cpu().numpy().astype(np.int64)
    mem = np.arange(d.count) if members is None else members.cpu().numpy()
    t1 = time.perf_counter()
    n = np.diff(off)
    gid = np.repeat(np.arange(n.size), n)
    dx = [f[k][mem].astype(np.float64) - centres[gid, a] for a, k in enumerate(("pos_x", "pos_y", "pos_z"))]
    u = [f[k][mem].astype(np.float64) - vels[gid, a] for a, k in enumerate(("vel_x", "vel_y", "vel_z"))]
    m = f["mass"][mem].astype(np.float64)
    r2 = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]
    q = r2.astype(np.float32)
    order = np.lexsort((q.view(np.uint32), gid))
    r = np.sqrt(r2[order])
    with np.errstate(invalid="ignore", divide="ignore"):
        vr = np.where(r > 0, (u[0] * dx[0] + u[1] * dx[1] + u[2] * dx[2])[order] / r, 0.0)
    ms = m[order]
    u2 = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2])[order]
    cum = np.cumsum(ms)
    base = np.concatenate(([0.0], cum[off[1:-1] - off[0] - 1])) if n.size > 1 else np.zeros(1)
    E = cum - base[gid]
    M = E[off[1:] - off[0] - 1]
    first = off[:-1] - off[0]
    rank = np.arange(ms.size) - first[gid]
    K = np.empty((n.size, len(cuts)), np.int64)
    for c, cut in enumerate(cuts):
        hit = np.where(E >= cut * M[gid], rank + 1, np.iinfo(np.int64).max)
        K[:, c] = np.minimum(np.minimum.reduceat(hit, first), n)
    edges = (first[:, None] + np.concatenate((np.zeros((n.size, 1), np.int64), K), 1)).reshape(-1)
    sums = []
    for t in (ms, ms * vr, ms * vr * vr, ms * (u2 - vr * vr)):
        s = np.add.reduceat(np.concatenate((t, [0.0])), np.minimum(edges, t.size))
        sums.append(s.reshape(n.size, -1)[:, :-1] * (np.diff(edges.reshape(n.size, -1), axis=1) > 0))
    radius = np.sqrt(q[order][first[:, None] + K - 1].astype(np.float64))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, radius, sums


def cases(nb, small):
    """(label, d, offsets, members, centres, vels, kind, grid, b) one after another; the bodies of a size are shared"""
    import torch
    ctx = nb.default_context()
    for n in ((1 << 16,) if small else (1 << 22,)):
        d, ic = bodies(nb, n)
        pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)
        for frac in (0.2, 0.9):
            b = float(np.float32(frac * SPACING))
            cell = nb.ParticleSystem.groupCellSize(pos.min(0), pos.max(0), n, b)
            grid = nb.SpatialHashGrid(n, cell)
            grid.build(d)
            cat = grid.findGroups(b, 1)
            props = cat.properties(d, None, ctx)
            label = (f"N = {n}, b = {frac} x mean spacing, min_members 1 (cell {cell:.6f}): {cat.n_groups} groups, "
                     f"{cat.n_members} members, largest {int(cat.sizes().max())}")
            yield label, d, cat, torch.from_numpy(props["com"].copy()).cuda(), torch.from_numpy(props["vel"].copy()).cuda(), "groups", grid, b
            grid.close()
        del d
    for n in ((1 << 14,) if small else (1 << 16, 1 << 22)):
        d, _ = bodies(nb, n)
        cat = nb.GroupCatalogue(torch.zeros(n, dtype=torch.int32, device="cuda"),
                                torch.tensor([0, n], dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 0.0, 1)
        cat.members, cat.n_members = None, n
        yield (f"N = {n}, all bodies as one group (members = NULL)", d, cat, torch.zeros((1, 3), dtype=torch.float64, device="cuda"),
               torch.zeros((1, 3), dtype=torch.float64, device="cuda"), "one", None, None)
        del d


def run(small, host_too, workload):
    import torch

    import nbody_amd as nb
    if not torch.cuda.is_available():
        raise SystemExit("radial_profile_bench.py measures on a GPU: none is visible")
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

    for label, d, cat, cen, vel, kind, grid, b in cases(nb, small):
        nc = len(FRACTIONS)
        groups, shells = nb.radial_tensors(cat.n_groups, nc, "cuda")
        sm = torch.empty(cat.n_members, dtype=torch.int32, device="cuda")
        sq = torch.empty(cat.n_members, dtype=torch.float32, device="cuda")

        def profile(cuts, mode, order_out):
            nb.groups_radial_profile_into(ctx, d, cat.offsets, cat.members, cen, cuts, groups, shells, mode, vel,
                                          sm if order_out else None, sq if order_out else None)

        mass = lambda: profile(FRACTIONS, "mass", False)  # noqa: E731
        if workload:
            for _ in range(WARM + REPS):
                mass()
            torch.cuda.synchronize()
            continue
        say(label)
        if grid is not None:
            out = nb.group_props_tensor(cat.n_groups, "cuda")
            say(f"    findGroups, whole call                     {spread(events(lambda: grid.findGroups(b, 1)))}")
            say(f"    properties, no phi                         {spread(events(lambda: cat.properties_into(d, out, None, ctx)))}")
        t_mass = events(mass)
        say(f"    radial profile, mass fractions             {spread(t_mass)}")
        say(f"    radial profile, number fractions           {spread(events(lambda: profile(FRACTIONS, 'number', False)))}")
        say(f"    radial profile, radii                      {spread(events(lambda: profile(RADII[kind], 'radius', False)))}")
        t_order = events(lambda: profile(FRACTIONS, "mass", True))
        say(f"    radial profile, mass, with the radial order{spread(t_order)}")
        for name, t, order_out in (("mass", t_mass, False), ("mass + order", t_order, True)):
            model = byte_model(cat.n_members, cat.n_groups, nc, order_out)
            floor = model / (HBM_TBS * 1e12) * 1e3
            say(f"    byte model, {name:13s} {model / 1e6:9.1f} MB = {floor:.3f} ms at {HBM_TBS} TB/s: "
                f"{100 * floor / np.median(t):.0f} % of the measured time")
        g, s = nb.radial_arrays(groups, shells, nc)
        say(f"    status 0 in {int((g['status'] == 0).sum())} of {len(g)} groups; workspace {ctx_workspace(cat, nc) / 1e6:.1f} MB")
        if host_too:
            t_copy, t_numpy, radius, sums = host_path(d, cat.offsets, cat.members, cen.cpu().numpy(), vel.cpu().numpy(), FRACTIONS)
            mass()
            g, s = nb.radial_arrays(groups, shells, nc)
            agree = float(np.mean(np.abs(radius - s["radius"]) <= 1e-6 * s["radius"]))
            say(f"    host path, one CPU thread: read-back {t_copy * 1e3:.1f} ms, numpy (lexsort, cumulative mass, cuts, shell sums) "
                f"{t_numpy * 1e3:.1f} ms; its radii agree with the device's in {100 * agree:.2f} % of the rows")
        del groups, shells, sm, sq


def ctx_workspace(cat, nc):
    """bytes of the workspace by the header's count (64 per member, 16 per group, 12 per row, 48 per possible chunk; the
    sort's and the scan's temporary storage come on top)"""
    return 64 * cat.n_members + 16 * cat.n_groups + 12 * cat.n_groups * nc + 48 * (cat.n_members // 1024 + cat.n_members // 33)


def stages(path):
    """kernel time per radial profile call (mass fractions) by kernel, from a kernel trace of --workload"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur, between = [], None, None
    for r in rows:
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        ours = next((s for k, s in OURS.items() if k in name), None)
        if ours == "check":
            cur = dict.fromkeys(STAGES, 0.0)
            cur["start"] = t0
            calls.append(cur)
        if cur is None:
            continue
        if ours:
            cur[ours] += (t1 - t0) / 1e6
            between = BETWEEN.get(ours)
            cur["end"] = t1
        elif between:
            cur[between] += (t1 - t0) / 1e6
            cur["end"] = t1
    per = WARM + REPS
    if not calls or len(calls) % per:
        raise SystemExit(f"{len(calls)} calls in the trace: not a multiple of {per}")
    say(f"kernel time per radial profile call (mass fractions) by kernel, from a kernel trace of the same calls (median of {REPS} "
        f"after {WARM}), ms; the cases in the order above:")
    for k in range(len(calls) // per):
        sel = calls[k * per + WARM:(k + 1) * per]
        med = {s: float(np.median([c[s] for c in sel])) for s in STAGES}
        text = ", ".join(f"{s} {v:.3f}" for s, v in med.items() if v > 0)
        span = np.median([(c["end"] - c["start"]) / 1e6 for c in sel])
        say(f"    case {k + 1}: {text}; sum {sum(med.values()):.3f}, span on the stream {span:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 2^16 and 2^14 only (a rehearsal)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--stages")
    a = ap.parse_args()
    global OUT
    OUT = a.out
    if a.stages:
        stages(a.stages)
    else:
        run(a.small, not a.no_host, a.workload)


if __name__ == "__main__":
    main()
