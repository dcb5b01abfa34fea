"""The block-step Hermite ENSEMBLE (BlockHermiteEnsemble) against a host loop over single-system
integrators: B independent systems of n bodies each, one macro step.

  systems    n >= 16: Plummer spheres (seed 42 + s), G = 1, eps = 0.01, eta = 0.02, eta_start = 0.01, max_level = 16,
             dt_max = 1/16; n = 3: the binary-with-a-perturber systems of tests/hermite_batch_cases.py (G = 1.7,
             eps = 1e-4, max_level = 10, dt_max = 1/16), drawn from one seeded generator
  (c)        this tree's ensemble: ONE advance(1) call for all B systems plus the stream synchronisation after it
  (a)        the host form of the tree given with --parent-tree (the parent commit; default this tree): one
             BlockHermiteIntegrator per system, advance(1) on each in a loop, then the synchronisation
  (b)        the same loop in "resident" scheduling
             For B > SUBSET the loops (a) and (b) run on the first SUBSET systems and their time is scaled by B / SUBSET
             (a loop's time is the sum of its systems' times); the rows say so.
  reading    wall-clock ms of the calls plus the synchronisation; every shape is warmed up by one macro step; per n,
             ROUNDS rounds of the child processes (a), (c), (b) in turn -- the parent tree and this tree alternately --
             each child under its own time limit, READINGS readings per shape and round; the median (min, max) of the
             ROUNDS x READINGS readings
  columns    ms per macro step of (c); aggregate body steps per second of (c) (the corrected bodies of all systems in that
             macro step over its time); (a) / (c) and (b) / (c); the spread of (a)'s own readings, max / min

Combinations above 2^20 bodies are skipped.  The first non-zero status of a child ends the run.
usage: python tools/hermite_batch_time.py [--parent-tree DIR] [--out profiles/r13_hermite_batch.txt] [--sizes 3,16]
                                          [--systems 1,64]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (3, 16, 64, 256, 1024)
SYSTEMS = (1, 64, 256, 1024, 4096)
MAX_BODIES = 1 << 20
SUBSET = 64
ROUNDS, READINGS = 2, 5
PLUMMER = dict(G=1.0, eps=0.01, dt_max=1.0 / 16, max_level=16)
ETA, ETA_START = 0.02, 0.01


def shapes(n, systems):
    return [b for b in systems if b * n <= MAX_BODIES]


def child(n, form, tree, systems):
    """one form, one n, every B: RESULT {B: {"ms": [...], "body_steps": [...], "timed_systems": S}}"""
    import numpy as np
    import torch
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    import hermite_batch_cases as bc
    from gpu_util import to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    c = bc.TRIPLE if n == 3 else PLUMMER
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(c["G"])
    fc.setSofteningParameter(c["eps"])
    out = {}
    for B in shapes(n, systems):
        count = B if form == "batch" else min(B, SUBSET)
        ics = bc.triples(count) if n == 3 else [nb.ic.plummer(n, seed=42 + s) for s in range(count)]
        ms, bodies = [], []
        if form == "batch":
            ic, off = nb.ic.concat(ics)
            d, _ = to_device(nb, ic)
            ens = nb.BlockHermiteEnsemble()
            ens.setParameters(ETA, ETA_START, c["max_level"])
            ens.setLayout(off)
            ens.prime(d, fc, c["dt_max"])
            ens.advance(d, 1)  # warm-up: the levels settle
            for _ in range(READINGS):
                before = ens.info()["body_steps"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ens.advance(d, 1)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                bodies.append(ens.info()["body_steps"] - before)
            ens.close()
        else:
            runs = []
            for ic in ics:
                d, _ = to_device(nb, ic)
                blk = nb.BlockHermiteIntegrator()
                blk.setParameters(ETA, ETA_START, c["max_level"])
                blk.setScheduling(form)
                blk.advance(d, fc, c["dt_max"], 1)  # warm-up: priming, the workspaces, the levels settle
                runs.append((d, blk))
            for _ in range(READINGS):
                before = sum(blk.info()["body_steps"] for _, blk in runs)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for d, blk in runs:
                    blk.advance(d, fc, c["dt_max"], 1)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 * B / count)
                bodies.append((sum(blk.info()["body_steps"] for _, blk in runs) - before) * B // count)
            for _, blk in runs:
                blk.close()
        out[B] = {"ms": ms, "body_steps": bodies, "timed_systems": count}
    print("RESULT " + json.dumps({"shapes": out, "device": torch.cuda.get_device_name(0),
                                  "lib": os.path.relpath(nb._lib.LIB_PATH, tree)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_hermite_batch.txt"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--systems", default=",".join(str(b) for b in SYSTEMS))
    ap.add_argument("--parent-tree", default=None, help="a built tree whose integrators are the loops (a) and (b)")
    ap.add_argument("--case", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--form", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    systems = [int(v) for v in a.systems.split(",")]
    if a.case:
        return child(a.case, a.form, a.tree, systems)
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    forms = (("a", "host", parent), ("c", "batch", ROOT), ("b", "resident", parent))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as fh:  # (kept current: a run that is cut short leaves its rows behind)
            fh.write("\n".join(lines) + "\n")

    def run(n, form, tree):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", str(n), "--form", form,
               "--tree", tree, "--systems", a.systems]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"n = {n}, {form}: status {r.returncode}; stopping")
            sys.exit(r.returncode)
        return json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))

    for n in (int(v) for v in a.sizes.split(",")):
        got = {k: [] for k, _, _ in forms}
        for _ in range(ROUNDS):
            for key, form, tree in forms:
                got[key].append(run(n, form, tree))
        if not lines:
            say(f"tools/hermite_batch_time.py on {got['c'][0]['device']}: ms per macro step, one advance(1) per system (a, b) or "
                f"per ensemble (c) + synchronisation, median (min, max) of {ROUNDS} x {READINGS} readings, child processes "
                f"(a), (c), (b) in turn; loops over more than {SUBSET} systems timed on the first {SUBSET} and scaled")
            say(f"  (a) host form, (b) resident form, one integrator per system in a loop: {got['a'][0]['lib']} of "
                f"{'the tree given with --parent-tree' if a.parent_tree else 'this tree'}")
            say(f"  (c) the ensemble, one launch: {got['c'][0]['lib']} of this tree")
            say("  n >= 16: Plummer spheres, G = 1, eps = 0.01, eta = 0.02, max_level = 16, dt_max = 1/16; n = 3: binary "
                "(e = 0.9) with a perturber, G = 1.7, eps = 1e-4, max_level = 10, dt_max = 1/16")
        for B in shapes(n, systems):
            row = {}
            for key in ("a", "b", "c"):
                ms = [v for r in got[key] for v in r["shapes"][str(B)]["ms"]]
                row[key] = (statistics.median(ms), min(ms), max(ms))
            bd = statistics.median([v for r in got["c"] for v in r["shapes"][str(B)]["body_steps"]])
            timed = got["a"][0]["shapes"][str(B)]["timed_systems"]
            spread = row["a"][2] / row["a"][1]
            say(f"n = {n:5d}  B = {B:5d}  (c) {row['c'][0]:10.3f} ({row['c'][1]:.3f}, {row['c'][2]:.3f}) ms  "
                f"{bd / row['c'][0] * 1e3:12.4e} body steps/s  (a) {row['a'][0]:10.3f} ({row['a'][1]:.3f}, {row['a'][2]:.3f})  "
                f"(b) {row['b'][0]:10.3f} ({row['b'][1]:.3f}, {row['b'][2]:.3f})  (a)/(c) = {row['a'][0] / row['c'][0]:8.2f}  "
                f"(b)/(c) = {row['b'][0] / row['c'][0]:8.2f}  spread of (a), max/min = {spread:.2f}  "
                f"{bd:.0f} body steps per macro step"
                + (f"  [(a), (b) timed on {timed} systems, x {B // timed}]" if timed < B else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
