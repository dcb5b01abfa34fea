"""What the ensemble EVENTS (BlockHermiteEnsemble.setEvents) cost and what they are for.

  table 1    B = 1,024 systems of n bodies, the median advance(1) plus the stream synchronisation after it:
               (p) the plain kernel of the tree given with --parent-tree (the parent commit; default this tree)
               (c) the plain kernel of this tree: the same kernel, so (c) / (p) has to lie inside (p)'s own spread
               (t) this tree with the closest approach tracked and radii of 1e-4 on every body, nothing stopping
             systems as tools/hermite_batch_time.py: n >= 16 Plummer spheres (seed 42 + s), G = 1, eps = 0.01, max_level 16,
             dt_max = 1/16; n = 3 the binary-with-a-perturber systems of tests/hermite_batch_cases.py
  table 2    1,024 of those triples, a drawn quarter with stars whose radii touch within the first macro steps
             (tests/hermite_batch_events_cases.py): ONE advance(64) with the closest approach tracked, (s) with
             stop-on-contact against (n) without it, on this tree; the systems stopped and the macro steps done
  reading    wall-clock ms; every shape is warmed up by one macro step (table 2: primed again before every reading); ROUNDS
             rounds of the child processes (p), (c), (t) in turn, each under its own time limit, READINGS readings per shape
             and round; the median (min, max) of the ROUNDS x READINGS readings

The first non-zero status of a child ends the run.
usage: python tools/hermite_batch_events_time.py [--parent-tree DIR] [--out profiles/r15_hermite_batch_events.txt]
                                                 [--sizes 3,64,256,1024]
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
SIZES = (3, 64, 256, 1024)
B = 1024
ROUNDS, READINGS = 2, 5
STOP_MACROS, STOP_READINGS = 64, 3
PLUMMER = dict(G=1.0, eps=0.01, dt_max=1.0 / 16, max_level=16)
ETA, ETA_START = 0.02, 0.01


def _calculator(nb, c):
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(c["G"])
    fc.setSofteningParameter(c["eps"])
    return fc


def child(form, tree, sizes):
    """one form, every n: RESULT {n: [ms, ...]}; form "stop": table 2"""
    import numpy as np
    import torch
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    import hermite_batch_cases as bc
    from gpu_util import to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    out = {}
    if form == "stop":
        import hermite_batch_events_cases as ec
        c = bc.TRIPLE
        ics, radii, hit = ec.colliding_triples(B, fraction=0.25)
        ic, off = nb.ic.concat(ics)
        fc = _calculator(nb, c)
        for key, stop in (("n", False), ("s", True)):
            d, _ = to_device(nb, ic)
            ens = nb.BlockHermiteEnsemble()
            ens.setParameters(ETA, ETA_START, c["max_level"])
            ens.setLayout(off)
            ens.setEvents(radii=np.concatenate(radii), track_closest=True, stop_on_contact=stop)
            ms = []
            for _ in range(STOP_READINGS + 1):  # (the first: warm-up)
                d, _ = to_device(nb, ic)
                ens.prime(d, fc, c["dt_max"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ens.advance(d, STOP_MACROS)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            ev = ens.events()
            out[key] = {"ms": ms[1:], "stopped": int((ev["stopped"] == 1).sum()), "with_radii": int(hit.sum()),
                        "macro_steps": int(ev["macro_steps_done"].sum()), "block_steps": int(ens.info()["block_steps"])}
            ens.close()
    else:
        for n in sizes:
            c = bc.TRIPLE if n == 3 else PLUMMER
            ics = bc.triples(B) if n == 3 else [nb.ic.plummer(n, seed=42 + s) for s in range(B)]
            ic, off = nb.ic.concat(ics)
            d, _ = to_device(nb, ic)
            ens = nb.BlockHermiteEnsemble()
            ens.setParameters(ETA, ETA_START, c["max_level"])
            ens.setLayout(off)
            if form == "tracked":
                ens.setEvents(radii=np.full(B * n, 1e-4, np.float32), track_closest=True)
            ens.prime(d, _calculator(nb, c), c["dt_max"])
            ens.advance(d, 1)  # warm-up: the levels settle
            ms = []
            for _ in range(READINGS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ens.advance(d, 1)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            out[n] = ms
            ens.close()
    print("RESULT " + json.dumps({"shapes": out, "device": torch.cuda.get_device_name(0),
                                  "lib": os.path.relpath(nb._lib.LIB_PATH, tree)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_hermite_batch_events.txt"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--parent-tree", default=None, help="a built tree whose plain kernel is (p)")
    ap.add_argument("--form", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    if a.form:
        return child(a.form, a.tree, sizes)
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as fh:  # (kept current: a run that is cut short leaves its rows behind)
            fh.write("\n".join(lines) + "\n")

    def run(form, tree):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--form", form, "--tree", tree,
               "--sizes", a.sizes]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"{form}: status {r.returncode}; stopping")
            sys.exit(r.returncode)
        return json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))

    forms = (("p", "plain", parent), ("c", "plain", ROOT), ("t", "tracked", ROOT))
    got = {k: [] for k, _, _ in forms}
    for _ in range(ROUNDS):
        for key, form, tree in forms:
            got[key].append(run(form, tree))
    say(f"tools/hermite_batch_events_time.py on {got['c'][0]['device']}: ms per advance(1) of B = {B} systems + synchronisation, "
        f"median (min, max) of {ROUNDS} x {READINGS} readings, child processes (p), (c), (t) in turn")
    say(f"  (p) the plain kernel, {got['p'][0]['lib']} of {'the tree given with --parent-tree' if a.parent_tree else 'this tree'}; "
        f"(c) the plain kernel of this tree; (t) this tree, closest approach tracked, radii 1e-4, nothing stopping")
    for n in sizes:
        row = {}
        for key in ("p", "c", "t"):
            ms = [v for r in got[key] for v in r["shapes"][str(n)]]
            row[key] = (statistics.median(ms), min(ms), max(ms))
        say(f"n = {n:5d}  (p) {row['p'][0]:9.3f} ({row['p'][1]:.3f}, {row['p'][2]:.3f})  (c) {row['c'][0]:9.3f} ({row['c'][1]:.3f}, "
            f"{row['c'][2]:.3f})  (t) {row['t'][0]:9.3f} ({row['t'][1]:.3f}, {row['t'][2]:.3f}) ms  (c)/(p) = "
            f"{row['c'][0] / row['p'][0]:.3f}  spread of (p), max/min = {row['p'][2] / row['p'][1]:.3f}  (t)/(c) = "
            f"{row['t'][0] / row['c'][0]:.3f}  spread of (t), max/min = {row['t'][2] / row['t'][1]:.3f}")
    stop = run("stop", ROOT)["shapes"]
    say(f"{B} triples, {stop['s']['with_radii']} with radii that touch, ONE advance({STOP_MACROS}), closest approach tracked, "
        f"median (min, max) of {STOP_READINGS} readings, each from a fresh priming")
    for key, name in (("n", "(n) no stopping     "), ("s", "(s) stop on contact ")):
        r = stop[key]
        say(f"  {name} {statistics.median(r['ms']):9.3f} ({min(r['ms']):.3f}, {max(r['ms']):.3f}) ms  {r['stopped']} systems stopped, "
            f"{r['macro_steps']} macro steps and {r['block_steps']} block steps done")
    say(f"  (n)/(s) = {statistics.median(stop['n']['ms']) / statistics.median(stop['s']['ms']):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
