"""What the ensemble OUTCOMES (EnsembleOutcomes) cost and what they are for.

  table 1    B = 1,024 systems of n bodies, the median advance(1) plus the stream synchronisation after it:
               (p) the event form of the tree given with --parent-tree (the parent commit; default this tree): the closest
                   approach tracked, radii of 1e-4 on every body, nothing stopping
               (c) the same on this tree: the same kernel, so (c) / (p) has to lie inside (p)'s own spread
               (o) this tree, the same events and the escape test besides (r_esc = 1e6: record-only, nothing escapes)
               (u) this tree, the escape test alone: the untracked sweep under the record logic
             systems as tools/hermite_batch_events_time.py: n >= 16 Plummer spheres (seed 42 + s), G = 1, eps = 0.01,
             max_level 16, dt_max = 1/16; n = 3 the binary-with-a-perturber systems of tests/hermite_batch_cases.py
  table 2    1,024 binary-single scatterings (seed 2025): an equal-mass circular binary of separation 0.5 in a drawn
             orientation and phase, a third body of the same mass from a distance of 6 at a drawn speed in [2, 4] and impact
             parameter in [0, 2]; G = 1, eps = 0, dt_max = 1/4, max_level 12, r_esc = 8: ONE advance(64), (s) with
             stop-on-escape against (n) record-only, on this tree; the systems stopped, the macro and block steps done, and
             the median and the largest block-step count of a system (the launch lasts as long as its slowest workgroups)
  reading    wall-clock ms; every shape is warmed up by one macro step (table 2: primed again before every reading); ROUNDS
             rounds of the child processes in turn, each under its own time limit, READINGS readings per shape and round;
             the median (min, max) of the ROUNDS x READINGS readings

The first non-zero status of a child ends the run.
usage: python tools/hermite_batch_outcomes_time.py [--parent-tree DIR] [--out profiles/r19_hermite_batch_outcomes.txt]
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
SCATTER = dict(G=1.0, eps=0.0, dt_max=1.0 / 4, max_level=12, r_esc=8.0, seed=2025)
ETA, ETA_START = 0.02, 0.01


def _calculator(nb, c):
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(c["G"])
    fc.setSofteningParameter(c["eps"])
    return fc


def scatterings(np, count, seed):
    """count binary-single scatterings as initial-condition dicts, in the centre-of-mass frame of each"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))  # a drawn orientation of the binary's plane
        phase = rng.uniform(0.0, 2.0 * np.pi)
        u = np.cos(phase) * q[:, 0] + np.sin(phase) * q[:, 1]
        t = -np.sin(phase) * q[:, 0] + np.cos(phase) * q[:, 1]
        vc = 0.5 * np.sqrt(1.0 / 0.5)  # G (m1 + m2) / a with m1 = m2 = 0.5, a = 0.5: each star moves at half of it
        pos = np.array([0.25 * u, -0.25 * u, [-6.0, rng.uniform(0.0, 2.0), 0.0]])
        vel = np.array([vc * t, -vc * t, [rng.uniform(2.0, 4.0), 0.0, 0.0]])
        m = np.array([0.5, 0.5, 0.5])
        pos -= (m[:, None] * pos).sum(0) / m.sum()
        vel -= (m[:, None] * vel).sum(0) / m.sum()
        keys = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z")
        ic = {k: np.concatenate([pos, vel], 1)[:, c].astype(np.float32) for c, k in enumerate(keys)}
        ic["mass"] = m.astype(np.float32)
        out.append(ic)
    return out


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
        c = SCATTER
        ic, off = nb.ic.concat(scatterings(np, B, c["seed"]))
        fc = _calculator(nb, c)
        for key, stop in (("n", False), ("s", True)):
            d, _ = to_device(nb, ic)
            ens = nb.BlockHermiteEnsemble()
            ens.setParameters(ETA, ETA_START, c["max_level"])
            ens.setLayout(off)
            oc = nb.EnsembleOutcomes(ens)
            oc.set(c["r_esc"], stop_on_escape=stop)
            ms = []
            for _ in range(STOP_READINGS + 1):  # (the first: warm-up)
                d, _ = to_device(nb, ic)
                ens.prime(d, fc, c["dt_max"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ens.advance(d, STOP_MACROS)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            ev, rec = ens.events(), oc.records()
            per_system = sorted(int(ens.info(k)["block_steps"]) for k in range(B))
            out[key] = {"ms": ms[1:], "stopped": int((ev["stopped"] == 3).sum()), "escaped": int((rec["escaped"] > 0).sum()),
                        "median_macro": float(np.median(rec["macro"][rec["escaped"] > 0])) if (rec["escaped"] > 0).any() else 0.0,
                        "macro_steps": int(ev["macro_steps_done"].sum()), "block_steps": int(ens.info()["block_steps"]),
                        "block_steps_max": per_system[-1], "block_steps_median": per_system[B // 2]}
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
            if form in ("tracked", "both"):
                ens.setEvents(radii=np.full(B * n, 1e-4, np.float32), track_closest=True)
            if form in ("both", "outcomes"):
                nb.EnsembleOutcomes(ens).set(1.0e6)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_hermite_batch_outcomes.txt"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--parent-tree", default=None, help="a built tree whose event form is (p)")
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

    forms = (("p", "tracked", parent), ("c", "tracked", ROOT), ("o", "both", ROOT), ("u", "outcomes", ROOT))
    got = {k: [] for k, _, _ in forms}
    for _ in range(ROUNDS):
        for key, form, tree in forms:
            got[key].append(run(form, tree))
    say(f"tools/hermite_batch_outcomes_time.py on {got['c'][0]['device']}: ms per advance(1) of B = {B} systems + "
        f"synchronisation, median (min, max) of {ROUNDS} x {READINGS} readings, child processes (p), (c), (o), (u) in turn")
    say(f"  (p) the event form (closest approach tracked, radii 1e-4, nothing stopping), {got['p'][0]['lib']} of "
        f"{'the tree given with --parent-tree' if a.parent_tree else 'this tree'}; (c) the same on this tree; (o) this tree, "
        f"the same events and the escape test (r_esc 1e6, record-only); (u) this tree, the escape test alone (untracked sweep)")
    for n in sizes:
        row = {}
        for key in got:
            ms = [v for r in got[key] for v in r["shapes"][str(n)]]
            row[key] = (statistics.median(ms), min(ms), max(ms))
        cells = "  ".join(f"({k}) {row[k][0]:9.3f} ({row[k][1]:.3f}, {row[k][2]:.3f})" for k in ("p", "c", "o", "u"))
        say(f"n = {n:5d}  {cells} ms  (c)/(p) = {row['c'][0] / row['p'][0]:.3f}  spread of (p), max/min = "
            f"{row['p'][2] / row['p'][1]:.3f}  (o)/(c) = {row['o'][0] / row['c'][0]:.3f}  spread of (o), max/min = "
            f"{row['o'][2] / row['o'][1]:.3f}  (u)/(c) = {row['u'][0] / row['c'][0]:.3f}")
        if row["p"][2] / row["p"][1] > 2.0:
            say(f"  note: the n = {n} row does not resolve the ratios: the readings of a column are successive macro steps of "
                f"evolving systems, whose cost varies {row['p'][2] / row['p'][1]:.0f}-fold")
    stop = run("stop", ROOT)["shapes"]
    say(f"{B} binary-single scatterings, r_esc = {SCATTER['r_esc']}, ONE advance({STOP_MACROS}), the escape test alone, median "
        f"(min, max) of {STOP_READINGS} readings, each from a fresh priming")
    for key, name in (("n", "(n) record-only    "), ("s", "(s) stop on escape ")):
        r = stop[key]
        say(f"  {name} {statistics.median(r['ms']):9.3f} ({min(r['ms']):.3f}, {max(r['ms']):.3f}) ms  {r['escaped']} systems with an "
            f"escape (median macro index {r['median_macro']:.0f}), {r['stopped']} stopped, {r['macro_steps']} macro steps and "
            f"{r['block_steps']} block steps done (per system: median {r['block_steps_median']}, largest {r['block_steps_max']})")
    say(f"  (n)/(s) = {statistics.median(stop['n']['ms']) / statistics.median(stop['s']['ms']):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
