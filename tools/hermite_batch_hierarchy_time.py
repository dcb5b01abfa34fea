"""What the ensemble HIERARCHIES (EnsembleHierarchy) cost and what they are for.

  table 1    B = 1,024 systems of n bodies, the median advance(1) plus the stream synchronisation after it, in ONE process
             with the forms taken in turn inside every round:
               (u) the escape test alone (r_esc = 1e6: record-only, nothing escapes): the untracked sweep under the record
                   logic, the form a hierarchy-only handle is nearest to
               (h) the examination alone (r_sep = 1e6, kappa = 1: record-only, nothing resolves, so EVERY boundary is
                   examined with all its rounds)
             systems as tools/hermite_batch_outcomes_time.py: n >= 16 Plummer spheres (seed 42 + s), G = 1, eps = 0.01,
             max_level 16, dt_max = 1/16; n = 3 the binary-with-a-perturber systems of tests/hermite_batch_cases.py
  table 2    the 1,024 binary-single scatterings of that tool (seed 2025; G = 1, eps = 0, dt_max = 1/4, max_level 12): ONE
             advance(64) with (e) stop-on-escape, r_esc = 8; (r) stop-when-resolved, r_sep = 8, kappa = 2; (n) the
             examination record-only; the systems stopped, the macro steps done, and the census of the forests on record
  reading    wall-clock ms; every shape is warmed up by one macro step (table 2: primed again before every reading);
             ROUNDS x READINGS readings per form, the median (min, max)

usage: python tools/hermite_batch_hierarchy_time.py [--out profiles/r22_hermite_batch_hierarchy.txt] [--sizes 3,64]
"""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
B, ROUNDS, READINGS = 1024, 3, 5
STOP_MACROS, STOP_READINGS = 64, 3


def _ensemble(nb, np, ics, c, configure):
    from gpu_util import to_device
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, c["max_level"])
    ens.setLayout(offsets)
    hier, out = nb.EnsembleHierarchy(ens), nb.EnsembleOutcomes(ens)
    configure(hier, out)
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(c["G"])
    fc.setSofteningParameter(c["eps"])
    return d, ens, hier, out, fc, ic


def _ms(ctx, f):
    ctx.synchronize()
    t = time.perf_counter()
    f()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t)


def _fmt(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f}, {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="3,64")
    args = ap.parse_args()
    import numpy as np
    import torch
    import nbody_amd as nb
    import hermite_batch_cases as bc
    import hermite_batch_outcomes_time as ot
    ctx = nb.default_context()
    lines = [f"tools/hermite_batch_hierarchy_time.py on {torch.cuda.get_device_name(0)}: ms per advance(1) of B = {B} systems + "
             f"synchronisation, median (min, max) of {ROUNDS} x {READINGS} readings, one process, the forms in turn",
             "  (u) the escape test alone (r_esc 1e6, record-only); (h) the examination alone (r_sep 1e6, kappa 1, record-only: "
             "every boundary examined in full)"]
    forms = {"u": lambda h, o: o.set(1.0e6), "h": lambda h, o: h.set(1.0e6, isolation=1.0)}
    for n in [int(s) for s in args.sizes.split(",")]:
        ics = bc.triples(B) if n == 3 else [nb.ic.plummer(n, seed=42 + s) for s in range(B)]
        runs = {}
        for tag, conf in forms.items():
            d, ens, _, _, fc, _ = _ensemble(nb, np, ics, ot.PLUMMER, conf)
            ens.prime(d, fc, ot.PLUMMER["dt_max"])
            ens.advance(d, 1)
            runs[tag] = (d, ens, [])
        for _ in range(ROUNDS):
            for tag, (d, ens, got) in runs.items():
                for _ in range(READINGS):
                    got.append(_ms(ctx, lambda: ens.advance(d, 1)))
        u, h = runs["u"][2], runs["h"][2]
        lines.append(f"n = {n:5d}  (u) {_fmt(u)}  (h) {_fmt(h)} ms  (h)/(u) = {statistics.median(h) / statistics.median(u):.3f}  "
                     f"spread of (u), max/min = {max(u) / min(u):.3f}")
        for _, ens, _ in runs.values():
            ens.close()
    c = ot.SCATTER
    ics = ot.scatterings(np, B, c["seed"])
    lines.append(f"{B} binary-single scatterings, ONE advance({STOP_MACROS}), median (min, max) of {STOP_READINGS} readings, each from a "
                 "fresh priming")
    stops = {"(e) stop on escape, r_esc 8    ": lambda h, o: o.set(c["r_esc"], stop_on_escape=True),
             "(r) stop when resolved, r_sep 8": lambda h, o: h.set(c["r_esc"], isolation=2.0, stop_on_resolved=True),
             "(n) examination record-only    ": lambda h, o: h.set(c["r_esc"], isolation=2.0)}
    for tag, conf in stops.items():
        d, ens, hier, out, fc, ic = _ensemble(nb, np, ics, c, conf)
        got = []
        for _ in range(STOP_READINGS):
            for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
                getattr(d, k).copy_(torch.from_numpy(np.ascontiguousarray(ic[k])))
            ens.prime(d, fc, c["dt_max"])
            got.append(_ms(ctx, lambda: ens.advance(d, STOP_MACROS)))
        ev, rec, nodes = ens.events(), hier.records(), hier.nodes()
        census = collections.Counter(hier.describe(s, nodes) for s in range(B) if rec["resolved"][s])
        lines.append(f"  {tag} {_fmt(got)} ms  {int((ev['stopped'] != 0).sum())} stopped, {int(ev['macro_steps_done'].sum())} macro steps done, "
                     f"{int(rec['resolved'].sum())} resolved" + (f": {dict(sorted(census.items()))}" if census else ""))
        ens.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
