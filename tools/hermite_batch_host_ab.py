"""The host path of the ensemble's configuration calls and of prime, a built parent tree against
this tree, one fresh child process per reading set under its own time limit, the two trees in turn for ROUNDS rounds.

Per child: B = 1,024 Plummer systems of 16 bodies, primed once with nothing configured.  Wall-clock ms with a device
synchronisation before and after:
  first   the first configuration of all four features (events with radii and stop_on_contact, outcomes, hierarchies,
          mergers: the allocations and the fresh clears) plus prime: one reading per child
  again   all four configured again (no allocation) plus prime: READINGS readings, their median
  prime   prime alone, everything configured (the four clears): READINGS readings, their median
  toggle  events, outcomes, hierarchies and mergers off, then on again: READINGS readings, their median
The yardstick is the parent's median of the rounds' medians; the margin is the spread of the parent's rounds.

usage: python tools/hermite_batch_host_ab.py PARENT_TREE [--out profiles/r24_hermite_batch_plan_host.txt]
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
B, N, READINGS, ROUNDS = 1024, 16, 20, 4


def child(tree):
    import numpy as np
    import torch
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    from gpu_util import to_device
    torch.cuda.set_device(0)
    ic, off = nb.ic.concat([nb.ic.plummer(N, seed=42 + s) for s in range(B)])
    d, _ = to_device(nb, ic)
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(1.0)
    fc.setSofteningParameter(0.01)
    radii = np.full(B * N, 1e-4, np.float32)
    esc, sep = np.full(B, 50.0, np.float32), np.full(B, 20.0, np.float32)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ens = nb.BlockHermiteEnsemble()
    ens.setLayout(off)
    ens.prime(d, fc, 1.0 / 16)  # (the handle exists; nothing configured yet)
    out, hier, mg = nb.EnsembleOutcomes(ens), nb.EnsembleHierarchy(ens), nb.EnsembleMergers(ens)

    def configure():
        ens.setEvents(radii=radii, stop_on_contact=True)
        out.set(esc, stop_on_escape=True)
        hier.set(sep, isolation=1.0, stop_on_resolved=True)
        mg.set()

    def off_on():
        ens.setEvents()
        out.set()
        hier.set()
        mg.set(False)
        configure()

    first = timed(lambda: (configure(), ens.prime(d, fc, 1.0 / 16)))
    again = [timed(lambda: (configure(), ens.prime(d, fc, 1.0 / 16))) for _ in range(READINGS)]
    prime = [timed(lambda: ens.prime(d, fc, 1.0 / 16)) for _ in range(READINGS)]
    toggle = [timed(off_on) for _ in range(READINGS)]
    ens.advance(d, 1)
    print("RESULT " + json.dumps(dict(first=first, again=again, prime=prime, toggle=toggle)), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree", help="a built tree of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_hermite_batch_plan_host.txt"))
    a = ap.parse_args()
    parent, out = os.path.abspath(a.parent_tree), a.out
    got = {"parent": [], "this": []}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as fh:  # (kept current: a run that is cut short leaves its rows behind)
            fh.write("\n".join(lines) + "\n")

    say(f"tools/hermite_batch_host_ab.py: B = {B} systems of {N} bodies, ms, {ROUNDS} rounds of child processes (parent, this) in "
        f"turn, {READINGS} readings per child")

    for r in range(ROUNDS):
        for name, tree in (("parent", parent), ("this", ROOT)):
            p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", tree],
                               capture_output=True, text=True)
            if p.returncode != 0:
                print(p.stdout[-2000:] + p.stderr[-2000:])
                print(f"{name}: status {p.returncode}; stopping")
                return p.returncode
            res = json.loads(re.search(r"^RESULT (.*)$", p.stdout, re.M).group(1))
            got[name].append(res)
            say(f"round {r + 1} {name:6s} first {res['first']:8.3f}  again median {statistics.median(res['again']):7.3f}  "
                f"prime median {statistics.median(res['prime']):7.3f}  toggle median {statistics.median(res['toggle']):7.3f} ms")
    for key in ("again", "prime", "toggle"):
        for name in ("parent", "this"):
            meds = [statistics.median(r[key]) for r in got[name]]
            say(f"{key:6s} {name:6s} median of the rounds' medians {statistics.median(meds):7.3f} ms, rounds (min, max) "
                f"({min(meds):.3f}, {max(meds):.3f})")
    for name in ("parent", "this"):
        f = [r["first"] for r in got[name]]
        say(f"first  {name:6s} median {statistics.median(f):7.3f} ms (min, max) ({min(f):.3f}, {max(f):.3f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
