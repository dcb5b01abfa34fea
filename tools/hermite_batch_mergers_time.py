"""What the ensemble MERGERS (EnsembleMergers) cost and what they are for.

  table (a)  B = 1,024 systems of n bodies, the median advance(1) plus the stream synchronisation after it:
               (p) the plain kernel of the tree given with --parent-tree (the parent commit; default this tree)
               (c) the plain kernel of this tree, mergers off: the same kernel, so (c) / (p) has to lie inside (p)'s spread
             systems as tools/hermite_batch_events_time.py: n >= 16 Plummer spheres (seed 42 + s), G = 1, eps = 0.01,
             max_level 16, dt_max = 1/16; n = 3 the binary-with-a-perturber systems of tests/hermite_batch_cases.py
  table (b)  the same ensembles with stop-on-contact and mergers on: one apply() plus the synchronisation after it,
               (i) with no system stopped (every workgroup leaves at once; the two priming kernels find no mark)
               (q) with a quarter of the systems stopped: bodies 0 and 1 of every fourth system get radii that overlap
                   from the start, advance(1) stops them, the timed apply() merges them (each reading from a fresh priming)
             each as a share of the advance(1) of the same ensemble
  table (c)  what the feature is for: 1,024 triples of which a drawn quarter touch early
             (tests/hermite_batch_events_cases.py), 64 macro steps:
               (d) run(d, 64, every=1) on the device: 64 x [advance(1), apply()], one synchronisation at the end
               (h) the host route a user has without it: 64 x [advance(1), read the event records; if a system stopped
                   on contact: read the state back, merge in numpy (tests/hermite_batch_mergers_ref.py), rebuild the
                   arrays, the layout and the radii, upload, prime the WHOLE ensemble again]
             both times and the number of mergers
  reading    wall-clock ms; ROUNDS rounds of the child processes in turn, each under its own time limit, READINGS
             readings per shape and round; the median (min, max) of the ROUNDS x READINGS readings

The first non-zero status of a child ends the run.
usage: python tools/hermite_batch_mergers_time.py [--parent-tree DIR] [--out profiles/r23_hermite_batch_mergers_time.txt]
                                                  [--sizes 3,64,1024]
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
SIZES = (3, 64, 1024)
B = 1024
ROUNDS, READINGS = 2, 5
RUN_MACROS, RUN_READINGS = 64, 2
PLUMMER = dict(G=1.0, eps=0.01, dt_max=1.0 / 16, max_level=16)
ETA, ETA_START = 0.02, 0.01


def _calculator(nb, c):
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(c["G"])
    fc.setSofteningParameter(c["eps"])
    return fc


def _timed(torch, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def child(form, tree, sizes):
    """one form: RESULT {shape: ...}"""
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

    def systems(n):
        c = bc.TRIPLE if n == 3 else PLUMMER
        return c, (bc.triples(B) if n == 3 else [nb.ic.plummer(n, seed=42 + s) for s in range(B)])

    def ensemble(c, off, radii=None):
        ens = nb.BlockHermiteEnsemble()
        ens.setParameters(ETA, ETA_START, c["max_level"])
        ens.setLayout(off)
        if radii is not None:
            ens.setEvents(radii=radii, stop_on_contact=True)
        return ens

    if form == "plain":
        for n in sizes:
            c, ics = systems(n)
            ic, off = nb.ic.concat(ics)
            d, _ = to_device(nb, ic)
            ens = ensemble(c, off)
            ens.prime(d, _calculator(nb, c), c["dt_max"])
            ens.advance(d, 1)  # warm-up: the levels settle
            out[n] = [_timed(torch, lambda: ens.advance(d, 1)) for _ in range(READINGS)]
            ens.close()
    elif form == "apply":
        for n in sizes:
            c, ics = systems(n)
            ic, off = nb.ic.concat(ics)
            fc = _calculator(nb, c)
            row = {}
            for key, every in (("i", 0), ("q", 4)):
                radii = np.zeros(B * n, np.float32)
                for s in (range(0, B, every) if every else ()):
                    a = int(off[s])
                    sep = np.sqrt(sum((np.float64(ic[k][a]) - np.float64(ic[k][a + 1])) ** 2 for k in ("pos_x", "pos_y", "pos_z")))
                    radii[a] = radii[a + 1] = 0.505 * sep
                ens = ensemble(c, off, radii)
                mg = nb.EnsembleMergers(ens)
                mg.set()
                adv, app = [], []
                for _ in range(READINGS + 1):  # (the first: warm-up)
                    d, _ = to_device(nb, ic)
                    ens.setEvents(radii=radii, stop_on_contact=True)  # (a pass changes the radii of what it merged)
                    ens.prime(d, fc, c["dt_max"])
                    adv.append(_timed(torch, lambda: ens.advance(d, 1)))
                    stopped = int((ens.events()["stopped"] == 1).sum())
                    app.append(_timed(torch, lambda: mg.apply(d)))
                row[key] = {"advance": adv[1:], "apply": app[1:], "stopped": stopped,
                            "merged": int((mg.records()["n_mergers"] > 0).sum())}
                ens.close()
            out[n] = row
    else:  # "run": table (c)
        import hermite_batch_events_cases as ec
        import hermite_batch_mergers_ref as mref
        c = bc.TRIPLE
        ics, radii, hit = ec.colliding_triples(B, fraction=0.25)
        ic, off = nb.ic.concat(ics)
        fc = _calculator(nb, c)
        r0 = np.concatenate(radii)
        dev, host = [], []
        for _ in range(RUN_READINGS + 1):  # (the first: warm-up)
            d, _ = to_device(nb, ic)
            ens = ensemble(c, off, r0)
            mg = nb.EnsembleMergers(ens)
            mg.set()
            ens.prime(d, fc, c["dt_max"])
            dev.append(_timed(torch, lambda: mg.run(d, RUN_MACROS, every=1)))
            n_dev = int(mg.records()["n_mergers"].sum())
            ens.close()

            def host_route():
                cur, o, r = {k: v.copy() for k, v in ic.items()}, np.asarray(off).astype(np.int64), r0.copy()
                d, _ = to_device(nb, cur)
                ens = ensemble(c, o, r)
                ens.prime(d, fc, c["dt_max"])
                merged = 0
                for _ in range(RUN_MACROS):
                    ens.advance(d, 1)
                    ev = ens.events()
                    hitnow = np.flatnonzero(ev["stopped"] == 1)
                    if hitnow.size == 0:
                        continue
                    h = nb.ParticleData()
                    nb.ParticleDataManager.allocateHost(h, d.count)
                    nb.ParticleDataManager.copyToHost(h, d)
                    cur = {k: np.array(getattr(h, k)) for k in cur}
                    keep = np.ones(d.count, bool)
                    for s in hitnow:
                        a, b = int(o[s]), int(o[s + 1])
                        sysr = mref.System(np.stack([cur[k][a:b] for k in ("pos_x", "pos_y", "pos_z")], 1),
                                           np.stack([cur[k][a:b] for k in ("vel_x", "vel_y", "vel_z")], 1), cur["mass"][a:b], r[a:b])
                        if mref.merge(sysr, ev["contact_i"][s], ev["contact_j"][s], c["G"], c["eps"]) is None:
                            continue
                        for x, k in enumerate(("pos_x", "pos_y", "pos_z")):
                            cur[k][a:b] = sysr.pos[:, x]
                        for x, k in enumerate(("vel_x", "vel_y", "vel_z")):
                            cur[k][a:b] = sysr.vel[:, x]
                        cur["mass"][a:b], r[a:b] = sysr.mass, sysr.radii
                        keep[b - 1] = False
                        merged += 1
                    sizes_now = np.array([keep[int(o[s]):int(o[s + 1])].sum() for s in range(o.size - 1)])
                    cur, r = {k: v[keep] for k, v in cur.items()}, r[keep]
                    o = np.concatenate([[0], np.cumsum(sizes_now)]).astype(np.int64)
                    d, _ = to_device(nb, cur)
                    ens.setLayout(o)
                    ens.setEvents(radii=r, stop_on_contact=True)
                    ens.prime(d, fc, c["dt_max"])  # (the whole ensemble: every counter and record starts over)
                torch.cuda.synchronize()
                ens.close()
                return merged

            t0 = time.perf_counter()
            n_host = host_route()
            host.append((time.perf_counter() - t0) * 1e3)
        out = {"device": dev[1:], "host": host[1:], "mergers_device": n_dev, "mergers_host": n_host, "with_radii": int(hit.sum())}
    print("RESULT " + json.dumps({"shapes": out, "device": torch.cuda.get_device_name(0),
                                  "lib": os.path.relpath(nb._lib.LIB_PATH, tree)}), flush=True)


def _mmm(ms):
    return f"{statistics.median(ms):9.3f} ({min(ms):.3f}, {max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_hermite_batch_mergers_time.txt"))
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

    def run(form, tree, limit=300):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--form", form, "--tree", tree,
               "--sizes", a.sizes]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"{form}: status {r.returncode}; stopping")
            sys.exit(r.returncode)
        return json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))

    got = {"p": [], "c": []}
    for _ in range(ROUNDS):
        got["p"].append(run("plain", parent))
        got["c"].append(run("plain", ROOT))
    say(f"tools/hermite_batch_mergers_time.py on {got['c'][0]['device']}: (a) ms per advance(1) of B = {B} systems + "
        f"synchronisation, median (min, max) of {ROUNDS} x {READINGS} readings, child processes (p), (c) in turn")
    say(f"  (p) the plain kernel, {got['p'][0]['lib']} of {'the tree given with --parent-tree' if a.parent_tree else 'this tree'}; "
        f"(c) the plain kernel of this tree, mergers off")
    for n in sizes:
        p = [v for r in got["p"] for v in r["shapes"][str(n)]]
        c = [v for r in got["c"] for v in r["shapes"][str(n)]]
        say(f"n = {n:5d}  (p) {_mmm(p)}  (c) {_mmm(c)} ms  (c)/(p) = {statistics.median(c) / statistics.median(p):.3f}  "
            f"spread of (p), max/min = {max(p) / min(p):.3f}")
    app = [run("apply", ROOT) for _ in range(ROUNDS)]
    say(f"(b) one apply() + synchronisation, stop-on-contact and mergers on, median (min, max) of {ROUNDS} x {READINGS} "
        f"readings, each after a fresh priming and advance(1); share of that advance(1)")
    for n in sizes:
        for key, name in (("i", "(i) nobody stopped  "), ("q", "(q) a quarter stopped")):
            rows = [r["shapes"][str(n)][key] for r in app]
            ms, adv = [v for r in rows for v in r["apply"]], [v for r in rows for v in r["advance"]]
            say(f"n = {n:5d}  {name} apply {_mmm(ms)} ms  advance(1) {_mmm(adv)} ms  share {statistics.median(ms) / statistics.median(adv):.4f}"
                f"  {rows[0]['stopped']} systems stopped, {rows[0]['merged']} merged")
    r = run("run", ROOT, limit=420)["shapes"]
    say(f"(c) {B} triples, {r['with_radii']} with radii that touch, {RUN_MACROS} macro steps, median (min, max) of {RUN_READINGS} readings")
    say(f"  (d) run(d, {RUN_MACROS}, every=1) on the device   {_mmm(r['device'])} ms  {r['mergers_device']} mergers")
    say(f"  (h) the host route (read back, numpy, prime)  {_mmm(r['host'])} ms  {r['mergers_host']} mergers")
    say(f"  (h)/(d) = {statistics.median(r['host']) / statistics.median(r['device']):.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
