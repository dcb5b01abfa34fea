"""The block-step Hermite family of this tree against the tree given with --parent-tree (the parent commit), A/B: the
BITS of every form that runs the shared resident block step or the merged narrow kernel, and
their TIME.

  bits   per case one SHA-256 over every state array: the 13 arrays of the particle data (x, v, a, a_old, mass), jerk,
         levels, ticks, want, X / V of the extended state, the counters and -- ensembles with events -- the records.
           resident n    one system, "resident" scheduling, advance(3), n = 1, 5, 257, 1,025, 4,096
           narrow n      one system, "host" scheduling with setTuning(1 << 30) (every block step takes the narrow kernel),
                         advance(1), n = 257, 1,025
           mixed         the ensemble of sizes 3, 257, 5, 1,025, 64, 1 of tests/test_hermite_batch_gpu.py, advance(2)
           mixed events  the same with the closest approach tracked, radii of 0.02 and stop-on-contact, advance(4)
           triples ev.   64 colliding triples of tests/hermite_batch_events_cases.py, tracked, stop-on-contact, advance(8)
         each in fp32 and extended state precision, with eps = 0.05 (the packed pair body) and eps = 0 (the guarded one);
         Plummer spheres with general masses, G = 1.7, dt_max = 1/16, max_level 16 (the triples: their own constants).
         Every digest has to be equal between the trees.
  time   wall-clock ms around one call plus the synchronisation, every shape warmed up by one macro step, ROUNDS rounds of
         READINGS readings: "resident" advance(1) at n = 64, 1,024, 4,096; ensembles of B = 1,024 systems of n = 3, 64,
         256, plain and tracked (radii 1e-4, nothing stopping); the host-narrow form at n = 4,096.  Systems as
         tools/hermite_batch_events_time.py.  Criterion per row: median(this) / median(parent) inside the spread of the
         parent's own readings, max / min.

--cases wide: the same A/B for the forms that run the tiled sweep direct_jerk_kernel, the priming sweep and the merged
per-body passes, each in fp32 and extended state precision:
  bits   shared n      HermiteIntegrator.integrate_steps(dt = 1/1024, 2 steps) at n = 1, 2, 255, 257, 1,000, 12,289, 32,768
                       (a partial tile, several source splits, four targets per lane); the digest takes in getJerk and
                       suggestTimeStep
         wide n        "host" scheduling with setTuning(1) (every block step takes the wide kernel), advance(1) with
                       max_level 6 at n = 257, 1,000, 12,289 and with max_level 0 at n = 32,768 (all bodies active: the
                       gathered kernels with four targets per lane)
  time   the shared step at N = 4,096 (20 steps per reading) and 65,536 (3 steps); one host-scheduled macro step at
         N = 65,536 (the system of tools/hermite_block_time.py); the priming of B = 1,024 systems of n = 64 and 256; and, in
         extended precision only, what the list above times in fp32: "resident" advance(1) at n = 1,024 and the ensemble
         of n = 256 (their kernels inline the merged predictor and corrector).

Child processes of the two trees in turn, each under its own time limit; the first non-zero status ends the run.  Exit
code 1 when a digest differs.
usage: python tools/resident_step_ab.py --parent-tree DIR [--cases resident|wide] [--out FILE]
       (--out defaults to profiles/r16_resident_step_ab.txt, profiles/r17_hermite_wide_ab.txt)
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, READINGS = 2, 5
B = 1024
G, DT, MAX_LEVEL = 1.7, 1.0 / 16, 16
ETA, ETA_START = 0.02, 0.01
FORMS = [("fp32", 0.05), ("fp32", 0.0), ("extended", 0.05), ("extended", 0.0)]
RESIDENT_N, NARROW_N = (1, 5, 257, 1025, 4096), (257, 1025)
SHARED_N, SHARED_DT = (1, 2, 255, 257, 1000, 12289, 32768), 1.0 / 1024
WIDE_N = ((257, 6), (1000, 6), (12289, 6), (32768, 0))  # (n, max_level)
OUT = {"resident": "r16_resident_step_ab.txt", "wide": "r17_hermite_wide_ab.txt"}
MIXED = (3, 257, 5, 1025, 64, 1)
TIME_PLUMMER = dict(G=1.0, eps=0.01, dt_max=1.0 / 16, max_level=16)
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")


def child(form, tree, cases):
    import numpy as np
    import torch
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    import hermite_batch_cases as bc
    import hermite_batch_events_cases as ec
    from gpu_util import to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)

    def calculator(g, eps):
        fc = nb.DirectForceCalculator()
        fc.setGravitationalConstant(g)
        fc.setSofteningParameter(eps)
        return fc

    def plummer(n, seed):  # (general masses, as the ensemble tests)
        ic = dict(nb.ic.plummer(n, seed=seed))
        ic["mass"] = (ic["mass"] * np.random.default_rng(5 + seed).uniform(0.5, 2.0, ic["mass"].size)).astype(np.float32)
        return ic

    def digest(d, integ, infos, events=None):
        h = hashlib.sha256()
        for k in F:
            h.update(getattr(d, k).cpu().numpy().tobytes())
        st = integ.getState()
        for k in ("jerk", "levels", "ticks", "want"):
            h.update(np.ascontiguousarray(st[k]).tobytes())
        if integ.getStatePrecision() == "extended":
            for a in integ.getExtendedState(d):
                h.update(np.ascontiguousarray(a).tobytes())
        h.update(json.dumps(infos, sort_keys=True).encode())
        if events is not None:
            h.update(events.tobytes())
        return h.hexdigest()

    def single(n, precision, eps, scheduling, macros, narrow_below=1 << 30, max_level=MAX_LEVEL):
        d, _ = to_device(nb, plummer(n, 42))
        b = nb.BlockHermiteIntegrator()
        b.setParameters(ETA, ETA_START, max_level)
        b.setStatePrecision(precision)
        b.setScheduling(scheduling)
        if scheduling == "host":
            b.setTuning(narrow_below)
        b.advance(d, calculator(G, eps), DT, macros)
        info = b.info()
        if narrow_below == 1:  # (no active set is smaller than 1: every block step is wide)
            assert info["wide_launches"] == info["block_steps"] > 0 and info["narrow_launches"] == 0, info
        else:
            assert (info["wide_launches"], info["narrow_launches"] == 0) == (0, scheduling == "resident"), info
        out = digest(d, b, info)
        b.close()
        return out

    def shared(n, precision, eps):
        d, _ = to_device(nb, plummer(n, 42))
        hi = nb.HermiteIntegrator()
        hi.setStatePrecision(precision)
        hi.integrate_steps(d, calculator(G, eps), SHARED_DT, 2)
        h = hashlib.sha256()
        for k in F:
            h.update(getattr(d, k).cpu().numpy().tobytes())
        h.update(hi.getJerk().cpu().numpy().tobytes())
        h.update(np.float32(hi.suggestTimeStep()).tobytes())
        if precision == "extended":
            for a in hi.getExtendedState(d):
                h.update(np.ascontiguousarray(a).tobytes())
        hi.close()
        return h.hexdigest()

    def ensemble(ics, c, precision, eps, macros, radii=None):
        ic, off = nb.ic.concat(ics)
        d, _ = to_device(nb, ic)
        ens = nb.BlockHermiteEnsemble()
        ens.setParameters(ETA, ETA_START, c["max_level"])
        ens.setStatePrecision(precision)
        ens.setLayout(off)
        if radii is not None:
            ens.setEvents(radii=radii, track_closest=True, stop_on_contact=True)
        ens.prime(d, calculator(c["G"], eps), c["dt_max"])
        ens.advance(d, macros)
        out = digest(d, ens, [ens.info(s) for s in range(len(ics))], None if radii is None else ens.events())
        ens.close()
        return out

    def readings(call):
        call()  # warm-up: the levels settle
        ms = []
        for _ in range(READINGS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    out = {}
    if cases == "wide" and form == "bits":
        for precision, eps in FORMS:
            tag = f"{precision:8s} eps {eps:4.2f}"
            for n in SHARED_N:
                out[f"shared n = {n:5d}  {tag}"] = shared(n, precision, eps)
            for n, max_level in WIDE_N:
                out[f"wide   n = {n:5d}  {tag}"] = single(n, precision, eps, "host", 1, 1, max_level)
    elif cases == "wide":
        c = TIME_PLUMMER
        fc = calculator(c["G"], c["eps"])
        for precision in ("fp32", "extended"):
            for n, steps in ((4096, 20), (65536, 3)):
                d, _ = to_device(nb, nb.ic.plummer(n, seed=42))
                hi = nb.HermiteIntegrator()
                hi.setStatePrecision(precision)
                out[f"shared x {steps:2d}     N = {n:5d}  {precision:8s}"] = readings(
                    lambda: hi.integrate_steps(d, fc, c["dt_max"] / 256, steps))
                hi.close()
            d, _ = to_device(nb, nb.ic.plummer(65536, seed=42))
            b = nb.BlockHermiteIntegrator()
            b.setParameters(ETA, ETA_START, c["max_level"])
            b.setStatePrecision(precision)
            out[f"host macro step N = 65536  {precision:8s}"] = readings(lambda: b.advance(d, fc, c["dt_max"], 1))
            b.close()
            for n in (64, 256):
                ic, off = nb.ic.concat([nb.ic.plummer(n, seed=42 + s) for s in range(B)])
                d, _ = to_device(nb, ic)
                ens = nb.BlockHermiteEnsemble()
                ens.setParameters(ETA, ETA_START, c["max_level"])
                ens.setStatePrecision(precision)
                ens.setLayout(off)
                out[f"ens. priming     n = {n:5d}  {precision:8s}"] = readings(lambda: ens.prime(d, fc, c["dt_max"]))
                if (n, precision) == (256, "extended"):
                    out[f"ens. advance     n = {n:5d}  {precision:8s}"] = readings(lambda: ens.advance(d, 1))
                ens.close()
        d, _ = to_device(nb, nb.ic.plummer(1024, seed=42))
        b = nb.BlockHermiteIntegrator()
        b.setParameters(ETA, ETA_START, c["max_level"])
        b.setStatePrecision("extended")
        b.setScheduling("resident")
        out["resident         n =  1024  extended"] = readings(lambda: b.advance(d, fc, c["dt_max"], 1))
        b.close()
    elif form == "bits":
        plain = dict(G=G, dt_max=DT, max_level=MAX_LEVEL)
        mixed = [plummer(n, 100 + k) for k, n in enumerate(MIXED)]
        triples, tradii, _ = ec.colliding_triples(64)
        for precision, eps in FORMS:
            tag = f"{precision:8s} eps {eps:4.2f}"
            for n in RESIDENT_N:
                out[f"resident n = {n:4d}  {tag}"] = single(n, precision, eps, "resident", 3)
            for n in NARROW_N:
                out[f"narrow   n = {n:4d}  {tag}"] = single(n, precision, eps, "host", 1)
            out[f"mixed             {tag}"] = ensemble(mixed, plain, precision, eps, 2)
            out[f"mixed, events     {tag}"] = ensemble(mixed, plain, precision, eps, 4, np.full(sum(MIXED), 0.02, np.float32))
            out[f"triples, events   {tag}"] = ensemble(triples, bc.TRIPLE, precision, eps, 8, np.concatenate(tradii))
    else:
        c = TIME_PLUMMER
        for key, n, scheduling in (("resident      n =   64", 64, "resident"), ("resident      n = 1024", 1024, "resident"),
                                   ("resident      n = 4096", 4096, "resident"), ("host-narrow   n = 4096", 4096, "host")):
            d, _ = to_device(nb, nb.ic.plummer(n, seed=42))
            b = nb.BlockHermiteIntegrator()
            b.setParameters(ETA, ETA_START, c["max_level"])
            b.setScheduling(scheduling)
            if scheduling == "host":
                b.setTuning(1 << 30)
            fc = calculator(c["G"], c["eps"])
            out[key] = readings(lambda: b.advance(d, fc, c["dt_max"], 1))
            b.close()
        for n in (3, 64, 256):
            cc = bc.TRIPLE if n == 3 else c
            ics = bc.triples(B) if n == 3 else [nb.ic.plummer(n, seed=42 + s) for s in range(B)]
            ic, off = nb.ic.concat(ics)
            for name in ("plain", "tracked"):
                d, _ = to_device(nb, ic)
                ens = nb.BlockHermiteEnsemble()
                ens.setParameters(ETA, ETA_START, cc["max_level"])
                ens.setLayout(off)
                if name == "tracked":
                    ens.setEvents(radii=np.full(B * n, 1e-4, np.float32), track_closest=True)
                ens.prime(d, calculator(cc["G"], cc["eps"]), cc["dt_max"])
                out[f"ens. {name:7s}  n = {n:4d}"] = readings(lambda: ens.advance(d, 1))
                ens.close()
    print("RESULT " + json.dumps({"rows": out, "device": torch.cuda.get_device_name(0),
                                  "lib": os.path.relpath(nb._lib.LIB_PATH, tree)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="resident", choices=sorted(OUT), help="the case list (see above)")
    ap.add_argument("--parent-tree", default=None, help="a built tree of the parent commit")
    ap.add_argument("--form", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.form:
        return child(a.form, a.tree, a.cases)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", OUT[a.cases])
    if not a.parent_tree:
        ap.error("--parent-tree is required")
    parent = os.path.abspath(a.parent_tree)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as fh:  # (kept current: a run that is cut short leaves its rows behind)
            fh.write("\n".join(lines) + "\n")

    def run(form, tree):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--form", form, "--tree", tree,
               "--cases", a.cases]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"{form} of {tree}: status {r.returncode}; stopping")
            sys.exit(r.returncode)
        print(f"  ({form} of {tree}: {time.perf_counter() - t0:.0f} s)", flush=True)
        return json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))

    bits_p, bits_c = run("bits", parent), run("bits", ROOT)
    say(f"tools/resident_step_ab.py --cases {a.cases} on {bits_c['device']}: (p) {bits_p['lib']} of the tree given with --parent-tree, (c) "
        f"{bits_c['lib']} of this tree")
    say("SHA-256 (first 16 digits) over x, v, a, a_old, mass, jerk, levels, ticks, want, X / V, the counters and the event records")
    differ = 0
    for k, v in bits_c["rows"].items():
        same = bits_p["rows"][k] == v
        differ += not same
        say(f"  {k}  (p) {bits_p['rows'][k][:16]}  (c) {v[:16]}  {'equal' if same else 'DIFFERENT'}")
    say(f"{len(bits_c['rows'])} cases, {differ} with different digests")

    got = {"p": [], "c": []}
    for _ in range(ROUNDS):
        got["p"].append(run("time", parent))
        got["c"].append(run("time", ROOT))
    say(f"ms per call + synchronisation, median (min, max) of {ROUNDS} x {READINGS} readings, child processes (p), (c) in turn; "
        f"ensembles: B = {B} systems")
    outside = 0
    for k in got["c"][0]["rows"]:
        row = {}
        for key in ("p", "c"):
            ms = [v for r in got[key] for v in r["rows"][k]]
            row[key] = (statistics.median(ms), min(ms), max(ms))
        ratio, spread = row["c"][0] / row["p"][0], row["p"][2] / row["p"][1]
        verdict = "SLOWER" if ratio > spread else "faster" if ratio < 1.0 / spread else "inside"
        outside += ratio > spread
        say(f"  {k}  (p) {row['p'][0]:9.3f} ({row['p'][1]:.3f}, {row['p'][2]:.3f})  (c) {row['c'][0]:9.3f} ({row['c'][1]:.3f}, "
            f"{row['c'][2]:.3f}) ms  (c)/(p) = {ratio:.3f}  spread of (p), max/min = {spread:.3f}  {verdict}")
    say(f"{len(got['c'][0]['rows'])} rows, {outside} slower than the spread of (p) allows")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
