"""The ensemble diagnostics (BlockHermiteEnsemble.diagnostics_into) against what a user did before
them, and against the macro step they follow: B independent systems of n bodies each, the ensembles of section 4.13's table.

  systems    n >= 16: Plummer spheres (seed 42 + s), G = 1, eps = 0.01, eta = 0.02, max_level = 16, dt_max = 1/16; n = 3: the
             binary-with-a-perturber systems of tests/hermite_batch_cases.py (G = 1.7, eps = 1e-4, max_level = 10)
  (d)        ONE diagnostics_into call for all B systems plus the stream synchronisation after it (the structs stay on the
             device; the blocking form adds a copy of 152 B bytes)
  (h)        the host path: getExtendedState (the fp64 state of all bodies to the host) plus the numpy loop over the systems,
             tests/hermite_ref.energy on each (KE and PE only: no momenta, no pairs).  For B > SUBSET the loop runs on the
             first SUBSET systems and its time is scaled by B / SUBSET; the read-back is always whole.
  (s)        advance(1) of the same ensemble plus the synchronisation
  reading    wall-clock ms; every shape is warmed up by one macro step and one call of each kind; ROUNDS rounds of one fresh
             child process per n, READINGS readings per shape and round in the order s, d, h; median (min, max) of the
             ROUNDS x READINGS readings

Combinations above 2^20 bodies are skipped.  The first non-zero status of a child ends the run.
usage: python tools/system_diag_time.py [--out profiles/r14_system_diag.txt] [--sizes 3,64] [--systems 64,1024]
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
SYSTEMS = (64, 1024, 4096)
MAX_BODIES = 1 << 20
SUBSET = 64
ROUNDS, READINGS = 2, 5
PLUMMER = dict(G=1.0, eps=0.01, dt_max=1.0 / 16, max_level=16)
ETA, ETA_START = 0.02, 0.01


def shapes(n, systems):
    return [b for b in systems if b * n <= MAX_BODIES]


def child(n, systems):
    """one n, every B: RESULT {B: {"d": [...], "h": [...], "s": [...]}} in ms"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    import hermite_batch_cases as bc
    import hermite_ref as hr
    from gpu_util import to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    c = bc.TRIPLE if n == 3 else PLUMMER
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(c["G"])
    fc.setSofteningParameter(c["eps"])
    out = {}
    for B in shapes(n, systems):
        ics = bc.triples(B) if n == 3 else [nb.ic.plummer(n, seed=42 + s) for s in range(B)]
        ic, off = nb.ic.concat(ics)
        off = [int(o) for o in off]
        d, _ = to_device(nb, ic)
        mass = np.asarray(ic["mass"], np.float64)
        ens = nb.BlockHermiteEnsemble()
        ens.setParameters(ETA, ETA_START, c["max_level"])
        ens.setLayout(off)
        ens.prime(d, fc, c["dt_max"])
        buf = nb.system_diag_tensor(B, d.pos_x.device)
        timed = min(B, SUBSET)
        g32 = float(np.float32(c["G"]))  # (the engine's G is the fp32 argument)

        def host():
            t0 = time.perf_counter()
            X, V = ens.getExtendedState(d)
            t1 = time.perf_counter()
            e = [hr.energy(X[off[s]:off[s + 1]], V[off[s]:off[s + 1]], mass[off[s]:off[s + 1]], g32, c["eps"])
                 for s in range(timed)]
            t2 = time.perf_counter()
            return ((t1 - t0) + (t2 - t1) * B / timed) * 1e3, e

        ens.advance(d, 1)  # warm-up: the levels settle
        ens.diagnostics_into(d, buf)
        host()
        torch.cuda.synchronize()
        ms = {"d": [], "h": [], "s": []}
        for _ in range(READINGS):
            t0 = time.perf_counter()
            ens.advance(d, 1)
            torch.cuda.synchronize()
            ms["s"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ens.diagnostics_into(d, buf)
            torch.cuda.synchronize()
            ms["d"].append((time.perf_counter() - t0) * 1e3)
            t, e = host()
            ms["h"].append(t)
        # (the two paths measure the same systems: the device's energies against the host loop's)
        got = nb.system_diag_array(buf)
        assert (got["status"] == 0).all()
        worst = max(abs(got["kinetic"][s] + got["potential"][s] - (e[s][0] + e[s][1])) / abs(e[s][1]) for s in range(timed))
        out[B] = dict(ms, worst=worst, timed_systems=timed)
        ens.close()
    print("RESULT " + json.dumps({"shapes": out, "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_system_diag.txt"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--systems", default=",".join(str(b) for b in SYSTEMS))
    ap.add_argument("--case", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    systems = [int(v) for v in a.systems.split(",")]
    if a.case:
        return child(a.case, systems)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as fh:  # (kept current: a run that is cut short leaves its rows behind)
            fh.write("\n".join(lines) + "\n")

    def run(n):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", str(n), "--systems", a.systems]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"n = {n}: status {r.returncode}; stopping")
            sys.exit(r.returncode)
        return json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))

    for n in (int(v) for v in a.sizes.split(",")):
        got = [run(n) for _ in range(ROUNDS)]
        if not lines:
            say(f"tools/system_diag_time.py on {got[0]['device']}: ms per call + synchronisation, median (min, max) of {ROUNDS} x "
                f"{READINGS} readings, one fresh child process per n and round")
            say("  (d) diagnostics_into, one launch for all systems; (h) getExtendedState + numpy loop of hermite_ref.energy over "
                f"the systems (loops over more than {SUBSET} systems timed on the first {SUBSET} and scaled); (s) advance(1)")
            say("  n >= 16: Plummer spheres, G = 1, eps = 0.01, eta = 0.02, max_level = 16, dt_max = 1/16; n = 3: binary "
                "(e = 0.9) with a perturber, G = 1.7, eps = 1e-4, max_level = 10, dt_max = 1/16")
        for B in shapes(n, systems):
            row = {}
            for key in ("d", "h", "s"):
                ms = [v for r in got for v in r["shapes"][str(B)][key]]
                row[key] = (statistics.median(ms), min(ms), max(ms))
            worst = max(r["shapes"][str(B)]["worst"] for r in got)
            timed = got[0]["shapes"][str(B)]["timed_systems"]
            pairs = B * n * (n - 1) / 2
            say(f"n = {n:5d}  B = {B:5d}  (d) {row['d'][0]:9.3f} ({row['d'][1]:.3f}, {row['d'][2]:.3f}) ms  "
                f"{pairs / row['d'][0] * 1e3:10.3e} pairs/s  (s) {row['s'][0]:9.3f} ({row['s'][1]:.3f}, {row['s'][2]:.3f})  "
                f"(h) {row['h'][0]:10.3f} ({row['h'][1]:.3f}, {row['h'][2]:.3f})  (d)/(s) = {row['d'][0] / row['s'][0]:7.3f}  "
                f"(h)/(d) = {row['h'][0] / row['d'][0]:8.1f}  |E_d - E_h| / |PE| <= {worst:.1e}"
                + (f"  [(h) loop timed on {timed} systems, x {B // timed}]" if timed < B else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
