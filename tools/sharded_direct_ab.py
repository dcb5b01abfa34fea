#!/usr/bin/env python3
"""Two builds of the library on the sharded Direct system (csrc/sharded.hip), for refactors of its host side that must
neither move a bit nor add a host call to the step.

    NBODY_HIP_LIB=path python tools/sharded_direct_ab.py state OUT.npz    every array of the cases below
    NBODY_HIP_LIB=path python tools/sharded_direct_ab.py time             "n ms_per_step" per size, one median per line
    python tools/sharded_direct_ab.py compare LIB_A LIB_B [--rounds 5] [--out F] [--names A B]

state: virtual ranks W in {1, 2, 3, 4, 5, 8} on device 0 (peer copies), n = 30,001, equal and random masses, eps = 0.01
(pair mode) and eps = 0 (the one-sided form): get_state after forces() and after three steps, energies() at both, and
the accelerations of the plugin form (compute_forces on a whole-system ParticleData).
time: nbody_hip_sharded_direct_time_steps at W = 8 virtual ranks, n = 1,048,576 and n = 65,536 (where the host's share
of a step shows); the median of three calls each.
compare: `state` once per build and `time` in alternating rounds, every run a fresh child process.  Every array of A
must equal the array of B (the path is deterministic run to run, so equality is the criterion), and B's median over the
rounds must not lie above the largest of A's rounds.  Exit code 1 otherwise.  Not imported by the product."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (1, 2, 3, 4, 5, 8)
N_STATE = 30001
TIMED = ((1 << 20, 1, 3), (1 << 16, 20, 200))  # n, warmup, steps


def _imports():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import nbody_amd as nb
    from nbody_amd.sharded import Comm, ShardedDirect
    return np, nb, Comm, ShardedDirect


def state(out):
    np, nb, Comm, ShardedDirect = _imports()
    from gpu_util import acc_of, to_device
    arrays = {}
    for W in WORLDS:
        comm = Comm.init_all(W, [0] * W)
        for masses in ("equal", "random"):
            ic = nb.ic.plummer(N_STATE, seed=200 + W)
            if masses == "random":
                ic["mass"] = (ic["mass"] * np.random.default_rng(W).uniform(0.5, 2.0, N_STATE)).astype(np.float32)
            for eps in (0.01, 0.0):
                tag = f"W{W}_{masses}_eps{eps}"
                s = ShardedDirect(comm, N_STATE, 1.3, eps)
                s.set_state(ic)
                s.forces()
                for k, v in s.get_state().items():
                    arrays[f"{tag}_forces_{k}"] = v
                arrays[f"{tag}_forces_energies"] = np.array(s.energies())
                s.step(1e-4 if eps == 0.0 else 1e-3, 3)
                for k, v in s.get_state().items():
                    arrays[f"{tag}_stepped_{k}"] = v
                arrays[f"{tag}_stepped_energies"] = np.array(s.energies())
                d, _ = to_device(nb, ic)
                s.compute_forces(d)
                arrays[f"{tag}_plugin_acc"] = acc_of(d)
                s.close()
        comm.close()
    np.savez(out, **arrays)
    print(f"{len(arrays)} arrays -> {out}")


def time_steps():
    np, nb, Comm, ShardedDirect = _imports()
    comm = Comm.init_all(8, [0] * 8)
    for n, warmup, steps in TIMED:
        s = ShardedDirect(comm, n, 1.0, 1e-3)
        s.set_state(nb.ic.plummer(n, seed=42))
        s.forces()
        print(n, statistics.median(s.time_steps(1e-3, warmup, steps) for _ in range(3)), flush=True)
        s.close()
    comm.close()


def child(lib, *args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=dict(os.environ, NBODY_HIP_LIB=os.path.abspath(lib)),
                       capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        sys.exit(f"{lib} {' '.join(args)}: exit code {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    print(f"  ran {os.path.basename(os.path.dirname(os.path.abspath(lib)))} {args[0]}", flush=True)  # (progress)
    return r.stdout


def compare(lib_a, lib_b, rounds, out, names):
    import numpy as np
    lines, bad = [f"A = {names[0]}", f"B = {names[1]}"], 0
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for tag, lib in (("a", lib_a), ("b", lib_b)):
            files.append(os.path.join(tmp, tag + ".npz"))
            child(lib, "state", files[-1])
        a, b = np.load(files[0]), np.load(files[1])
        differ = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k])] + [k for k in b.files if k not in a.files]
        finite = all(np.all(np.isfinite(a[k])) for k in a.files)
        lines.append(f"state: {len(a.files)} arrays (W in {WORLDS}, n = {N_STATE}, equal and random masses, eps 0.01 and 0; after forces(), "
                     f"after 3 steps, energies, plugin form), all finite: {finite}; array_equal fails on {len(differ)}")
        lines += [f"  DIFFERS {k}" for k in differ]
        bad += len(differ) + (0 if finite else 1)
    ms = {"A": {}, "B": {}}
    for _ in range(rounds):
        for tag, lib in (("A", lib_a), ("B", lib_b)):
            for ln in child(lib, "time").splitlines():
                ms[tag].setdefault(int(ln.split()[0]), []).append(float(ln.split()[1]))
    for n, warmup, steps in TIMED:
        xa, xb = ms["A"][n], ms["B"][n]
        ok = statistics.median(xb) <= max(xa)
        bad += 0 if ok else 1
        lines.append(f"time_steps W = 8 virtual ranks, n = {n}, {steps} steps after {warmup}, ms per step, {rounds} alternating rounds of "
                     f"fresh processes (each the median of 3 calls):")
        lines.append(f"  A rounds {' '.join(f'{x:.4f}' for x in xa)}   median {statistics.median(xa):.4f}  spread [{min(xa):.4f}, {max(xa):.4f}]")
        lines.append(f"  B rounds {' '.join(f'{x:.4f}' for x in xb)}   median {statistics.median(xb):.4f}  "
                     f"{'within' if ok else 'ABOVE'} A's spread")
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("state").add_argument("out")
    sub.add_parser("time")
    c = sub.add_parser("compare")
    c.add_argument("lib_a")
    c.add_argument("lib_b")
    c.add_argument("--rounds", type=int, default=5)
    c.add_argument("--out", default=None)
    c.add_argument("--names", nargs=2, default=["the first library", "the second library"], help="what the record calls A and B")
    a = ap.parse_args()
    if a.cmd == "state":
        return state(a.out)
    if a.cmd == "time":
        return time_steps()
    return compare(a.lib_a, a.lib_b, a.rounds, a.out, a.names)


if __name__ == "__main__":
    sys.exit(main())
