#!/usr/bin/env python3
"""Bit parity of two builds of libnbody_hip.so on the Barnes-Hut host state machine (a driver, not a test).

    python tools/tree_parity.py OTHER_LIB [--sizes 131072 6000] [--keep DIR]

Runs the sequence of tests/tree_sequence.py -- every walk, range walk, potential and visit total of one reused tree, and
after every build stats(), idLayout(), copyNodesToHost(), copyMomentsToHost() and a field call at 1,000 points -- once
against OTHER_LIB (selected with NBODY_HIP_LIB) and once against this tree's library, each in a fresh process under its
own timeout, and compares every recorded array byte for byte.  Prints the number of arrays compared; exit code 1 when
one differs or is missing on a side.

    python tools/tree_parity.py --record OUT.npz [--sizes ...]     (what the two child processes run)
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def record(out, sizes):
    import numpy as np
    import torch
    import nbody_amd as nb
    import tree_sequence as ts
    from gpu_util import to_device
    ctx = nb.default_context(0)
    arrays = {}
    for n in sizes:
        ic = nb.ic.two_galaxies(n, seed=31)
        d, _ = to_device(nb, ic)
        rng = np.random.default_rng(5)
        pts = torch.from_numpy((rng.random((1000, 3)) * 40.0 - 20.0).astype(np.float32)).cuda()
        for k, (label, s, kind, got) in enumerate(ts.sequence(nb, ctx, d, n, inspect=pts)):
            for name, a in got.items():
                arrays[f"n{n} | {k:02d} {label} | {name}"] = np.asarray(a)
    np.savez(out, **arrays)
    print(f"recorded {len(arrays)} arrays with {nb._lib.LIB_PATH}", flush=True)


def compare(path_a, path_b):
    import numpy as np
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("on one side only:", k)
    equal = 0
    for k in a.files:
        if k not in b.files:
            continue
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        equal += same
        if not same:
            bad.append(k)
            print("DIFFERS:", k)
    nbytes = sum(a[k].nbytes for k in a.files)
    print(f"{len(a.files)} arrays ({nbytes} bytes) compared, {equal} bit-equal, {len(bad)} different or missing")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other_lib", nargs="?")
    ap.add_argument("--record", metavar="OUT.npz")
    ap.add_argument("--sizes", type=int, nargs="*", default=[131072, 6000])
    ap.add_argument("--keep", metavar="DIR", help="keep the two recordings here")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    a = ap.parse_args()
    if a.record:
        return record(a.record, a.sizes)
    if not a.other_lib:
        ap.error("the other library, or --record")
    out_dir = a.keep or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for tag, lib in (("other", os.path.abspath(a.other_lib)), ("this", None)):
        env = dict(os.environ)
        env.pop("NBODY_HIP_LIB", None)
        if lib:
            env["NBODY_HIP_LIB"] = lib
        paths.append(os.path.join(out_dir, f"tree_parity_{tag}.npz"))
        cmd = [sys.executable, os.path.abspath(__file__), "--record", paths[-1], "--sizes"] + [str(n) for n in a.sizes]
        r = subprocess.run(cmd, env=env, timeout=a.timeout)
        if r.returncode != 0:  # (nothing more is started on the device after a failed run)
            print(f"the {tag} run ended with status {r.returncode}")
            return 2
    return compare(*paths)


if __name__ == "__main__":
    sys.exit(main())
