#!/usr/bin/env python3
"""A/B of the Barnes-Hut step (or, with --workload hash / direct, the spatial-hash / Direct N^2 step) between a parent
checkout and this tree, where the HOST path shows: bench.py --workload bh / hash / direct at small (launch-bound) and large
body counts, the two trees alternating, every run a fresh process under its own timeout.

    python tools/bh_host_ab.py PARENT_TREE [--workload {bh,hash,direct}] [--bodies 4096 16384 98304 1048576] [--rounds 5]
                               [--out profiles/NAME.txt]

PARENT_TREE is a built checkout of the parent commit (its own bench.py, package and library).  Prints every run's
ms/step, then per body count both medians and the parent's own spread (min .. max of its rounds); exit code 1 when this
tree's median lies above the parent's slowest round at some body count, 2 when a run failed (nothing is started after it).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree, workload, n, steps, warmup, timeout):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--workload", workload, "--bodies", str(n), "--steps", str(steps),
           "--warmup", str(warmup), "--no-cpu-baseline", "--no-extra", "--no-clock"]
    env = dict(os.environ)
    env.pop("NBODY_HIP_LIB", None)
    r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        return None
    return float(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--workload", choices=["bh", "hash", "direct"], default="bh")
    ap.add_argument("--bodies", type=int, nargs="*", default=[4096, 16384, 98304, 1048576])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="0: 2000 below 500,000 bodies (a window of a few tenths of a second), 300 above")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    trees = (("parent", os.path.abspath(a.parent)), ("this", ROOT))
    lines = [f"bench.py --workload {a.workload} --steps {a.steps or '2000 / 300'} --warmup {a.warmup}, ms/step; parent and this tree alternate, "
             f"{a.rounds} rounds, one fresh process per run"]
    ms = {(tag, n): [] for tag, _ in trees for n in a.bodies}
    for n in a.bodies:
        for k in range(a.rounds):
            for tag, tree in trees:
                v = bench(tree, a.workload, n, a.steps or (2000 if n < 500000 else 300), a.warmup, a.timeout)
                if v is None:
                    print(f"N {n} round {k} {tag}: the run failed", flush=True)
                    return 2
                ms[(tag, n)].append(v)
                lines.append(f"N {n:8d} round {k} {tag:6s} {v:.4f}")
                print(lines[-1], flush=True)
    worse = False
    for n in a.bodies:
        p, t = ms[("parent", n)], ms[("this", n)]
        mp, mt = statistics.median(p), statistics.median(t)
        inside = mt <= max(p)
        worse = worse or not inside
        lines.append(f"N {n:8d} median parent {mp:.4f} (rounds {min(p):.4f} .. {max(p):.4f}), this {mt:.4f} "
                     f"(rounds {min(t):.4f} .. {max(t):.4f}), this / parent {mt / mp:.4f}: "
                     f"{'within' if inside else 'ABOVE'} the parent's spread")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
