"""The Hermite integrator with individual block time steps against the shared-step one, and the crossover between the
narrow and the wide form of its force-and-jerk kernel (Plummer sphere, eps = 0.01, eta = 0.02, eta_start = 0.01,
max_level = 16, macro step 1/16).

  macro      nbody_hip_hermite_block_advance: wall-clock ms per macro step (the call blocks: it reads {t, n_active} back
             once per block step), median of 3 after a warm-up macro step; the block steps and body steps of the timed
             macro steps from nbody_hip_hermite_block_info; pairs/s = body steps x N / time
  shared     nbody_hip_hermite_step with dt = the smallest step a body took in that macro step, dt_max 2^-kmax: ms per step
             (HIP events around 3 steps), times the 2^kmax steps that cover the macro step
  crossover  ONE block step with a forced active set (set_levels: n_active scattered bodies on level 1, the others on
             level 0), the narrow and the wide form forced in turn through nbody_hip_hermite_block_tuning: wall-clock
             microseconds of the step call plus the stream synchronisation after it, median of 9 alternating readings.
             Both forms share the schedule, predict and finalize launches and the host read, so their difference is the
             difference of the two kernels.

Every size runs in a child process of its own under a time limit; the first non-zero status ends the run.  The compiler's
resource report of the new kernels is appended (hipcc -Rpass-analysis=kernel-resource-usage: no GPU needed).
usage: python tools/hermite_block_time.py [--out profiles/r10_hermite_block.txt] [--sizes 4096,65536] [--no-macro]

  --resident [--parent-tree DIR]   the resident scheduler instead: ms per macro step of
             (a) the host form with its automatic kernel choice -- of the built tree DIR when given (the parent commit),
                 else of this tree,
             (b) this tree's host form held to the narrow kernel, and
             (c) this tree's resident form,
             at N = 64, 256, 1024, 2048, 4096 (--sizes).  One reading is one advance(1) call plus the stream
             synchronisation after it.  Per size, ROUNDS rounds of the child processes (a), (c) ALTERNATELY (then (b)),
             each child under its own time limit: one warm-up macro step, then READINGS timed ones; the median, min and
             max of the ROUNDS x READINGS readings of each form, and the block steps and body steps of a macro step.
             Default --out profiles/r12_hermite_block_resident.txt.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 65536)
G, EPS, DT_MAX, ETA, ETA_START, L = 1.0, 0.01, 1.0 / 16, 0.02, 0.01, 16
ACTIVE = (1, 4, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 2048)


def child(n, macro):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    from gpu_util import to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    ctx = nb.default_context(0)
    lib = ctx._lib
    ic = nb.ic.plummer(n, seed=42)
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(G)
    fc.setSofteningParameter(EPS)
    res = {"n": n, "device": torch.cuda.get_device_name(0)}

    # -- crossover: one forced block step, both forms ---------------------------------------------------------------
    d, _ = to_device(nb, ic)
    blk = nb.BlockHermiteIntegrator()
    blk.setParameters(ETA, ETA_START, 6)
    rng = np.random.default_rng(1)
    sweep = {}
    for k in (a for a in ACTIVE if a < n):
        levels = np.zeros(n, np.int32)
        levels[rng.choice(n, k, replace=False)] = 1
        t = {"narrow": [], "wide": []}
        for rep in range(10):
            for form, below in (("narrow", 1 << 30), ("wide", 1)):
                blk.setTuning(below)
                blk.prime(d, fc, DT_MAX)
                blk.setLevels(levels)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                blk.block_step(d, fc, DT_MAX, 1)
                torch.cuda.synchronize()
                if rep:  # (the first reading of each form grows the workspaces)
                    t[form].append((time.perf_counter() - t0) * 1e6)
        sweep[k] = {f: [float(np.median(v)), float(min(v)), float(max(v))] for f, v in t.items()}
    res["sweep"] = sweep
    blk.setTuning(0)
    blk.prime(d, fc, DT_MAX)
    res["narrow_below"] = blk.info()["narrow_below"]
    blk.close()

    # -- macro steps against the shared step ------------------------------------------------------------------------
    if macro:
        d, _ = to_device(nb, ic)
        blk = nb.BlockHermiteIntegrator()
        blk.setParameters(ETA, ETA_START, L)
        blk.advance(d, fc, DT_MAX, 1)  # warm-up: priming, the workspaces, the levels settle
        ms, steps, bodies, levels = [], [], [], []
        for _ in range(3):
            before = blk.info()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blk.advance(d, fc, DT_MAX, 1)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            after = blk.info()
            steps.append(after["block_steps"] - before["block_steps"])
            bodies.append(after["body_steps"] - before["body_steps"])
            levels.append([a - b for a, b in zip(after["level_steps"], before["level_steps"])])
        info = blk.info()
        order = int(np.argsort(ms)[1])  # the macro step with the median time: its own counts
        kmax = max(k for k, v in enumerate(levels[order]) if v)
        res.update(macro_ms=[ms[order], min(ms), max(ms)], block_steps=steps[order], body_steps=bodies[order], kmax=kmax,
                   level_steps=levels[order], floor_hits=info["floor_hits"], narrow=info["narrow_launches"],
                   wide=info["wide_launches"])
        blk.close()
        d, _ = to_device(nb, ic)
        s = d.struct()
        h = C.c_void_p()
        nb._lib.check(lib.nbody_hip_hermite_create(ctx.handle, n, C.byref(h)))
        dt = DT_MAX / 2 ** kmax
        nb._lib.check(lib.nbody_hip_hermite_step(h, C.byref(s), G, EPS, dt, 1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        nb._lib.check(lib.nbody_hip_hermite_step(h, C.byref(s), G, EPS, dt, 3))
        e1.record()
        e1.synchronize()
        res["shared_step_ms"] = e0.elapsed_time(e1) / 3
        lib.nbody_hip_hermite_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


RES_SIZES = (64, 256, 1024, 2048, 4096)
ROUNDS, READINGS = 2, 5


def resident_child(n, form, tree):
    """one form at one size: RESULT {"ms": [...], "block_steps": [...], "body_steps": [...]} of READINGS macro steps"""
    import torch
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    from gpu_util import to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    ic = nb.ic.plummer(n, seed=42)
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(G)
    fc.setSofteningParameter(EPS)
    d, _ = to_device(nb, ic)
    blk = nb.BlockHermiteIntegrator()
    blk.setParameters(ETA, ETA_START, L)
    if form == "narrow":
        blk.setTuning(1 << 30)
    elif form == "resident":
        blk.setScheduling("resident")
    blk.advance(d, fc, DT_MAX, 1)  # warm-up: priming, the workspaces, the levels settle
    ms, steps, bodies = [], [], []
    for _ in range(READINGS):
        before = blk.info()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blk.advance(d, fc, DT_MAX, 1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        after = blk.info()
        steps.append(after["block_steps"] - before["block_steps"])
        bodies.append(after["body_steps"] - before["body_steps"])
    info = blk.info()
    print("RESULT " + json.dumps({"ms": ms, "block_steps": steps, "body_steps": bodies, "narrow": info["narrow_launches"],
                                  "wide": info["wide_launches"], "device": torch.cuda.get_device_name(0),
                                  "lib": os.path.relpath(nb._lib.LIB_PATH, tree)}), flush=True)


def resident_main(a):
    import statistics
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    forms = (("a", "host", parent), ("c", "resident", ROOT), ("b", "narrow", ROOT))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def run(n, form, tree):
        cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--case", str(n), "--form", form,
               "--tree", tree]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"N = {n}, {form}: status {r.returncode}; stopping")
            sys.exit(r.returncode)
        return json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))

    sizes = [int(v) for v in a.sizes.split(",")] if a.sizes else list(RES_SIZES)
    table = []
    for n in sizes:
        got = {k: [] for k, _, _ in forms}
        for rnd in range(ROUNDS):
            for key, form, tree in forms[:2]:  # (a) and (c) alternately
                got[key].append(run(n, form, tree))
        got["b"].append(run(n, "narrow", ROOT))
        if not lines:
            say(f"tools/hermite_block_time.py --resident on {got['a'][0]['device']}: Plummer sphere, eps = {EPS}, eta = {ETA}, "
                f"eta_start = {ETA_START}, max_level = {L}, dt_max = 1/{round(1 / DT_MAX)}; ms per macro step (one advance(1) "
                f"call + synchronisation), median (min, max) of {ROUNDS} x {READINGS} readings, (a) and (c) in alternating "
                f"child processes, (b) {READINGS} readings")
            say(f"  (a) host form, automatic kernel choice: {got['a'][0]['lib']} of "
                f"{'the tree given with --parent-tree' if a.parent_tree else 'this tree'}")
            say(f"  (b) host form held to the narrow kernel, (c) resident: {got['c'][0]['lib']} of this tree")
        row = {}
        for key in ("a", "b", "c"):
            ms = [v for r in got[key] for v in r["ms"]]
            row[key] = (statistics.median(ms), min(ms), max(ms))
        bs = statistics.median([v for r in got["c"] for v in r["block_steps"]])
        bd = statistics.median([v for r in got["c"] for v in r["body_steps"]])
        spread = row["a"][2] - row["a"][1]
        win = row["a"][0] - row["c"][0]
        table.append((n, row, win > spread))
        say(f"N = {n:5d}  (a) {row['a'][0]:8.3f} ({row['a'][1]:.3f}, {row['a'][2]:.3f})   (b) {row['b'][0]:8.3f} "
            f"({row['b'][1]:.3f}, {row['b'][2]:.3f})   (c) {row['c'][0]:8.3f} ({row['c'][1]:.3f}, {row['c'][2]:.3f})   "
            f"(a) / (c) = {row['a'][0] / row['c'][0]:6.2f}   {bs:.0f} block steps, {bd:.0f} body steps per macro step, "
            f"{row['c'][0] * 1e3 / bs:.1f} us per resident block step, {row['a'][0] * 1e3 / bs:.1f} us per host block step; "
            f"(a) - (c) = {win:+.3f} ms against a spread of (a) of {spread:.3f} ms: "
            f"{'(c) wins' if win > spread else '(c) does not win'}")
    wins = [n for n, _, w in table if w]
    say(f"crossover of the automatic scheduling: the largest measured N at which (c) beats (a) by more than the spread of "
        f"(a)'s repeats is {max(wins) if wins else 'none'}")
    say("compiler resource report, csrc/hermite_block.hip (gfx950):")
    for line in resources():
        say(line)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


def resources():
    src = os.path.join(ROOT, "n-body_amd", "csrc", "hermite_block.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "--cuda-device-only",
           "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = {"name": re.sub(r"\(.*", "", name).replace("nbh::", "").replace("void ", "")}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[\w/]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return [f"  {r['name']:48s} vgpr {r.get('VGPRs', 0):3d} agpr {r.get('AGPRs', 0):3d} sgpr {r.get('TotalSGPRs', 0):3d} "
            f"scratch {r.get('ScratchSize', 0):3d} lds {r.get('LDS Size', 0):6d} occupancy {r.get('Occupancy', 0)}" for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--resident", action="store_true", help="the resident scheduler against the host form")
    ap.add_argument("--parent-tree", default=None, help="--resident: a built tree whose host form is form (a)")
    ap.add_argument("--form", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--no-macro", action="store_true", help="the crossover sweep only")
    ap.add_argument("--case", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case and a.form:
        return resident_child(a.case, a.form, a.tree)
    if a.resident:
        a.out = a.out or os.path.join(ROOT, "profiles", "r12_hermite_block_resident.txt")
        return resident_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "r10_hermite_block.txt")
    a.sizes = a.sizes or ",".join(str(n) for n in SIZES)
    if a.case:
        return child(a.case, not a.no_macro)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for n in (int(v) for v in a.sizes.split(",")):
        # 15 active-set sizes x 20 single steps, then 4 macro steps of at most a few thousand block steps each
        cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--case", str(n)]
        r = subprocess.run(cmd + (["--no-macro"] if a.no_macro else []), capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"N = {n}: status {r.returncode}; stopping")
            return r.returncode
        res = json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))
        if not lines:
            say(f"tools/hermite_block_time.py on {res['device']}: Plummer sphere, eps = {EPS}, eta = {ETA}, eta_start = "
                f"{ETA_START}, dt_max = 1/{round(1 / DT_MAX)}")
        say(f"N = {n}")
        if "macro_ms" in res:
            t = res["macro_ms"]
            pairs = res["body_steps"] * float(n)
            shared_steps = 2 ** res["kmax"]
            shared = res["shared_step_ms"] * shared_steps
            say(f"  block steps, max_level {L}: {t[0]:10.3f} ms per macro step (min {t[1]:.3f}, max {t[2]:.3f}); "
                f"{res['block_steps']} block steps, {res['body_steps']} body steps, {pairs / t[0] / 1e9:.4f}e12 pairs/s; "
                f"narrow {res['narrow']} / wide {res['wide']} launches and {res['floor_hits']} floor hits in the four macro steps "
                "since priming")
            say("  body steps by level in that macro step: " +
                ", ".join(f"{k}: {v}" for k, v in enumerate(res["level_steps"]) if v))
            say(f"  shared step at the smallest step taken, dt_max / {shared_steps}: {res['shared_step_ms']:.3f} ms per step "
                f"x {shared_steps} = {shared:10.3f} ms per macro step, {shared_steps * n} body steps  "
                f"=> block / shared = {t[0] / shared:.3f} in time, {res['body_steps'] / (shared_steps * n):.4f} in body steps")
        say(f"  one forced block step, microseconds of the call + synchronisation, median of 9 (min, max); automatic "
            f"crossover in this build: narrow below {res['narrow_below']}")
        for k, row in res["sweep"].items():
            nw, wd = row["narrow"], row["wide"]
            say(f"    n_active {int(k):5d}   narrow {nw[0]:8.1f} ({nw[1]:.1f}, {nw[2]:.1f})   wide {wd[0]:8.1f} "
                f"({wd[1]:.1f}, {wd[2]:.1f})   narrow - wide {nw[0] - wd[0]:+8.1f}")
    say("compiler resource report, csrc/hermite_block.hip (gfx950):")
    for line in resources():
        say(line)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
