"""Direct force-and-jerk against the one-sided force kernel, and the whole Hermite step: ms per call at 4,096, 65,536,
262,144 and 1,048,576 bodies (Plummer sphere, eps = 0.01).

  force   the one-sided packed force kernel + finalize: nbody_hip_direct_tuning(variant = 1), timed with
          nbody_hip_time_direct_packed (HIP events, 3 launches per reading)
  jerk    nbody_hip_direct_acc_jerk: pack + direct_jerk_kernel + finalize (HIP events around 3 calls)
  step    nbody_hip_hermite_step: predict + direct_jerk_kernel + finalize with the corrector (HIP events around 3 steps)

Per size: one warm-up reading of each, then five rounds force / jerk / step ALTERNATING; the median of the five (min,
max) is reported, with the ratios jerk / force and step / force.  Every size runs in a child process of its own under a
time limit; the first non-zero status ends the run.  The compiler's resource report of the three new kernels is appended
(hipcc -Rpass-analysis=kernel-resource-usage: cross-compiles, no GPU needed).
--extended adds the extended state precision to the same alternating rounds:
  jerk_ext  nbody_hip_direct_acc_jerk_ext: pack + direct_jerk_kernel<.., EXT> + finalize
  step_ext  nbody_hip_hermite_step on a second handle in extended mode (its own copy of the bodies)
and reports jerk_ext / jerk and step_ext / step: the fp32 kernels of the same build are the yardstick.  32,767 against
32,768 bodies compares two targets per lane with four (the launch shape changes there, the pair count by 0.006 %).
usage: python tools/hermite_time.py [--out profiles/r07_hermite.txt] [--sizes 4096,65536] [--extended]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 65536, 262144, 1048576)
G, EPS = 1.0, 0.01


def child(n, extended=False):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nbody_amd as nb
    from gpu_util import packed, to_device

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    ctx = nb.default_context(0)
    lib = ctx._lib
    ic = nb.ic.plummer(n, seed=42)
    d, _ = to_device(nb, ic)
    posm = packed(ic)
    out4 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    acc = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    jerk = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    eps2 = float(np.float32(EPS) * np.float32(EPS))
    s = d.struct()
    h = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_create(ctx.handle, n, C.byref(h)))
    nb._lib.check(lib.nbody_hip_hermite_prime(h, C.byref(s), G, EPS))
    reps = 3

    def force():
        ctx.tuning(variant=1)
        try:
            return nb.time_direct_packed(ctx, posm, posm, G, eps2, reps, out4)
        finally:
            ctx.tuning()

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def eval_jerk():
        nb._lib.check(lib.nbody_hip_direct_acc_jerk(ctx.handle, C.byref(s), G, EPS, acc.data_ptr(), jerk.data_ptr()))

    def step():
        nb._lib.check(lib.nbody_hip_hermite_step(h, C.byref(s), G, EPS, 1e-4, 1))

    kinds = {"force": force, "jerk": lambda: events(eval_jerk), "step": lambda: events(step)}
    if extended:
        d2, _ = to_device(nb, ic)
        s2 = d2.struct()
        lo4 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        lo4[:, :3] = (torch.rand((n, 3), device="cuda") - 0.5) * 2.0 ** -25  # residuals of positions of order 1
        h2 = C.c_void_p()
        nb._lib.check(lib.nbody_hip_hermite_create(ctx.handle, n, C.byref(h2)))
        nb._lib.check(lib.nbody_hip_hermite_set_precision(h2, 1))
        nb._lib.check(lib.nbody_hip_hermite_prime(h2, C.byref(s2), G, EPS))

        def eval_jerk_ext():
            nb._lib.check(lib.nbody_hip_direct_acc_jerk_ext(ctx.handle, C.byref(s), lo4.data_ptr(), G, EPS, acc.data_ptr(),
                                                            jerk.data_ptr()))

        def step_ext():
            nb._lib.check(lib.nbody_hip_hermite_step(h2, C.byref(s2), G, EPS, 1e-4, 1))

        kinds["jerk_ext"] = lambda: events(eval_jerk_ext)
        kinds["step_ext"] = lambda: events(step_ext)
    for fn in kinds.values():  # warm-up: workspaces grow here
        fn()
    t = {k: [] for k in kinds}
    for _ in range(5):
        for k, fn in kinds.items():
            t[k].append(fn())
    torch.cuda.synchronize()
    lib.nbody_hip_hermite_destroy(h)
    if extended:
        lib.nbody_hip_hermite_destroy(h2)
    print("RESULT " + json.dumps({"n": n, "device": torch.cuda.get_device_name(0),
                                  **{k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in t.items()}}),
          flush=True)


def resources(name="hermite.hip"):
    src = os.path.join(ROOT, "n-body_amd", "csrc", name)
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
    return [f"  {r['name']:58s} vgpr {r.get('VGPRs', 0):3d} agpr {r.get('AGPRs', 0):3d} sgpr {r.get('TotalSGPRs', 0):3d} "
            f"scratch {r.get('ScratchSize', 0):3d} lds {r.get('LDS Size', 0):6d} occupancy {r.get('Occupancy', 0)}" for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_hermite.txt"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--extended", action="store_true", help="also time the extended state precision")
    ap.add_argument("--case", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.extended)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    fmt = lambda t: f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"  # noqa: E731
    for n in (int(v) for v in a.sizes.split(",")):
        # the largest size: (1 + 5) rounds x 3 readings x ~1.3 s; a minute of set-up at the outside
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--case", str(n)]
                           + (["--extended"] if a.extended else []), capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"N = {n}: status {r.returncode}; stopping")
            return r.returncode
        res = json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))
        if not lines:
            say(f"tools/hermite_time.py on {res['device']}: Plummer sphere, eps = {EPS}; ms per call, median of 5 "
                "alternating rounds (min, max) after a warm-up, 3 launches per reading, HIP events")
        pairs = float(n) * n
        say(f"N = {n}")
        say(f"  force (one-sided packed kernel, variant 1) {fmt(res['force'])}  {pairs / res['force'][0] / 1e9:7.3f}e12 pairs/s")
        say(f"  jerk  (nbody_hip_direct_acc_jerk)          {fmt(res['jerk'])}  {pairs / res['jerk'][0] / 1e9:7.3f}e12 pairs/s"
            f"  = {res['jerk'][0] / res['force'][0]:.3f} x force")
        say(f"  step  (nbody_hip_hermite_step)             {fmt(res['step'])}  {pairs / res['step'][0] / 1e9:7.3f}e12 pairs/s"
            f"  = {res['step'][0] / res['force'][0]:.3f} x force")
        if a.extended:
            say(f"  jerk_ext (nbody_hip_direct_acc_jerk_ext)   {fmt(res['jerk_ext'])}  {pairs / res['jerk_ext'][0] / 1e9:7.3f}e12 pairs/s"
                f"  = {res['jerk_ext'][0] / res['jerk'][0]:.3f} x jerk")
            say(f"  step_ext (hermite_step, extended)          {fmt(res['step_ext'])}  {pairs / res['step_ext'][0] / 1e9:7.3f}e12 pairs/s"
                f"  = {res['step_ext'][0] / res['step'][0]:.3f} x step")
    say("compiler resource report, csrc/hermite.hip (gfx950):")
    for line in resources():
        say(line)
    if a.extended:
        say("compiler resource report, csrc/hermite_block.hip (gfx950):")
        for line in resources("hermite_block.hip"):
            say(line)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
