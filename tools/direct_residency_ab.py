#!/usr/bin/env python3
"""Symmetric Direct N^2 kernel at N = 2^20, 16 bodies per lane: where the fp64 I-side sums live.  Alternates tuning
variant 4 (all 48 sums of a lane in LDS: one workgroup per CU, one wave per SIMD) with variant 3 (36 in LDS, 12 in
registers: two workgroups per CU), equal masses first, then general masses, each arm run for ~3 s with the engine
clock / package power (sysfs) sampled beside it: ms per launch, median engine clock, mean power and Mcycles per launch
-- what the second wave saves in cycles and what the power limit gives back in clock.  A last line times the automatic
choice for general masses (12 bodies per lane in deterministic mode) for reference.
Usage: python tools/direct_residency_ab.py [rounds [atomics]]   (atomics: the fp64-atomic form instead of the slots)"""
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbody_amd as nb  # noqa: E402
from gpu_util import packed  # noqa: E402
from bench import ClockSampler  # noqa: E402  (sysfs reader: a process that holds the GPU starts no rocm-smi child)

_clock = ClockSampler(0)


def smi():
    r = _clock.read() if _clock.src else None
    return {"sclk": r["sclk_mhz"], "power": r.get("power_w", 0.0)} if r else {}


def arm(ctx, p, label, variant, tpl, launches=20):
    ctx.tuning(variant, tpl, 0)
    nb.time_direct_packed(ctx, p, p, 1.0, 1e-6, 2)
    samples, stop = [], threading.Event()

    def run():
        while not stop.is_set():
            r = smi()
            if r.get("power", 0) > 600:
                samples.append(r)
            stop.wait(0.1)
    t = threading.Thread(target=run, daemon=True)
    t.start()
    ms = nb.time_direct_packed(ctx, p, p, 1.0, 1e-6, launches)
    stop.set()
    t.join()
    ctx.tuning()
    clk = sorted(s["sclk"] for s in samples) or [0]
    pw = [s["power"] for s in samples] or [0]
    med = clk[len(clk) // 2]
    print(f"{label}: {ms:7.2f} ms per launch, sclk median {med:.0f} MHz, power mean {sum(pw) / len(pw):.0f} W "
          f"({len(samples)} samples) -> {ms * med / 1e3:.1f} Mcycles per launch", flush=True)
    return ms


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    atomics = len(sys.argv) > 2 and sys.argv[2] == "atomics"
    torch.cuda.set_device(0)
    ctx = nb.default_context(0)
    ctx.deterministic(not atomics)
    n = 1 << 20
    p_eq = packed(nb.ic.plummer(n, seed=42))
    p_gen = p_eq.clone()
    p_gen[:, 3] *= torch.from_numpy((0.75 + 0.5 * np.random.default_rng(7).random(n)).astype(np.float32)).cuda()
    for name, p in (("equal masses", p_eq), ("general masses", p_gen)):
        print(f"{name}, N = {n}, 16 bodies per lane, {'fp64 atomics' if atomics else 'deterministic slots'}:")
        t = {4: [], 3: []}
        for _ in range(rounds):
            for variant, label in ((4, "variant 4, all sums in LDS, 1 workgroup/CU "), (3, "variant 3, 12 in LDS + 4 in VGPRs, 2 wg/CU")):
                t[variant].append(arm(ctx, p, label, variant, 16))
        lo4, hi3 = min(t[4]), max(t[3])
        print(f"  fastest variant 4 {lo4:.2f} ms, slowest variant 3 {hi3:.2f} ms: "
              f"{'ranges apart' if hi3 < lo4 else 'RANGES OVERLAP'}, medians {sorted(t[4])[len(t[4]) // 2]:.2f} -> "
              f"{sorted(t[3])[len(t[3]) // 2]:.2f} ms")
    arm(ctx, p_gen, "general masses, automatic choice           ", -1, 0)


if __name__ == "__main__":
    main()
