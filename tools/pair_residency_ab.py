#!/usr/bin/env python3
"""Atomic two-set (shard pair) Direct kernel at 16 bodies per lane: tuning variant 4 (every fp64 I-side sum in LDS, one
workgroup per CU) alternated with the default (12 bodies' sums in LDS, 4 in registers: two workgroups per CU), four rounds
of 40 launches per arm at three shard sizes, equal and general masses.   Usage: python tools/pair_residency_ab.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbody_amd as nb  # noqa: E402
from gpu_util import packed  # noqa: E402

torch.cuda.set_device(0)
ctx = nb.default_context(0)
ctx.deterministic(0)
for S in (65536, 131072, 262144):
    p = packed(nb.ic.plummer(2 * S, seed=42))
    pg = p.clone()
    pg[:, 3] *= torch.from_numpy((0.75 + 0.5 * np.random.default_rng(7).random(2 * S)).astype(np.float32)).cuda()
    for name, q in (("equal", p), ("general", pg)):
        a, b = q[:S].contiguous(), q[S:].contiguous()
        acc_a, acc_b = torch.zeros_like(a), torch.zeros_like(b)
        res = {4: [], -1: []}
        for rnd in range(4):
            for variant in (4, -1):
                ctx.tuning(variant, 16, 0)
                nb.direct_forces_pair_packed(ctx, a, b, 1.0, 1e-6, acc_a, acc_b)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(40):
                    nb.direct_forces_pair_packed(ctx, a, b, 1.0, 1e-6, acc_a, acc_b)
                e1.record()
                e1.synchronize()
                res[variant].append(e0.elapsed_time(e1) / 40)
        f = lambda v: " ".join(f"{x:.3f}" for x in v)
        print(f"pair {S} x {S} {name} masses, atomics, R=16: variant 4 [{f(res[4])}] ms   RL=12 [{f(res[-1])}] ms   "
              f"{'ranges apart' if max(res[-1]) < min(res[4]) else 'overlap or slower'}", flush=True)
ctx.tuning()
ctx.deterministic(1)
