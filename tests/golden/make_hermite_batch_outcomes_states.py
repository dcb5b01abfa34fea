#!/usr/bin/env python3
"""Writes tests/golden/hermite_batch_outcomes_states.npz again (needs an MI355X; a few seconds): the states the engine
reaches in the cases of tests/hermite_batch_outcomes_ref.py -- X and V (hi + lo as fp64, getExtendedState) after every
macro step of each case run as a B = 1 ensemble, and of the eight fly-bys run as one ensemble.  Data only: per case k
the arrays c<k>_X, c<k>_V [macros, n, 3] and c<k>_m [n]; fly_X, fly_V [7, 24, 3] and fly_m [24].
tests/test_hermite_batch_outcomes_cpu.py holds the restatement to its derived bound against exact arithmetic on them and
asserts every decision clear; tests/test_hermite_batch_outcomes_gpu.py asserts that the engine still reaches them bit
for bit.

    python tests/golden/make_hermite_batch_outcomes_states.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbody_amd as nb  # noqa: E402
import hermite_batch_outcomes_ref as oref  # noqa: E402
from gpu_util import to_device  # noqa: E402


def walk(ics, c, dt, macros):
    """(X [macros, n, 3], V, m) of the ensemble of `ics` after each of `macros` macro steps"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, c["L"])
    ens.setStatePrecision(c["precision"])
    ens.setLayout(offsets)
    calc = nb.DirectForceCalculator()
    calc.setGravitationalConstant(c["G"])
    calc.setSofteningParameter(c["eps"])
    ens.prime(d, calc, dt)
    Xs, Vs = [], []
    for _ in range(macros):
        ens.advance(d, 1)
        X, V = ens.getExtendedState(d)
        Xs.append(np.array(X, np.float64))
        Vs.append(np.array(V, np.float64))
    m = d.mass.cpu().numpy().copy()
    ens.close()
    return np.stack(Xs), np.stack(Vs), m


if __name__ == "__main__":
    out = {}
    for k, (name, c) in enumerate(oref.cases(nb).items()):
        out[f"c{k}_X"], out[f"c{k}_V"], out[f"c{k}_m"] = walk([c["ic"]], c, c["dt"], c["macros"])
        print(k, name, out[f"c{k}_X"].shape)
    ics = [oref.flyby_ic() for _ in oref.FLY_DT]
    out["fly_X"], out["fly_V"], out["fly_m"] = walk(ics, oref.FLY, np.array(oref.FLY_DT, np.float32), oref.FLY["macros"])
    path = sys.argv[1] if len(sys.argv) > 1 else oref.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
