#!/usr/bin/env python3
"""Writes tests/golden/hermite_batch_hierarchy_states.npz again (needs an MI355X; a few seconds): the states the engine
reaches in the small running cases of tests/hermite_batch_hierarchy_ref.py -- X and V (hi + lo as fp64, getExtendedState)
after every macro step of the walk (the fly-by and the 2+2 encounter as one plain ensemble, ten macro steps of 1/8) and of
the eight fly-bys (one plain ensemble, nine macro steps).  Data only: walk_X, walk_V [10, 7, 3], walk_m [7]; fly_X, fly_V
[9, 24, 3], fly_m [24].  tests/test_hermite_batch_hierarchy_cpu.py holds the restatement to its own bound against exact
arithmetic on them and asserts every decision clear.  The snapshot cases are examined at their initial states, which
need no recording.

    python tests/golden/make_hermite_batch_hierarchy_states.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbody_amd as nb  # noqa: E402
import hermite_batch_hierarchy_ref as href  # noqa: E402
import hermite_batch_outcomes_ref as oref  # noqa: E402
from gpu_util import to_device  # noqa: E402


def walk(ics, dt, macros):
    """(X [macros, n, 3], V, m) of the plain ensemble of `ics` after each of `macros` macro steps"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, href.FLY["L"])
    ens.setStatePrecision(href.FLY["precision"])
    ens.setLayout(offsets)
    calc = nb.DirectForceCalculator()
    calc.setGravitationalConstant(href.FLY["G"])
    calc.setSofteningParameter(href.FLY["eps"])
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
    out["walk_X"], out["walk_V"], out["walk_m"] = walk([oref.flyby_ic(), href.two_plus_two_ic()], href.WALK["dt"], href.WALK["macros"])
    ics = [oref.flyby_ic() for _ in href.FLY_DT]
    out["fly_X"], out["fly_V"], out["fly_m"] = walk(ics, np.array(href.FLY_DT, np.float32), href.FLY["macros"])
    path = sys.argv[1] if len(sys.argv) > 1 else href.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
