#!/usr/bin/env python3
"""Writes tests/golden/hermite_ext_refs.npz again: the fp64 end states the accuracy checks of the extended state
precision are measured against (tests/hermite_ext_ref.compute_references; numpy only, about a minute).

    python tests/golden/make_hermite_ext_refs.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hermite_ext_ref as xr  # noqa: E402

if __name__ == "__main__":
    refs = xr.compute_references()
    np.savez(xr.GOLDEN, **refs)
    print({k: v.tolist() for k, v in refs.items()})
