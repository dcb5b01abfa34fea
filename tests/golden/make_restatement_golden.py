"""Writes restatement_twogalaxies2048.npz: the outputs of quadrupole_ref.Restatement (acc, phi and interaction counts of
every 16th body, theta 0.5, eps 0 and 0.05, orders 1 and 2) on the node table that tree_ref.RefTree makes of
twogalaxies2048_barnes_hut.npz.  Recorded before Restatement.walk learned its `detail` outputs;
test_walk_edges_cpu.py::test_restatement_reproduces_its_recorded_outputs holds every later version to it bit for bit.
Run from the repository root after build():  python tests/golden/make_restatement_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_bind  # noqa: E402
import quadrupole_ref as qr  # noqa: E402
import tree_ref  # noqa: E402
import walk_edge_ref as we  # noqa: E402


def main():
    z = np.load(os.path.join(HERE, "twogalaxies2048_barnes_hut.npz"))
    ic = {k: z[k] for k in ("pos_x", "pos_y", "pos_z", "mass")}
    ref = tree_ref.RefTree(oracle_bind.load(), ic, 20, 1)
    r = qr.Restatement(we.node_table(ref), ref.order, we.positions(ic), ic["mass"])
    targets = np.arange(0, 2048, 16)
    out = {"targets": targets}
    for eps in (0.0, 0.05):
        for order in (1, 2):
            out[f"acc_o{order}_eps{eps}"], out[f"phi_o{order}_eps{eps}"] = r.walk(targets, 0.5, 1.0, eps, order)
        out[f"counts_eps{eps}"] = r.interaction_counts(targets, 0.5, eps)
    np.savez(os.path.join(HERE, "restatement_twogalaxies2048.npz"), **out)


if __name__ == "__main__":
    main()
