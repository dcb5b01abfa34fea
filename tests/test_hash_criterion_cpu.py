"""The parity criterion of the spatial-hash comparisons (tests/gpu_util.py assert_hash_parity) tested
on the CPU: the oracle's pair loop summed the way the kernels sum (oracle_spatial_hash_forces_emulated), once with correct
arithmetic and once with the defects a kernel could plausibly acquire -- terms a few ulps off (a worse rsqrt, a lost
refinement), a systematic bias, partial sums never folded into fp64.  Correct arithmetic must pass both tiers; every
defect passes the single ceiling C = 83 of round 4 (which is why tier 2 exists) and must fail tier 2."""
import numpy as np
import pytest

import nbody_amd
from gpu_util import (C_SUM, TAIL_MIN, TIER2, U, assert_hash_parity, hash_c, hash_stats, rel_err,
                      tier2_failures)

EPS2 = float(np.float32(0.01) ** 2)
ROUND4_C = 83          # the one tier-1 constant every comparison used in round 4, whatever the kernel

# uniform: BASELINE config 5's density (16 bodies per unit volume), cutoff = cell = 1;
# dense: 100,000 bodies in a +-4 box (~195 per unit volume), cutoff 2 > cell 1 (thousands of terms per body)
REGIMES = {"uniform": (262144, 0.5 * (262144 / 16.0) ** (1 / 3), 1.0), "dense": (100000, 4.0, 2.0)}
_cache = {}


def _regime(oracle, name):
    if name not in _cache:
        n, half, cutoff = REGIMES[name]
        ic = nbody_amd.ic.uniform_box(n, seed=7, lo=-half, hi=half)
        ref, _, kappa = oracle.spatial_hash_forces_cond(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], 1.0, EPS2,
                                                        1.0, cutoff)
        _cache[name] = (ic, cutoff, ref, kappa, np.linalg.norm(ref, axis=1) > 0)
    return _cache[name]


def _emulate(oracle, name, run, ulps=0, bias=False):
    """per-body error and kappa of the emulated kernel against the oracle, over the bodies with a non-zero force"""
    ic, cutoff, ref, kappa, nz = _regime(oracle, name)
    a = oracle.spatial_hash_forces_emulated(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], 1.0, EPS2, 1.0, cutoff,
                                            run, ulps, bias)
    assert np.all(a[~nz] == 0)
    return rel_err(a[nz], ref[nz]), kappa[nz]


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_emulation_is_the_oracle_pair_set(oracle, name):
    """run 1 folds every term into fp64 as it comes: the oracle itself, bit for bit (same pairs, same terms, same order)"""
    ic, cutoff, ref, _, nz = _regime(oracle, name)
    a = oracle.spatial_hash_forces_emulated(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], 1.0, EPS2, 1.0, cutoff,
                                            1, 0, False)
    assert np.array_equal(a, ref)
    assert nz.mean() > 0.99 and ic["pos_x"].size >= TAIL_MIN    # both regimes are large enough for the tail statistics


# 3.1 correct arithmetic passes both tiers: partial sums of 32 (kernels 2-4, 7) and 64 (kernels 1, 6, 10) entries,
# exact terms and terms within +-1 ulp of inv (what v_rsq_f32 is allowed) -- the constants are not tighter than that
@pytest.mark.parametrize("name", sorted(REGIMES))
@pytest.mark.parametrize("run,kernel", [(32, 2), (64, 1)])
@pytest.mark.parametrize("ulps", [0, 1])
def test_correct_arithmetic_passes_both_tiers(oracle, name, run, kernel, ulps):
    e, k = _emulate(oracle, name, run, ulps)
    st = assert_hash_parity(f"emulated {name} run {run} +-{ulps} ulp", e, k, "oracle", kernel)
    assert st["n"] >= TAIL_MIN          # the tails were asserted too


# 3.2 the defects: each passes round 4's gate (asserted: the gap this tier closes) and fails tier 2
DEFECTS = [("uniform", 64, 8, False), ("uniform", 64, 16, False),     # +-8 / +-16 ulp per term, pseudo-random per pair
           ("uniform", 64, 4, True), ("uniform", 64, 16, True),       # +4 / +16 ulp on every term
           ("dense", 0, 0, False)]                                    # no fp64 fold: one fp32 sum of thousands of terms


@pytest.mark.parametrize("name,run,ulps,bias", DEFECTS)
def test_degraded_kernel_fails_tier_2(oracle, name, run, ulps, bias):
    e, k = _emulate(oracle, name, run, ulps, bias)
    assert np.all(e <= np.maximum(1e-5, ROUND4_C * U * k)), "round 4's gate was expected to let this defect through"
    st = hash_stats(e, k)
    bad = tier2_failures(st, "oracle")
    print(f"emulated {name} run {run} ulps {ulps} bias {bias}: median {st['median']:.3e} p99.99 {st['p9999']:.3e} "
          f"above 1e-5 {st['over']} margin {st['margin']:.2f} -> {bad}")
    assert bad, st
    with pytest.raises(AssertionError, match="tier 2"):
        assert_hash_parity(f"emulated defect {name}", e, k, "oracle", 0)


# 3.3 the per-kernel table of tier 1: C_SUM counts the roundings a term passes through in its fp32 run, its own entry
# into the run included, so no kernel may keep a run longer than 64 entries (one more rounding than the 63 additions
# round 4 counted: the automatic choice's ceilings are 84 / 73 / 128)
def test_per_kernel_table():
    from test_spatial_hash_gpu import KERNELS
    for kern in set(KERNELS) | {6, 0}:
        assert isinstance(C_SUM[kern], int) and 0 < C_SUM[kern] <= 64, kern
    assert C_SUM[0] == max(C_SUM[k] for k in (1, 3, 6, 8, 9))       # what the automatic choice can pick
    assert hash_c("oracle", 0) == ROUND4_C + 1 and hash_c("gold", 0) == 73 and hash_c("gpu", 0) == 128
    for kern in C_SUM:
        assert hash_c("oracle", kern) <= ROUND4_C + 1 and hash_c("gpu", kern) == 2 * C_SUM[kern]
    for kind in ("oracle", "gold", "gpu"):
        assert set(TIER2[kind]) == {"median", "p9999", "frac", "margin"}
        assert all(0 < v < np.inf for v in TIER2[kind].values()), kind
