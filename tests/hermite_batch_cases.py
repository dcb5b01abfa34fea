"""The small systems the ensemble tests (tests/test_hermite_batch_*.py) and tools/hermite_batch_time.py share.  numpy only."""
import numpy as np

import hermite_ref as hr

# the binary-with-a-perturber ensemble: hermite_ref.binary(e = 0.9) plus one third body per system
TRIPLE = dict(G=1.7, eps=1e-4, dt_max=1.0 / 16, max_level=10, seed=2024, systems=300)


def triple(rng):
    """hermite_ref.binary(e = 0.9) and a third body drawn from rng: mass in [0.01, 0.5], at a distance in [0.3, 3] from
    one of the two stars (which one, and the direction, drawn too), with up to the local circular speed in a drawn
    direction -- so its level, and with it the schedule, differs from system to system.  -> ic dict (fp32)"""
    pos, vel, m = hr.binary(e=0.9)
    star = int(rng.integers(0, 2))
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    r = rng.uniform(0.3, 3.0)
    speed = rng.uniform(0.0, 1.0) * np.sqrt(0.5 / r)
    p3 = pos[star].astype(np.float64) + r * u
    v3 = vel[star].astype(np.float64) + speed * w
    pos = np.concatenate([pos, p3[None, :].astype(np.float32)])
    vel = np.concatenate([vel, v3[None, :].astype(np.float32)])
    m = np.concatenate([m, np.array([rng.uniform(0.01, 0.5)], np.float32)])
    return ic_of(pos, vel, m)


def triples(count, seed=TRIPLE["seed"]):
    rng = np.random.default_rng(seed)
    return [triple(rng) for _ in range(count)]


def ic_of(pos, vel, m):
    return dict(pos_x=pos[:, 0].copy(), pos_y=pos[:, 1].copy(), pos_z=pos[:, 2].copy(), vel_x=vel[:, 0].copy(),
                vel_y=vel[:, 1].copy(), vel_z=vel[:, 2].copy(), mass=np.asarray(m, np.float32).copy())


def arrays_of(ic):
    """-> pos [n, 3], vel [n, 3], m"""
    return (np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1), np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1),
            ic["mass"])
