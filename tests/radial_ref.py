"""The radial profiles (include/nbody_hip_radial.h) restated in numpy: the per-member arithmetic in fp64 with separate
roundings, the radial order by np.lexsort on (position, bits(q)), the enclosed mass in the model's order and as a long
double cumulative sum, the three cut rules, the shell sums in the order of nbody_hip_group_props.h; the two lattice
recipes of the GPU tests; and the bounds of the general-data comparison.  No GPU, no package import: the CPU tests hold
this file against a plain-Python loop, the GPU tests hold the kernels against it."""
import math

import numpy as np

import group_props_ref as gp

S, C = gp.S, gp.C  # the two sizes of group_props_plan.h: a group / shell of at most S in turn, else chunks of C
MAX_CUTS = 16
MASS, NUMBER, RADIUS = 0, 1, 2
MODES = {"mass": MASS, "number": NUMBER, "radius": RADIUS}

GROUP_DTYPE = np.dtype([("mass", "<f8"), ("r_max", "<f8"), ("n", "<i4"), ("status", "<i4"), ("reserved", "<i4", (2,))])
SHELL_DTYPE = np.dtype([("radius", "<f8"), ("enclosed_mass", "<f8"), ("mass", "<f8"), ("m_vr", "<f8"), ("m_vr2", "<f8"),
                        ("m_vt2", "<f8"), ("count", "<i4"), ("enclosed_count", "<i4"), ("reserved", "<i4", (2,))])
assert GROUP_DTYPE.itemsize == 32 and SHELL_DTYPE.itemsize == 64
SUMS = ("mass", "m_vr", "m_vr2", "m_vt2")
POS, VEL = gp.POS, gp.VEL


# ---- the per-member arithmetic ---------------------------------------------------------------------------------------------
def member_terms(x, v, m, c, V):
    """x, v, c, V: lists of three fp64 arrays (member coordinates / the member's group's centre), m fp64.
    -> (r2, terms [4, T]); every operation one fp64 rounding, parenthesised as the model writes it"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = [x[a] - c[a] for a in range(3)]
        u = [v[a] - V[a] for a in range(3)]
        r2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
        s = ((u[0] * d[0]) + (u[1] * d[1])) + (u[2] * d[2])
        u2 = ((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2])
        r = np.sqrt(r2)
        vr = np.where(r2 > 0, s / np.where(r2 > 0, r, 1.0), 0.0)
        vr2 = vr * vr
        vt2 = u2 - vr2
        return r2, np.stack([m, m * vr, m * vr2, m * vt2])


def q_of(r2):
    """(float)r2: round to nearest, overflow gives +inf"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(r2, np.float64).astype(np.float32)


# ---- the orders of the sums ------------------------------------------------------------------------------------------------
def enclosed_model(m):
    """E(s) of one group in the model's order (n alone decides it): fp64 array [n]"""
    m = np.asarray(m, np.float64)
    n = m.size
    if n <= S:
        return np.cumsum(m)  # (np.cumsum adds in turn)
    nch = (n + C - 1) // C
    a = np.zeros(nch * C)
    a[:n] = m
    a = np.cumsum(a.reshape(nch, C // 4, 4), axis=2)
    P = a[:, :, 3].copy()
    o = 1
    while o < C // 4:
        P[:, o:] = P[:, :-o] + P[:, o:]  # (the right side is evaluated before the store: the values before the round)
        o *= 2
    W = a.copy()
    W[:, 1:, :] = P[:, :-1, None] + a[:, 1:, :]
    E = W.reshape(nch, C)
    if nch > 1:
        B = np.cumsum(P[:-1, -1])  # B_1 = C_0, B_k = B_(k-1) + C_(k-1)
        E[1:] = B[:, None] + E[1:]
    return E.reshape(-1)[:n].copy()


def _fold64(s):
    """s[..., 64] -> s[..., 0] after s_l += s_(l + 32), 16, 8, 4, 2, 1"""
    s = s.copy()
    off = 32
    while off:
        s[..., :off] = s[..., :off] + s[..., off:2 * off]
        off //= 2
    return s[..., 0]


def ordered_sum(t):
    """the sum of the fp64 terms t (positions 0 .. count - 1) in THE ORDER OF EVERY SUM of nbody_hip_group_props.h"""
    t = np.asarray(t, np.float64)
    n = t.size
    acc = 0.0
    if n <= S:
        for v in t:
            acc = acc + v
        return np.float64(acc)
    nch = (n + C - 1) // C
    a = np.zeros(nch * C)
    a[:n] = t
    a = a.reshape(nch, 4, 256)
    s = np.zeros((nch, 256))
    for j in range(4):
        s = s + a[:, j, :]
    runs = _fold64(s.reshape(nch, 4, 64))
    chunk = ((runs[:, 0] + runs[:, 1]) + runs[:, 2]) + runs[:, 3]
    rounds = (nch + 63) // 64
    cpad = np.zeros(rounds * 64)
    cpad[:nch] = chunk
    lanes = np.zeros(64)
    for r in range(rounds):
        lanes = lanes + cpad[64 * r:64 * r + 64]
    return np.float64(_fold64(lanes))


# ---- the cuts ----------------------------------------------------------------------------------------------------------------
def check_cuts(cuts, mode):
    """what the host refuses (radial_plan.h: radial_cuts_check): 0 legal, else 1 n_cuts, 2 mode, 3 range, 4 order"""
    cuts = [float(c) for c in cuts]
    if not 1 <= len(cuts) <= MAX_CUTS:
        return 1
    if mode not in (MASS, NUMBER, RADIUS):
        return 2
    for i, v in enumerate(cuts):
        if mode == RADIUS:
            if not v >= 0.0:
                return 3
        elif not 0.0 < v <= 1.0:
            return 3
        if i and not cuts[i - 1] < v:
            return 4
    return 0


def k_of(mode, cut, E, q):
    """K_c of one group from its E and q in rank order (before K is raised to K_(c-1))"""
    n = len(E)
    if mode == NUMBER:
        return min(n, max(1, int(math.ceil(np.float64(cut) * np.float64(n)))))
    if mode == MASS:
        T = np.float64(cut) * E[n - 1]
        hit = np.nonzero(E >= T)[0]
        return int(hit[0]) + 1 if hit.size else n
    return int((np.sqrt(q.astype(np.float64)) <= cut).sum())


# ---- the reference -----------------------------------------------------------------------------------------------------------
def reference(fields, offsets, members, centres, cuts, mode, vels=None, count=None):
    """-> dict: groups [G] GROUP_DTYPE, shells [G, n_cuts] SHELL_DTYPE, sorted_members [n_members] int32, sorted_q
    [n_members] float32 -- the model, to the bit -- and `state`: what wide() needs (the terms in rank order)."""
    mode = MODES.get(mode, mode)
    assert check_cuts(cuts, mode) == 0
    cuts = np.asarray(cuts, np.float64)
    count = int(fields["mass"].size if count is None else count)
    off = np.asarray(offsets, np.int64)
    G, nc = off.size - 1, cuts.size
    n_members = count if members is None else len(members)
    mem = np.arange(n_members, dtype=np.int64) if members is None else np.asarray(members, np.int64)
    centres = np.asarray(centres, np.float64).reshape(G, 3)
    vels = np.zeros((G, 3)) if vels is None else np.asarray(vels, np.float64).reshape(G, 3)
    groups, shells = np.zeros(G, GROUP_DTYPE), np.zeros((G, nc), SHELL_DTYPE)
    sm, sq = np.full(n_members, -1, np.int32), np.zeros(n_members, np.float32)
    out = dict(groups=groups, shells=shells, sorted_members=sm, sorted_q=sq, state={})
    ordered = G == 0 or (off[0] >= 0 and (off[:-1] <= off[1:]).all() and off[-1] <= n_members)
    if not ordered:
        groups["status"] = 1
        return out
    state = {}
    for g in range(G):
        o0, o1 = int(off[g]), int(off[g + 1])
        n = o1 - o0
        idx = mem[o0:o1]
        if n == 0 or ((idx < 0) | (idx >= count)).any():
            groups[g]["status"] = 1
            continue
        x = [fields[k][idx].astype(np.float64) for k in POS]
        v = [fields[k][idx].astype(np.float64) for k in VEL]
        m = fields["mass"][idx].astype(np.float64)
        r2, terms = member_terms(x, v, m, list(centres[g]), list(vels[g]))
        if np.isnan(r2).any():
            groups[g]["status"] = 2
            continue
        q = q_of(r2)
        order = np.lexsort((np.arange(n), q.view(np.uint32)))  # ascending by (bits(q), p)
        q, terms, idx = q[order], terms[:, order], idx[order]
        sm[o0:o1], sq[o0:o1] = idx, q
        E = enclosed_model(terms[0])
        groups[g] = (E[-1], np.sqrt(np.float64(q[-1])), n, 0, (0, 0))
        prev, Ks = 0, []
        for c in range(nc):
            K = max(k_of(mode, cuts[c], E, q), prev)
            row = shells[g, c]
            row["radius"] = cuts[c] if mode == RADIUS else (np.sqrt(np.float64(q[K - 1])) if K else 0.0)
            row["enclosed_mass"] = E[K - 1] if K else 0.0
            for i, name in enumerate(SUMS):
                row[name] = ordered_sum(terms[i, prev:K])
            row["count"], row["enclosed_count"] = K - prev, K
            Ks.append(K)
            prev = K
        state[g] = dict(terms=terms, q=q, E=E, K=Ks)
    out["state"] = state
    return out


def wide(state, K_of_group, n_cuts):
    """For the cuts K_of_group[g][c] (the DEVICE's: the shells are then the same ranks on both sides), per good group
    the long double restatement rounded to fp64 once: the four sums and the enclosed mass of every shell, and the
    absolute sums and term counts their bounds are made of.  -> dict of [G_good, n_cuts(, 4)] arrays keyed by group."""
    res = {}
    for g, st in state.items():
        t = st["terms"].astype(np.longdouble)
        cum = np.cumsum(t[0])
        Ks = [int(k) for k in K_of_group[g]]
        sums, asum, enc = np.zeros((n_cuts, 4)), np.zeros((n_cuts, 4)), np.zeros(n_cuts)
        prev = 0
        for c, K in enumerate(Ks):
            if K > prev:
                sums[c] = t[:, prev:K].sum(axis=1, dtype=np.longdouble).astype(np.float64)
                asum[c] = np.abs(t[:, prev:K]).sum(axis=1, dtype=np.longdouble).astype(np.float64)
            enc[c] = np.float64(cum[K - 1]) if K else 0.0
            prev = max(prev, K)
        res[g] = dict(sums=sums, abs=asum, enclosed=enc, cum=cum)
    return res


def plain_python(fields, offsets, members, centres, cuts, mode, vels=None):
    """The model as nested Python loops over Python floats, for legal catalogues of groups of at most S members.
    -> per group dict(order, q, E, K, sums [n_cuts][4], radius [n_cuts])"""
    mode = MODES.get(mode, mode)
    f = {k: [float(t) for t in a] for k, a in fields.items()}
    res = []
    for g in range(len(offsets) - 1):
        mem = [int(i) for i in members[offsets[g]:offsets[g + 1]]]
        n = len(mem)
        assert 1 <= n <= S
        c = [float(t) for t in centres[g]]
        V = [0.0] * 3 if vels is None else [float(t) for t in vels[g]]
        keyed = []
        for p, i in enumerate(mem):
            d = [f[POS[a]][i] - c[a] for a in range(3)]
            u = [f[VEL[a]][i] - V[a] for a in range(3)]
            r2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
            s = ((u[0] * d[0]) + (u[1] * d[1])) + (u[2] * d[2])
            u2 = ((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2])
            vr = s / math.sqrt(r2) if r2 > 0 else 0.0
            vr2 = vr * vr
            m = f["mass"][i]
            q = np.float32(r2)
            keyed.append((int(q.view(np.uint32)), p, i, q, [m, m * vr, m * vr2, m * (u2 - vr2)]))
        keyed.sort(key=lambda e: (e[0], e[1]))
        E, e = [], None
        for k in keyed:
            e = k[4][0] if e is None else e + k[4][0]
            E.append(e)
        Ks, sums, radius, prev = [], [], [], 0
        for cut in cuts:
            cut = float(cut)
            if mode == NUMBER:
                K = min(n, max(1, int(math.ceil(cut * float(n)))))
            elif mode == MASS:
                T = cut * E[-1]
                K = next((s + 1 for s in range(n) if E[s] >= T), n)
            else:
                K = sum(1 for k in keyed if math.sqrt(float(k[3])) <= cut)
            K = max(K, prev)
            four = []
            for i in range(4):
                acc = 0.0
                for k in keyed[prev:K]:
                    acc = acc + k[4][i]
                four.append(acc)
            sums.append(four)
            radius.append(cut if mode == RADIUS else (math.sqrt(float(keyed[K - 1][3])) if K else 0.0))
            Ks.append(K)
            prev = K
        res.append(dict(order=[k[2] for k in keyed], q=[k[3] for k in keyed], E=E, K=Ks, sums=sums, radius=radius))
    return res


# ---- the two lattices ---------------------------------------------------------------------------------------------------------
LADDER = [1, 2, 3, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C, 2 * C + 1]


def lattice_sizes(small_before=1500, small_after=1500, seed=5):
    """the sizes of the integer lattice: those of the group properties' lattice (every size at which a pass takes another
    path, one group of 64 C + 3, thousands of groups of at most 6 before and after it)"""
    return [int(s) for s in gp.lattice_sizes(small_before, small_after, seed)]


def axis_sizes(small=300, seed=6):
    """the sizes of the axis lattice: the ladder up to 2 C + 1 between small groups"""
    rng = np.random.default_rng(seed)
    return [int(s) for s in list(rng.integers(1, 7, small)) + LADDER + list(rng.integers(1, 7, small))]


def lattice(sizes, count, axis=False, seed=1):
    """A catalogue on which the model is exact.  Integer centres c (|c| <= 500) and integer offsets d, so integer
    coordinates |x| <= 512 and r2 < 2^24: q is exact, and few distinct values give long runs of equal q.  Masses are
    powers of two from 2^-4 to 2^3 (a span within 2^8): every E(s) and M is exact in any order.  Integer velocities
    about an integer bulk velocity.  axis=False: |d_a| <= 8 on every axis.  axis=True: ONE non-zero component, |d| <= 20,
    so r = |d|, vr = +-u_a, vr2 and vt2 are exact too and every field of every shell is.  Every fifth group has its
    first member on the centre; the group of 2 C members has equal masses 1, so that half its mass is rank C exactly.
    The groups' bodies are scattered over [0, count) by a seeded permutation; the rest is background.
    -> (fields, offsets int32, members int32, centres [G, 3] float64, vels [G, 3] float64)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    total, G = int(sizes.sum()), sizes.size
    assert total < count
    gid = np.repeat(np.arange(G), sizes)
    start = np.concatenate(([0], np.cumsum(sizes)))
    c = rng.integers(-500, 501, (G, 3))
    Vg = rng.integers(-16, 17, (G, 3))
    if axis:
        d = np.zeros((total, 3), np.int64)
        d[np.arange(total), rng.integers(0, 3, total)] = rng.integers(-20, 21, total)
    else:
        d = rng.integers(-8, 9, (total, 3))
    d[start[:-1][::5]] = 0
    w = rng.integers(-8, 9, (total, 3))
    m = 2.0 ** rng.integers(-4, 4, total)
    m[np.isin(gid, np.nonzero(sizes == 2 * C)[0])] = 1.0
    members = rng.permutation(count)[:total].astype(np.int32)
    bg = rng.integers(-600, 601, (count, 7)).astype(np.float32)
    fields = {}
    for a in range(3):
        fields[POS[a]] = bg[:, a].copy()
        fields[VEL[a]] = bg[:, 3 + a].copy()
        fields[POS[a]][members] = (c[gid] + d)[:, a]
        fields[VEL[a]][members] = (Vg[gid] + w)[:, a]
    fields["mass"] = np.abs(bg[:, 6]) + 1
    fields["mass"][members] = m
    return fields, start.astype(np.int32), members, c.astype(np.float64), Vg.astype(np.float64)


# the cuts of the lattice tests.  Mass fractions are dyadic: f * M is exact (M has at most 24 bits).  On the lattice some
# group has K = 1 (every group of one member), K = n (f = 1), K = C exactly (f = 1/2 of the group of 2 C equal masses), an
# empty shell (every group of one member from the second cut on), radius 0 (only the members on the centre) and +inf.
LATTICE_CUTS = {"mass": [0.125, 0.25, 0.5, 0.75, 1.0], "number": [0.1, 0.25, 0.5, 0.9, 1.0],
                "radius": [0.0, 2.0, 5.0, 11.5, float("inf")]}
AXIS_CUTS = {"mass": [0.125, 0.5, 1.0], "number": [0.1, 0.5, 1.0], "radius": [0.0, 3.0, 10.0, float("inf")]}


# ---- general data --------------------------------------------------------------------------------------------------------------
FRACTIONS = [0.1, 0.25, 0.5, 0.75, 0.9, 1.0]


def partition(n_bodies, seed=9):
    """an arbitrary partition of the bodies 0 .. n_bodies - 1 into the size ladder (repeated until the bodies run out), so
    that the chunked form meets inexact data.  -> (offsets int32, members int32)"""
    rng = np.random.default_rng(seed)
    members = rng.permutation(n_bodies).astype(np.int32)
    sizes, left, i = [], n_bodies, 0
    ladder = LADDER + [3 * C + 7, 5, 4]
    while left:
        s = min(ladder[i % len(ladder)], left)
        sizes.append(s)
        left -= s
        i += 1
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32), members


U = 2.0 ** -53
# (n + K_SUM) u sum|t| bounds |device - wide reference| of one sum of n terms (a shell's sum over its count, or the
# enclosed mass over its K_c ranks).  Both sides sum the SAME fp64 terms -- the per-member arithmetic is a fixed sequence
# of correctly rounded fp64 operations on both, and the rank order is asserted equal first -- so no rounding inside a
# term counts.  What is left:
#   n - 1  roundings of the device's additions: whatever the order, the sum is a tree over its n terms (the +0 that fill a
#          chunk add exactly), each addition off by at most u times the absolute sum below it <= sum|t|;
#   1      the second-order remainder of those (1 + u)^(n - 1) - 1 <= (n - 1) u (1 + n u), n <= 2^15;
#   1      the reference's own rounding of its long double sum to fp64;
#   16     the reference's long double summation, n 2^-64 sum|t| = n / 2048 u sum|t|, n <= 2^15.
# -1 + 1 + 1 + 16 = 17 <= K_SUM = 18.  sum|t| is the reference's long double sum of the absolute terms.
K_SUM = 18
N_MAX = 2 ** 15


def delta(n):
    """the relative slack of the mass-fraction test: the summation bound of n non-negative terms, (n - 1) u, plus the
    rounding of T and of the reference's two long double quantities: (n + 4) 2^-53"""
    return (n + 4) * U


def mass_cut_checks(cum, n, f, K):
    """(passes, ambiguous) of a device K for the mass fraction f against the wide cumulative mass `cum` (long double):
    passes: E(K - 1) >= T (1 - delta) and (K == 1 or E(K - 2) < T (1 + delta)); ambiguous: K + 1 passes as well"""
    dl = np.longdouble(delta(n))
    T = np.longdouble(f) * cum[n - 1]
    lo, hi = T * (1 - dl), T * (1 + dl)

    def passes(k):
        return 1 <= k <= n and cum[k - 1] >= lo and (k == 1 or cum[k - 2] < hi)

    return passes(K), passes(K) and passes(K + 1)


AMBIGUITY_CAP = 0.001  # at most 0.1 % of the (group, cut) pairs may be ambiguous
