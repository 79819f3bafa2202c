"""Coding to an average bit rate, stated in NumPy over rate_model (test helper).

The definition (include/pacx.h, pacx_rate_curve_batch / pacx_rate_solve).  Units, cap and J are rate_model's.

  The curve, per unit, j = 0 ... J:
    worst[j] = max_b NMR_b of the unit coded with BitAlloc budget 32 j     (rate_model.code_unit, nmr_model.band_values)
    bits[j]  = oracle.pac_oracle.block_bits of that allocation
  One row of `row` entries per channel-frame, sub-block sb at sb * sub_stride; steps [n_cf, 8] = J, -1 without a unit.

  The solve, T = t / 64 dB, t an integer in [t_lo, t_hi]:
    pick(unit, T): rate_model.search_unit's bisection with ok(j) := worst[j] <= T -> j*; not ok(J): j* = J, capped
    bytes(cf, T) = 0 for a dropped hop, else ((sum over its units of bits[j*]) + 4 + 7) >> 3
    total(T)     = sum over cf with bytes > 0 of (bytes + 4)
    total(t_hi) > limit: met = 0, t = t_hi;  else lo = t_lo - 1, hi = t_hi, bisection on total(mid) <= limit, t = hi

curve() needs the analysis of rate_model; pick / frame / total / solve work on the arrays alone, the GPU's included.
"""
import numpy as np

import nmr_model as nm
import rate_model as rm
from oracle import pac_oracle as po

SUB, STEP, GRID = rm.SUB, rm.STEP, 64


def steps_of(a, max_kbps, short, last_or_next):
    """J of a long block / short sub-block with these flags: the budget rule with the cap rate, in steps of 32 bits"""
    pc = po.make_params(a["sample_rate"], a["n_ch"], max_kbps, rm.HOP, *rm.widths(a))
    if short:
        pc.nMDCTLines = pc.nSamplesPerBlock = rm.SHORT
    return max(int(np.floor(po.bit_budget(pc, last_or_next, short, False) / STEP)), 0)


def layout(a, max_kbps):
    """(row, sub_stride): the maximum over the flag combinations"""
    j_long = max(steps_of(a, max_kbps, False, lon) for lon in (False, True))
    j_short = max(steps_of(a, max_kbps, True, lon) for lon in (False, True))
    return max(j_long + 1, SUB * (j_short + 1)), j_short + 1


def curve(a, max_kbps, fill_worst=np.nan, fill_bits=0):
    """-> dict worst float64 [n_cf, row], bits int32 [n_cf, row], steps int32 [n_cf, 8], row, sub_stride, evals;
    entries no unit uses hold the fill values"""
    p, n_ch = a["p"], a["n_ch"]
    row, sub = layout(a, max_kbps)
    n_cf = len(a["flags"]) * n_ch
    worst = np.full((n_cf, row), fill_worst, np.float64)
    bits = np.full((n_cf, row), fill_bits, np.int32)
    steps = np.full((n_cf, SUB), -1, np.int32)
    evals = 0
    for f, units in enumerate(a["units"]):
        if units is None:
            continue
        for ch, us in enumerate(units):
            cf = f * n_ch + ch
            for sb, u in enumerate(us):
                J = rm.cap_steps(a, u, max_kbps)
                steps[cf, sb] = J
                for j in range(J + 1):
                    (sf, alloc, mant, overall), xh = rm.code_unit(p, u, STEP * j)
                    worst[cf, sb * sub + j] = np.max(nm.band_values(u.x, xh, u.thr, u.bands)[2])
                    bits[cf, sb * sub + j] = po.block_bits(p, alloc, u.short)
                    evals += 1
    return {"worst": worst, "bits": bits, "steps": steps, "row": row, "sub_stride": sub, "evals": evals}


def pick(worst, J, T):
    """one unit: worst[0 ... J] -> (j*, capped)"""
    if not worst[J] <= T:
        return J, True
    lo, hi = -1, J
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if worst[mid] <= T:
            hi = mid
        else:
            lo = mid
    return hi, False


def frame(c, cf, T):
    """one channel-frame -> (budget int32 [8], bytes, capped)"""
    budget, total, capped, units = np.zeros(SUB, np.int32), 0, False, 0
    for sb in range(SUB):
        J = int(c["steps"][cf, sb])
        if J < 0:
            continue
        at = sb * c["sub_stride"]
        j, cap = pick(c["worst"][cf, at:at + J + 1], J, T)
        budget[sb], total, capped, units = STEP * j, total + int(c["bits"][cf, at + j]), capped or cap, units + 1
    return budget, ((total + 4 + 7) >> 3) if units else 0, capped


def total_slow(c, t):
    """total(t) by pick() and frame(), unit by unit"""
    n = [frame(c, cf, t / GRID)[1] for cf in range(len(c["steps"]))]
    return sum(b + 4 for b in n if b > 0)


def evaluate(c, t):
    """every channel-frame at T = t / 64, all units at once: -> (total, budget [n_cf, 8], n_bytes [n_cf], capped
    [n_cf]); the same bisection as pick(), carried for all units together"""
    T = t / GRID
    steps = np.asarray(c["steps"], np.int64)
    n_cf = len(steps)
    worst, bits = np.asarray(c["worst"]), np.asarray(c["bits"])
    live = steps >= 0
    J = np.where(live, steps, 0)
    base = np.arange(n_cf)[:, None], np.arange(SUB)[None, :] * c["sub_stride"]
    at = lambda j: worst[base[0], base[1] + j]                                    # noqa: E731
    with np.errstate(invalid="ignore"):
        cap = live & ~(at(J) <= T)
    lo, hi = np.where(live & ~cap, -1, J), J.copy()
    while True:
        go = hi - lo > 1
        if not go.any():
            break
        mid = np.where(go, (lo + hi) // 2, hi)
        with np.errstate(invalid="ignore"):
            ok = at(mid) <= T
        hi = np.where(go & ok, mid, hi)
        lo = np.where(go & ~ok, mid, lo)
    unit_bits = np.where(live, bits[base[0], base[1] + hi], 0).astype(np.int64)
    n_bytes = np.where(live.any(axis=1), (unit_bits.sum(axis=1) + 4 + 7) >> 3, 0)
    budget = np.where(live, STEP * hi, 0).astype(np.int32)
    return int(np.sum(n_bytes[n_bytes > 0] + 4)), budget, n_bytes.astype(np.int32), cap.any(axis=1)


def total(c, t):
    return evaluate(c, t)[0]


def solve(c, limit, t_lo=-30 * GRID, t_hi=30 * GRID):
    """-> dict t, met, total, budget, n_bytes, capped, path: (t, total(t)) of every probe in order"""
    path = [(t_hi, total(c, t_hi))]
    if path[0][1] > limit:
        t, met = t_hi, 0
    else:
        lo, hi, met = t_lo - 1, t_hi, 1
        while hi - lo > 1:
            mid = (lo + hi) // 2                                   # floor, for negative sums too
            path.append((mid, total(c, mid)))
            if path[-1][1] <= limit:
                hi = mid
            else:
                lo = mid
        t = hi
    tot, budget, n_bytes, capped = evaluate(c, t)
    return {"t": t, "met": met, "total": tot, "budget": budget, "n_bytes": n_bytes, "capped": capped, "path": path}


def pairs(t_lo, t_hi):
    """launch pairs the device solve enqueues: 2 + ceil(log2(t_hi - t_lo + 2))"""
    n = 0
    while (1 << n) < t_hi - t_lo + 2:
        n += 1
    return 2 + n


def synthetic(n_cf, j_long, j_short, seed, p_short=0.3, p_drop=0.1):
    """a curve no encoder made: mixed long / short / dropped channel-frames, random J, random non-monotone worst
    (falling from +25 to -25 dB over the unit's steps under +-6 dB of noise), random bits; unused entries NaN / -1"""
    rng = np.random.default_rng(seed)
    sub = j_short + 1
    row = max(j_long + 1, SUB * sub)
    worst = np.full((n_cf, row), np.nan)
    bits = np.full((n_cf, row), -1, np.int32)
    steps = np.full((n_cf, SUB), -1, np.int32)
    kind = rng.choice(3, n_cf, p=[1 - p_short - p_drop, p_short, p_drop])
    for cf in range(n_cf):
        if kind[cf] == 2:
            continue
        for sb in range(SUB if kind[cf] == 1 else 1):
            J = int(rng.integers(0, (j_short if kind[cf] == 1 else j_long) + 1))
            steps[cf, sb] = J
            at = sb * sub
            worst[cf, at:at + J + 1] = 25.0 - np.arange(J + 1) * (50.0 / (J + 1)) + rng.uniform(-6, 6, J + 1)
            bits[cf, at:at + J + 1] = rng.integers(100, 200) + 32 * np.arange(J + 1) + rng.integers(-40, 41, J + 1)
    return {"worst": worst, "bits": bits, "steps": steps, "row": row, "sub_stride": sub}
