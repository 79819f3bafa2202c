"""The size of a band curve at every target of the grid, stated in NumPy over band_model (test helper).

The definition (include/pacx.h, pacx_band_profile / pacx_profile_solve): profile[g] = band_model.total(c, t_lo + g).
profile() does not evaluate the curve G times; it goes the way the kernel goes:

  per band slot, size i passes from the grid index e_i = ceil(64 nmr[i]) - t_lo on (0 where 64 nmr[i] <= t_lo, never
  where nmr[i] is NaN or 64 nmr[i] > t_hi), decided in floating point before anything is made an integer;
  the pick at g is the smallest i with e_i <= g, so size i holds on [m_i, m_(i-1)), m_i = min(e_0 ... e_i), m_(-1) = G,
  and below every step the band is missed: bits(n_cand - 1);
  per unit the steps go as deltas of a_b lines_b into a difference array over the grid, a running sum gives the unit's
  sum at every g, the cap rule replaces what exceeds the cap by the unit's cap_alloc sum;
  per frame: bits -> ((bits + 4 + 7) >> 3) + 4, summed over the frames.

solve() is band_model.solve's decision with a look-up in the profile where that evaluates the curve.
"""
import numpy as np

import band_model as bm

GRID, SUB = bm.GRID, bm.SUB
PROFILE_MAX = 8193


def steps(c, t_lo, t_hi):
    """e [n_cf, band_stride, n_cand]: the grid index from which each size passes, G where it never does"""
    G = t_hi - t_lo + 1
    x = np.asarray(c["nmr"])[:, :, :c["n_cand"]] * float(GRID)
    with np.errstate(invalid="ignore"):
        passes, low = x <= float(t_hi), x <= float(t_lo)
    inside = passes & ~low                                  # finite, in (t_lo, t_hi]: safe to make an integer
    e = np.full(x.shape, G, np.int64)
    e[low] = 0
    e[inside] = np.ceil(x[inside]).astype(np.int64) - t_lo
    return e


def profile(c, t_lo=-30 * GRID, t_hi=30 * GRID, out=None):
    """-> int64 [G]; with out: added to it (and returned)"""
    G = t_hi - t_lo + 1
    assert 1 <= G <= PROFILE_MAX
    cap = np.asarray(c["cap"]).astype(np.int64)
    n_cf, n_cand = len(cap), c["n_cand"]
    res = np.zeros(G, np.int64) if out is None else out
    if n_cf == 0:
        return res
    if n_cf > 64:                                           # additive over frames: bounded memory, piece by piece
        for a in range(0, n_cf, 64):
            profile(bm.with_arrays(c, c["nmr"][a:a + 64], c["cap"][a:a + 64], c["cap_alloc"][a:a + 64]), t_lo, t_hi, res)
        return res
    unit, lines = bm.layout(c)
    live = unit >= 0
    miss = bm.bits_of(n_cand - 1)
    e = steps(c, t_lo, t_hi)
    diff = np.zeros((n_cf, SUB, G + 1), np.int64)           # [..., G]: where the deltas of "never" go
    cf_i, slot_i = np.nonzero(live)
    u_i, l_i = unit[cf_i, slot_i], lines[cf_i, slot_i]
    hi = np.full(len(cf_i), G, np.int64)
    for i in range(n_cand):
        ei = e[cf_i, slot_i, i]
        on = ei < hi
        d = (bm.bits_of(i) - miss) * l_i
        np.add.at(diff, (cf_i[on], u_i[on], ei[on]), d[on])
        np.add.at(diff, (cf_i[on], u_i[on], hi[on]), -d[on])
        hi = np.where(on, ei, hi)
    base = np.zeros((n_cf, SUB), np.int64)                  # every band missed
    ca = np.zeros((n_cf, SUB), np.int64)                    # sum_b cap_alloc_b lines_b
    np.add.at(base, (cf_i, u_i), miss * l_i)
    np.add.at(ca, (cf_i, u_i), np.asarray(c["cap_alloc"]).astype(np.int64)[cf_i, slot_i] * l_i)
    unit_sum = np.cumsum(diff[:, :, :G], axis=2) + base[:, :, None]
    unit_sum = np.where(unit_sum > cap[:, :, None], ca[:, :, None], unit_sum)
    has = cap >= 0
    units = has.sum(axis=1)
    per_unit = c["n_mant_size_bits"] + c["n_scale_bits"]
    head = units * c["n_scale_bits"] + np.sum(np.where(live, per_unit, 0), axis=1)
    bits = np.sum(np.where(has[:, :, None], unit_sum, 0), axis=1) + head[:, None]
    n_bytes = np.where(units[:, None] > 0, (bits + 4 + 7) >> 3, 0)
    res += np.sum(np.where(n_bytes > 0, n_bytes + 4, 0), axis=0)
    return res


def solve(prof, limit, t_lo=-30 * GRID, t_hi=30 * GRID):
    """band_model.solve's decision on a profile -> dict t, met, total"""
    assert len(prof) == t_hi - t_lo + 1
    if prof[t_hi - t_lo] > limit:
        t, met = t_hi, 0
    else:
        lo, hi, met = t_lo - 1, t_hi, 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if prof[mid - t_lo] <= limit:
                hi = mid
            else:
                lo = mid
        t = hi
    return {"t": t, "met": met, "total": int(prof[t - t_lo])}


def planted(n_cf, seed, t_lo, t_hi, cap_scale=1.0):
    """band_model.synthetic with what the step route can get wrong planted into live rows: values exactly on a grid
    point and one ulp to either side, rows of +inf and of -inf, rows of nothing but NaN, rows entirely below t_lo and
    entirely above t_hi, huge values of either sign"""
    c = bm.synthetic(n_cf, seed, cap_scale=cap_scale)
    rng = np.random.default_rng(seed + 1000)
    unit, _ = bm.layout(c)
    cf_i, slot_i = np.nonzero(unit >= 0)
    n_cand, nmr = c["n_cand"], c["nmr"]
    pick = rng.permutation(len(cf_i))
    kinds = 9
    for j, at in enumerate(pick[:max(kinds * 6, len(pick) // 3)]):
        cf, slot, kind = cf_i[at], slot_i[at], j % kinds
        row = nmr[cf, slot, :n_cand]
        if kind < 3:                                        # on the grid, and one ulp below / above
            t = rng.integers(t_lo - 2, t_hi + 3, n_cand)
            v = t / float(GRID)
            row[:] = v if kind == 0 else np.nextafter(v, -np.inf if kind == 1 else np.inf)
        elif kind == 3:
            row[:] = np.inf
        elif kind == 4:
            row[:] = -np.inf
        elif kind == 5:
            row[:] = np.nan
        elif kind == 6:
            row[:] = t_lo / float(GRID) - rng.uniform(0.001, 50, n_cand)
        elif kind == 7:
            row[:] = t_hi / float(GRID) + rng.uniform(0.001, 50, n_cand)
        else:
            row[:] = rng.choice([1e300, -1e300, 3e9, -3e9, 5e-324, -5e-324], n_cand)
    return c
