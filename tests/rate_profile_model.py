"""The size of a rate curve at every target of the grid, per stream and per segment, and the pick at a known target,
stated in NumPy over abr_model (test helper).

The definitions (include/pacx.h, pacx_rate_profile / pacx_rate_profile_segments / pacx_rate_pick[_segments]):

  profile        profile[g] = abr_model.total(c, t_lo + g), evaluated target by target: the definition, G evaluations.
                 Before it, the one rule of pacx_rate_solve that abr_model leaves to its caller: a J that would leave
                 its row is cut to the row (cut()).
  profile_steps  the way the kernel goes, all g at once: entry j passes from the grid index
                 e_j = ceil(64 worst[j]) - t_lo on (0 where 64 worst[j] <= t_lo, never where worst[j] is NaN or
                 64 worst[j] > t_hi), decided in floating point before anything is made an integer; the pick at g is
                 abr_model.pick's bisection with ok(j) := e_j <= g.  The CPU tests assert it equal to profile(); the
                 GPU tests compare with it.
  rows           row s = the profile of the slice of the curve that is segment s; added to what is there
  pick           abr_model.evaluate at the target; pick_segments: per segment at its own target, stitched
"""
import numpy as np

import abr_model as am

GRID, SUB = am.GRID, am.SUB
PROFILE_MAX = 8193


def piece(c, a, b):
    d = dict(c)
    for k in ("worst", "bits", "steps"):
        d[k] = np.asarray(c[k])[a:b]
    return d


def narrowed(c, row):
    """the same arrays read with a shorter row (row >= 7 sub_stride + 1): units whose J leaves it are cut by the rule"""
    assert 7 * c["sub_stride"] + 1 <= row <= c["row"]
    d = dict(c)
    d["worst"], d["bits"], d["row"] = np.ascontiguousarray(c["worst"][:, :row]), np.ascontiguousarray(c["bits"][:, :row]), row
    return d


def cut(c):
    """steps with every J that would leave its row cut to the row (include/pacx.h, pacx_rate_solve)"""
    steps = np.asarray(c["steps"]).astype(np.int64)
    room = c["row"] - 1 - np.arange(SUB)[None, :] * c["sub_stride"]
    assert (room >= 0).all()
    d = dict(c)
    d["steps"] = np.where(steps >= 0, np.minimum(steps, room), steps).astype(np.int32)
    return d


def profile(c, t_lo, t_hi, out=None):
    """the definition -> int64 [G]; with out: added to it (and returned)"""
    G = t_hi - t_lo + 1
    assert 1 <= G <= PROFILE_MAX
    res = np.zeros(G, np.int64) if out is None else out
    if len(c["steps"]):
        cc = cut(c)
        res += np.array([am.total(cc, t_lo + g) for g in range(G)], np.int64)
    return res


def thresholds(worst, t_lo, t_hi):
    """e, int64 like worst: the grid index from which each entry passes, G where it never does"""
    G = t_hi - t_lo + 1
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(worst) * float(GRID)
        passes, low = x <= float(t_hi), x <= float(t_lo)
    inside = passes & ~low                                  # finite, in (t_lo, t_hi]: safe to make an integer
    e = np.full(x.shape, G, np.int64)
    e[low] = 0
    e[inside] = np.ceil(x[inside]).astype(np.int64) - t_lo
    return e


def profile_steps(c, t_lo, t_hi, out=None, frames=16):
    """the threshold route -> int64 [G]; with out: added to it (and returned)"""
    G = t_hi - t_lo + 1
    assert 1 <= G <= PROFILE_MAX
    res = np.zeros(G, np.int64) if out is None else out
    n_cf = len(c["steps"])
    if n_cf > frames:                                       # additive over frames: bounded memory, piece by piece
        for a in range(0, n_cf, frames):
            profile_steps(piece(c, a, a + frames), t_lo, t_hi, res, frames)
        return res
    if n_cf == 0:
        return res
    steps = cut(c)["steps"].astype(np.int64)
    e, bits = thresholds(c["worst"], t_lo, t_hi), np.asarray(c["bits"]).astype(np.int64)
    live = steps >= 0
    J = np.where(live, steps, 0)[:, :, None]                                       # [n_cf, 8, 1]
    g = np.arange(G)[None, None, :]
    cf = np.arange(n_cf)[:, None, None]
    at = (np.arange(SUB) * c["sub_stride"])[None, :, None]
    ok = lambda j: e[cf, at + j] <= g                                              # noqa: E731
    cap = ~ok(J)
    lo, hi = np.where(cap, J, -1) + 0 * g, J + 0 * g
    while True:
        go = hi - lo > 1
        if not go.any():
            break
        mid = np.where(go, (lo + hi) // 2, hi)
        good = ok(mid)
        hi = np.where(go & good, mid, hi)
        lo = np.where(go & ~good, mid, lo)
    unit_bits = np.where(live[:, :, None], bits[cf, at + hi], 0)
    n_bytes = np.where(live.any(axis=1)[:, None], (unit_bits.sum(axis=1) + 4 + 7) >> 3, 0)
    res += np.sum(np.where(n_bytes > 0, n_bytes + 4, 0), axis=0)
    return res


def rows(c, seg_first, t_lo, t_hi, out=None, route=profile_steps):
    """-> int64 [n_seg, G]; with out (at least n_seg rows): added to its first n_seg rows"""
    n_seg = len(seg_first) - 1
    res = np.zeros((n_seg, t_hi - t_lo + 1), np.int64) if out is None else out
    for s, (a, b) in enumerate(zip(seg_first, seg_first[1:])):
        route(piece(c, int(a), int(b)), t_lo, t_hi, out=res[s])
    return res


def pick(c, t):
    """every frame at t / 64 -> dict budget [n_cf, 8], n_bytes [n_cf], capped [n_cf]"""
    _, budget, n_bytes, capped = am.evaluate(cut(c), int(t))
    return {"budget": budget, "n_bytes": n_bytes, "capped": capped}


def pick_segments(c, seg_first, targets):
    parts = [pick(piece(c, int(a), int(b)), t) for a, b, t in zip(seg_first, seg_first[1:], targets)]
    return {k: np.concatenate([p[k] for p in parts]) for k in ("budget", "n_bytes", "capped")}


def planted(n_cf, seed, t_lo, t_hi, j_long=40, j_short=12, **kw):
    """abr_model.synthetic with what the threshold route can get wrong planted into the entries of live units: values
    exactly on a grid point and one ulp to either side, +inf, -inf, NaN (for whole units, and at single entries inside
    [0, J] with J itself among them), units entirely below t_lo and entirely above t_hi, huge values of either sign
    (1e300: its 64-fold overflows) and denormals"""
    c = am.synthetic(n_cf, j_long, j_short, seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    cf_i, sb_i = np.nonzero(c["steps"] >= 0)
    order = rng.permutation(len(cf_i))
    kinds = 11
    for n, i in enumerate(order[:max(kinds * 6, len(order) // 2)]):
        cf, sb, kind = cf_i[i], sb_i[i], n % kinds
        J = int(c["steps"][cf, sb])
        w = c["worst"][cf, sb * c["sub_stride"]:sb * c["sub_stride"] + J + 1]
        if kind < 3:                                        # on the grid, and one ulp below / above
            v = rng.integers(t_lo - 2, t_hi + 3, J + 1) / float(GRID)
            w[:] = v if kind == 0 else np.nextafter(v, -np.inf if kind == 1 else np.inf)
        elif kind == 3:
            w[:] = np.inf
        elif kind == 4:
            w[:] = -np.inf
        elif kind == 5:
            w[:] = np.nan
        elif kind == 6:
            w[:] = t_lo / float(GRID) - rng.uniform(0.001, 50, J + 1)
        elif kind == 7:
            w[:] = t_hi / float(GRID) + rng.uniform(0.001, 50, J + 1)
        elif kind == 8:
            w[:] = rng.choice([1e300, -1e300, 3e9, -3e9, 5e-324, -5e-324, 2.2e-308], J + 1)
        elif kind == 9:                                     # NaN at J: the cap test fails whatever the target
            w[J] = np.nan
        else:                                               # NaN and the infinities somewhere inside
            w[rng.integers(0, J + 1, 3)] = rng.choice([np.nan, np.inf, -np.inf], 3)
    return c
