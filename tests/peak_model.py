"""An average for the stream and a peak for every stretch of it, stated over segment_model and the plain models (test
helper).

The definition (include/pacx.h, pacx_rate_solve_peak / pacx_band_solve_peak), and nothing beside it:

  stage A   u_s      = the t of segment_model.solve_segments(seg_first, peaks)               floors()
  stage B   T_s(t)   = max(t, u_s);  total*(t) = sum over s of segment_model.total(slice s, T_s(t))   total_star()
            the plain model's solve -- the probe of t_hi, its bisection -- on total* against the stream's limit: the
            model's own function runs, with its module's total() standing for total* during the call       decide()
  outputs   the plain model's solve of every slice with the range [T_s, T_s] and the segment's peak: t = T_s, met =
            total_s(T_s) <= peak, total, and the per-cf outputs at T_s, stitched by segment_model.solve_segments' rule
"""
from unittest import mock

import numpy as np

import abr_model as am
import band_model as bm
import segment_model as sm

GRID = sm.GRID


def floors(kind, c, seg_first, peaks, t_lo=-30 * GRID, t_hi=30 * GRID):
    return sm.solve_segments(kind, c, seg_first, peaks, t_lo, t_hi)["t"]


def total_star(kind, c, seg_first, u, memo=None):
    """-> the function t -> total*(t); memo keeps total_s at the targets seen (a pinned segment is asked the same
    question at every probe below its floor)"""
    memo = {} if memo is None else memo
    parts = [sm.slice_curve(kind, c, int(a), int(b)) for a, b in zip(seg_first, seg_first[1:])]

    def at(t):
        tot = 0
        for s, part in enumerate(parts):
            key = s, max(int(t), int(u[s]))
            if key not in memo:
                memo[key] = sm.total(kind, part, key[1])
            tot += memo[key]
        return tot
    return at


def decide(kind, star, limit, t_lo, t_hi):
    """the plain model's decision on total*: its solve runs as it is, on a total that is the sum over the segments"""
    model = bm if kind == "band" else am
    total, evaluate = model.total, model.evaluate               # the segments' own totals still go through these
    with mock.patch.object(model, "total", lambda c, t: star(t) if c is None else total(c, t)), \
            mock.patch.object(model, "evaluate", lambda c, t: (star(t), None, None, None) if c is None else evaluate(c, t)):
        r = model.solve(None, int(limit), t_lo, t_hi)           # None: the stream
    return int(r["t"]), int(r["met"]), int(r["total"])


def solve_peak(kind, c, seg_first, peaks, limit, t_lo=-30 * GRID, t_hi=30 * GRID, u=None):
    """-> dict floor, t, met, total [n_seg]; t_stream, met_stream, total_stream; the per-cf outputs.  u: floors() of the
    same arguments, for a caller who has them already"""
    seg_first = [int(v) for v in seg_first]
    u = floors(kind, c, seg_first, peaks, t_lo, t_hi) if u is None else u
    t_star, met_star, tot_star = decide(kind, total_star(kind, c, seg_first, u), limit, t_lo, t_hi)
    solve = bm.solve if kind == "band" else am.solve
    parts = []
    for s, (a, b) in enumerate(zip(seg_first, seg_first[1:])):
        T = max(t_star, int(u[s]))
        parts.append(solve(sm.slice_curve(kind, c, a, b), int(peaks[s]), T, T))
        assert parts[-1]["t"] == T
    out = {"floor": np.asarray(u, np.int64), "t_stream": t_star, "met_stream": met_star, "total_stream": tot_star,
           "t": np.array([p["t"] for p in parts], np.int64), "met": np.array([p["met"] for p in parts], np.int64),
           "total": np.array([p["total"] for p in parts], np.int64)}
    for k in sm.PER_CF[kind]:
        out[k] = np.concatenate([np.asarray(p[k]) for p in parts])
    assert int(out["total"].sum()) == tot_star
    return out


def stream_limits(kind, c, seg_first, peaks, t_lo=-30 * GRID, t_hi=30 * GRID, u=None):
    """four limits for the stream: the midpoint of total*(t_lo) and total*(t_hi); total*(t_hi) - 1, which cannot be
    reached; exactly total*(t_hi); 10^12"""
    star = total_star(kind, c, seg_first, floors(kind, c, seg_first, peaks, t_lo, t_hi) if u is None else u)
    small, big = star(t_hi), star(t_lo)
    return [(small + big) // 2, small - 1, small, 10 ** 12]
