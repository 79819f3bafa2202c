"""A profile row per segment, the solve per row and the clamped sum, stated over profile_model (test helper).

The definitions (include/pacx.h, pacx_band_profile_segments / pacx_profile_solve_segments / pacx_profile_clamp_add),
and nothing beside them:

  rows         row s = profile_model.profile of the slice of the curve that is segment s; added to what is there
  solve_rows   per row profile_model.solve against its own limit (a negative limit is never met), and worst_above =
               the largest entry of the row from the target found on
  clamp_add    out[g] += sum over s of row_s[max(g, t_s - t_lo)]
  solve_peak   the two-level solve on rows alone: floors = solve_rows against the peaks, the stream's decision =
               profile_model.solve on the clamped sum, T_s = max(t*, u_s), total_s = row_s[T_s - t_lo]

Segments are any boundaries here (rows) or the uniform stretches the C API takes by value (uniform_first)."""
import numpy as np

import band_model as bm
import profile_model as pm

GRID = bm.GRID


def piece(c, a, b):
    return bm.with_arrays(c, c["nmr"][a:b], c["cap"][a:b], c["cap_alloc"][a:b])


def uniform_first(n_cf, seg_cf, first_off):
    """boundaries, in the piece's frames, of the local segments: frame cf lies in segment (first_off + cf) // seg_cf"""
    assert seg_cf >= 1 and 0 <= first_off < seg_cf
    n_seg = -(-(first_off + n_cf) // seg_cf)
    return np.array([min(max(s * seg_cf - first_off, 0), n_cf) for s in range(n_seg + 1)], np.int64)


def rows(c, seg_first, t_lo, t_hi, out=None):
    """-> int64 [n_seg, G]; with out (at least n_seg rows): added to its first n_seg rows"""
    n_seg = len(seg_first) - 1
    res = np.zeros((n_seg, t_hi - t_lo + 1), np.int64) if out is None else out
    for s, (a, b) in enumerate(zip(seg_first, seg_first[1:])):
        pm.profile(piece(c, int(a), int(b)), t_lo, t_hi, out=res[s])
    return res


def solve_rows(rows_, limits, t_lo, t_hi):
    """-> dict t, met, total, worst_above [n_seg]"""
    out = {k: [] for k in ("t", "met", "total", "worst_above")}
    for row, limit in zip(rows_, limits):
        r = pm.solve(row, int(limit), t_lo, t_hi) if limit >= 0 else {"t": t_hi, "met": 0, "total": int(row[-1])}
        for k in ("t", "met", "total"):
            out[k].append(r[k])
        out["worst_above"].append(int(row[r["t"] - t_lo:].max()))
    return {k: np.array(v, np.int64) for k, v in out.items()}


def clamp_add(rows_, t, t_lo, out=None):
    G = rows_.shape[1]
    res = np.zeros(G, np.int64) if out is None else out
    g = np.arange(G)
    for row, ts in zip(rows_, t):
        res += row[np.maximum(g, int(ts) - t_lo)]
    return res


def solve_peak(rows_, peaks, limit, t_lo, t_hi):
    """-> dict floor, floor_met, worst_above, t, met, total [n_seg]; t_stream, met_stream, total_stream"""
    a = solve_rows(rows_, peaks, t_lo, t_hi)
    star = pm.solve(clamp_add(rows_, a["t"], t_lo), int(limit), t_lo, t_hi)
    t = np.maximum(a["t"], star["t"])
    total = np.array([int(row[ts - t_lo]) for row, ts in zip(rows_, t)], np.int64)
    return {"floor": a["t"], "floor_met": a["met"], "worst_above": a["worst_above"], "t": t,
            "met": (total <= np.asarray(peaks)).astype(np.int64), "total": total,
            "t_stream": star["t"], "met_stream": star["met"], "total_stream": star["total"]}
