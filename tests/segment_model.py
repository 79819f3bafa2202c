"""One noise-to-mask target per stretch of a stream, stated over band_model and abr_model (test helper).

The definition (include/pacx.h, pacx_rate_solve_segments / pacx_band_solve_segments): segment s holds the
channel-frames [seg_first[s], seg_first[s + 1]) and gets what the plain solve gives on that slice of every array with
limits[s].  solve_segments() does exactly that -- slice, band_model.solve / abr_model.solve, stitch -- so it holds no
rule of its own.  material() is the pattern the CPU and GPU tests share: segment lengths that put boundaries inside a
wave, inside a workgroup of either pick kernel and next to empty segments, and limits of four kinds.
"""
import numpy as np

import abr_model as am
import band_model as bm

GRID = 64
LENGTHS = [1, 3, 0, 63, 65, 4, 257, 2, 128, 5]
PER_CF = {"band": ("bit_alloc", "n_bytes", "capped"), "rate": ("budget", "n_bytes", "capped")}


def slice_curve(kind, c, a, b):
    """the curve of the channel-frames [a, b)"""
    if kind == "band":
        return bm.with_arrays(c, c["nmr"][a:b], c["cap"][a:b], c["cap_alloc"][a:b])
    d = dict(c)
    for k in ("worst", "bits", "steps"):
        d[k] = np.asarray(c[k])[a:b]
    return d


def n_cf_of(kind, c):
    return len(c["cap"] if kind == "band" else c["steps"])


def total(kind, c, t):
    return bm.total(c, t) if kind == "band" else am.total(c, t)


def solve_segments(kind, c, seg_first, limits, t_lo=-30 * GRID, t_hi=30 * GRID):
    """-> dict t, met, total [n_seg] and the per-cf outputs of the plain solve (bit_alloc or budget, n_bytes, capped)
    stitched from the segments' own solves"""
    solve = bm.solve if kind == "band" else am.solve
    seg_first = [int(v) for v in seg_first]
    assert seg_first[0] == 0 and seg_first[-1] == n_cf_of(kind, c) and len(limits) == len(seg_first) - 1
    parts = [solve(slice_curve(kind, c, a, b), int(limit), t_lo, t_hi)
             for a, b, limit in zip(seg_first, seg_first[1:], limits)]
    out = {"t": np.array([p["t"] for p in parts], np.int64), "met": np.array([p["met"] for p in parts], np.int64),
           "total": np.array([p["total"] for p in parts], np.int64)}
    for k in PER_CF[kind]:
        out[k] = np.concatenate([np.asarray(p[k]) for p in parts])
    return out


def boundaries(n_cf, lengths=LENGTHS):
    """seg_first for segment lengths cycling through `lengths` until n_cf is used up (the last one cut)"""
    first, i = [0], 0
    while first[-1] < n_cf:
        first.append(min(first[-1] + lengths[i % len(lengths)], n_cf))
        i += 1
    return np.array(first, np.int64)


def limits_for(kind, c, seg_first, t_lo=-30 * GRID, t_hi=30 * GRID):
    """per segment, cycling: the midpoint of total(t_lo) and total(t_hi); max(total(t_hi) - 1, 0), which a segment
    with records cannot reach; exactly total(t_hi); 10^12"""
    out = []
    for s, (a, b) in enumerate(zip(seg_first, seg_first[1:])):
        part = slice_curve(kind, c, int(a), int(b))
        small, big = total(kind, part, t_hi), total(kind, part, t_lo)
        out.append([(small + big) // 2, max(small - 1, 0), small, 10 ** 12][s % 4])
    return np.array(out, np.int64)


def synthetic(kind, n_cf, seed):
    return bm.synthetic(n_cf, seed) if kind == "band" else am.synthetic(n_cf, 40, 12, seed)


def material(kind, seed=7, n_cf=3000):
    """(curve, seg_first, limits) of the shared pattern"""
    c = synthetic(kind, n_cf, seed)
    first = boundaries(n_cf)
    return c, first, limits_for(kind, c, first)
