"""A curve kept as thresholds and the picks on that form, stated in NumPy (test helper).

The definition (include/pacx.h, pacx_band_thresholds / pacx_rate_thresholds and the four picks on them).  With
[t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db] and G = t_hi - t_lo + 1, the threshold of a curve entry x is the grid index from
which it passes: 0 where 64 x <= t_lo, ceil(64 x) - t_lo inside, G ("never") where x is NaN, +inf or above the range --
exactly profile_model.steps / rate_profile_model.thresholds, which this module calls and does not restate.

  band_thresholds  e uint16 [n_cf, band_stride, 16]: G for candidates i >= n_cand, for slots no band of the frame uses and
                   for every slot of a dropped hop; cap copied; cap_alloc uint8, saturated, 0 where there is no band
  rate_thresholds  e uint16 [n_cf, row]; bits int32, 0 where no unit uses the entry (there e = G); steps cut to the row
  band_pick        per band the smallest i in ascending order with e_i <= g; miss rule, cap rule, bits and bytes as
                   band_model.evaluate, written out again on the integers
  rate_pick        abr_model.evaluate's bisection with ok(j) := e_j <= g, the cap test on entry J first
  *_segments       frame cf at target_t[(first_off + cf) // seg_cf], clamped into the range

The picks read nothing but the kept arrays and the tables: that they equal the models on the curve itself at every grid
target is what tests/test_kept_model.py asserts.
"""
import numpy as np

import band_model as bm
import profile_model as pm
import rate_profile_model as rpm

GRID, SUB, CAND = bm.GRID, bm.SUB, bm.CAND
KEPT_KEYS = ("n_scale_bits", "n_mant_size_bits", "n_cand", "band_stride", "lines_long", "lines_short")


def band_bytes_per_cf(band_stride):
    return 33 * band_stride + 32


def rate_bytes_per_cf(row):
    return 6 * row + 32


def band_thresholds(c, t_lo, t_hi):
    """c: a band curve with band_model.tables() -> the kept dict (the tables carried along)"""
    G = t_hi - t_lo + 1
    assert 1 <= G <= pm.PROFILE_MAX
    cap = np.asarray(c["cap"]).astype(np.int32)
    n_cf, stride = len(cap), c["band_stride"]
    unit, _ = bm.layout(c)
    live = unit >= 0
    e = np.full((n_cf, stride, CAND), G, np.int64)
    e[:, :, :c["n_cand"]] = np.where(live[:, :, None], pm.steps(c, t_lo, t_hi), G)
    ca = np.where(live, np.clip(np.asarray(c["cap_alloc"]).astype(np.int64), 0, 255), 0)
    kept = {k: c[k] for k in KEPT_KEYS}
    kept.update(e=e.astype(np.uint16), cap=cap.copy(), cap_alloc=ca.astype(np.uint8), t_lo=t_lo, t_hi=t_hi)
    return kept


def _band_layout(kept):
    return bm.layout({"cap": kept["cap"], "band_stride": kept["band_stride"], "lines_long": kept["lines_long"],
                      "lines_short": kept["lines_short"]})


def band_pick_at(kept, g):
    """g: int [n_cf], the grid index of every frame's target -> dict bit_alloc, n_bytes, capped"""
    e, cap = kept["e"].astype(np.int64), kept["cap"].astype(np.int64)
    n_cf, n_cand = len(cap), kept["n_cand"]
    unit, lines = _band_layout(kept)
    live = unit >= 0
    ok = e[:, :, :n_cand] <= np.asarray(g, np.int64)[:, None, None]
    hit = ok.any(axis=2)
    a = np.where(hit, bm.BITS[np.argmax(ok, axis=2)], bm.bits_of(n_cand - 1))
    a = np.where(live, a, 0)
    capped = np.zeros(n_cf, bool)
    for sb in range(SUB):
        mine = unit == sb
        over = (np.sum(np.where(mine, a * lines, 0), axis=1) > cap[:, sb]) & (cap[:, sb] >= 0)
        capped |= over | (mine & ~hit).any(axis=1)
        a = np.where(mine & over[:, None], kept["cap_alloc"].astype(np.int64), a)
    units = (cap >= 0).sum(axis=1)
    bits = np.sum(np.where(live, kept["n_mant_size_bits"] + kept["n_scale_bits"] + a * lines, 0), axis=1) + \
        units * kept["n_scale_bits"]
    n_bytes = np.where(units > 0, (bits + 4 + 7) >> 3, 0)
    return {"bit_alloc": a.astype(np.int32), "n_bytes": n_bytes.astype(np.int32), "capped": capped}


def _grid_index(kept, t):
    return np.clip(np.asarray(t, np.int64), kept["t_lo"], kept["t_hi"]) - kept["t_lo"]


def _segment_targets(n_cf, seg_cf, first_off, target_t):
    assert seg_cf >= 1 and 0 <= first_off < seg_cf
    seg = (first_off + np.arange(n_cf)) // seg_cf
    assert len(target_t) == (-(-(first_off + n_cf) // seg_cf))
    return np.asarray(target_t, np.int64)[seg] if n_cf else np.zeros(0, np.int64)


def band_pick(kept, t):
    assert kept["t_lo"] <= t <= kept["t_hi"]
    return band_pick_at(kept, _grid_index(kept, np.full(len(kept["cap"]), t)))


def band_pick_segments(kept, seg_cf, first_off, target_t):
    return band_pick_at(kept, _grid_index(kept, _segment_targets(len(kept["cap"]), seg_cf, first_off, target_t)))


def rate_thresholds(c, t_lo, t_hi):
    """c: a rate curve (worst, bits, steps, row, sub_stride) -> the kept dict"""
    G = t_hi - t_lo + 1
    assert 1 <= G <= rpm.PROFILE_MAX
    row, sub = c["row"], c["sub_stride"]
    steps = rpm.cut(c)["steps"].astype(np.int64) if len(c["steps"]) else np.zeros((0, SUB), np.int64)
    n_cf = len(steps)
    j = np.arange(row)[None, None, :] - (np.arange(SUB) * sub)[None, :, None]                 # [1, 8, row]
    used = ((steps[:, :, None] >= 0) & (j >= 0) & (j <= steps[:, :, None])).any(axis=1)       # [n_cf, row]
    worst = np.asarray(c["worst"]).reshape(n_cf, row)
    e = np.where(used, rpm.thresholds(worst, t_lo, t_hi), G)
    bits = np.where(used, np.asarray(c["bits"]).reshape(n_cf, row), 0)
    return {"e": e.astype(np.uint16), "bits": bits.astype(np.int32), "steps": steps.astype(np.int32), "row": row,
            "sub_stride": sub, "t_lo": t_lo, "t_hi": t_hi}


def rate_pick_at(kept, g):
    e, bits, steps = kept["e"].astype(np.int64), kept["bits"].astype(np.int64), kept["steps"].astype(np.int64)
    n_cf = len(steps)
    g = np.asarray(g, np.int64)[:, None]
    live = steps >= 0
    J = np.where(live, steps, 0)
    base = np.arange(n_cf)[:, None], np.arange(SUB)[None, :] * kept["sub_stride"]
    ok = lambda j: e[base[0], base[1] + j] <= g                                               # noqa: E731
    cap = live & ~ok(J)
    lo, hi = np.where(live & ~cap, -1, J), J.copy()
    while True:
        go = hi - lo > 1
        if not go.any():
            break
        mid = np.where(go, (lo + hi) // 2, hi)
        good = ok(mid)
        hi = np.where(go & good, mid, hi)
        lo = np.where(go & ~good, mid, lo)
    unit_bits = np.where(live, bits[base[0], base[1] + hi], 0)
    n_bytes = np.where(live.any(axis=1), (unit_bits.sum(axis=1) + 4 + 7) >> 3, 0)
    return {"budget": np.where(live, 32 * hi, 0).astype(np.int32), "n_bytes": n_bytes.astype(np.int32),
            "capped": cap.any(axis=1)}


def rate_pick(kept, t):
    assert kept["t_lo"] <= t <= kept["t_hi"]
    return rate_pick_at(kept, _grid_index(kept, np.full(len(kept["steps"]), t)))


def rate_pick_segments(kept, seg_cf, first_off, target_t):
    return rate_pick_at(kept, _grid_index(kept, _segment_targets(len(kept["steps"]), seg_cf, first_off, target_t)))
