"""Per-block targets under a leaky bucket (include/pacx_bucket_pin.h: pacx_bucket_through, pacx_band_solve_bucket_pinned /
pacx_rate_solve_bucket_pinned) in plain Python integers (test helper), on top of bucket_model:

    R_h       = X_h + max(0, R_h+1 - drain)        nothing behind the last hop
    through_h = F_h + R_h

through() walks the recursion; brute() takes the maximum over all stretches of consecutive hops that contain h, the
start level counted as a stretch that begins before hop 0; solve() is the header's pinned solve, phase by phase, over
bucket_model.scan, with the path of every probe.
"""
import bucket_model as kb

Q = kb.Q
PHASES_MAX = 16


def through(n_bytes, n_ch, bucket):
    """-> (through_h of every hop, bucket_model.scan's dict)"""
    drain = int(bucket[0])
    s = kb.scan(n_bytes, n_ch, bucket)
    X = [x << Q for x in kb.hop_bytes(n_bytes, n_ch)]
    R, behind = [0] * len(X), 0
    for h in range(len(X) - 1, -1, -1):
        R[h] = X[h] + max(0, behind - drain)
        behind = R[h]
    return [lv - x + r for lv, x, r in zip(s["level"], X, R)], s              # F_h = L_h - X_h


def brute(n_bytes, n_ch, bucket):
    """through_h as the highest level any stretch a ... e with a <= h <= e brings the buffer to at hop e: from an empty
    buffer at a, X_a + ... + X_e - (e - a) drain; from the start level before hop 0, that too"""
    drain, _, start = (int(v) for v in bucket)
    X = [x << Q for x in kb.hop_bytes(n_bytes, n_ch)]
    n, out = len(X), []
    for h in range(n):
        best = None
        for e in range(h, n):
            cands = [start + sum(X[:e + 1]) - e * drain]
            cands += [sum(X[a:e + 1]) - (e - a) * drain for a in range(h + 1)]
            best = max(cands + ([best] if best is not None else []))
        out.append(best)
    return out


def per_hop(uniform, n_ch):
    """uniform(t) -> band_model.evaluate's / abr_model.evaluate's tuple at one target (a frame's outputs depend on its
    own target only).  -> evaluate(targets): the same tuple with hop h at targets[h], row by row from uniform() at
    every distinct target"""
    import numpy as np

    def evaluate(targets):
        tg = np.repeat(np.asarray(targets, np.int64), n_ch)
        got = {int(u): uniform(int(u)) for u in np.unique(tg)}
        if not got:
            return uniform(0)                                                     # no frames: the empty arrays
        first = next(iter(got.values()))
        per_cf, n_bytes, capped = (np.array(first[i], copy=True) for i in (1, 2, 3))
        for u, g in got.items():
            at = tg == u
            per_cf[at], n_bytes[at], capped[at] = g[1][at], g[2][at], g[3][at]
        return int(np.sum(n_bytes[n_bytes > 0] + 4)), per_cf, n_bytes, capped
    return evaluate


def solve(evaluate, n_ch, n_hops, limit, bucket, t_lo=-30 * 64, t_hi=30 * 64, pin_step_t=64, max_phases=8):
    """evaluate(targets) -> bytes(A): band_model.evaluate's / abr_model.evaluate's tuple (total, per channel-frame,
    n_bytes, capped) with hop h at the grid target targets[h], or just n_bytes.  -> dict t, met, total, target_t,
    phase_of, phases, open, levels (p_k of every phase), n_bytes, per_cf, capped, bucket (scan's dict of the bytes
    returned) and path: a tuple (phase, "fit", level, total, peak_q16, fits) for every probe of a bisection and
    (phase, "freeze", q, hops pinned) for every through-scan, in order"""
    assert pin_step_t >= 1 and 1 <= max_phases <= PHASES_MAX
    size_q16 = int(bucket[1]) << Q
    pin, phase_of, path = [t_lo - 1] * n_hops, [-1] * n_hops, []

    def A(p):
        return [max(p, v) for v in pin]

    def nb(got):
        return got[2] if isinstance(got, tuple) else got

    def fits(k, p):
        s = kb.scan(nb(evaluate(A(p))), n_ch, bucket)
        ok = s["total"] <= limit and s["peak_q16"] <= size_q16
        path.append((k, "fit", p, s["total"], s["peak_q16"], ok))
        return ok

    T, met, phases, still_open, levels = t_hi, 1, 0, 0, []
    for k in range(max_phases):
        if k == 0 and not fits(0, t_hi):
            met = 0
            break
        phases += 1
        lo, hi = t_lo - 1, T
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fits(k, mid):
                hi = mid
            else:
                lo = mid
        T = hi
        levels.append(T)
        if T == t_lo:
            break
        q = max(t_lo, T - pin_step_t)
        thr, _ = through(nb(evaluate(A(q))), n_ch, bucket)
        frozen = [h for h in range(n_hops) if pin[h] < t_lo and thr[h] > size_q16]
        for h in frozen:
            pin[h], phase_of[h] = T, k
        path.append((k, "freeze", q, len(frozen)))
        if not frozen:
            break
        if k == max_phases - 1:
            still_open = 1
    target_t = A(T)
    got = evaluate(target_t)
    whole = isinstance(got, tuple)
    s = kb.scan(nb(got), n_ch, bucket)
    return {"t": T, "met": met, "total": s["total"], "target_t": target_t, "phase_of": phase_of, "phases": phases,
            "open": still_open, "levels": levels, "n_bytes": nb(got), "per_cf": got[1] if whole else None,
            "capped": got[3] if whole else None, "bucket": s, "path": path}
