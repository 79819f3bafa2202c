"""The leaky bucket of include/pacx_bucket.h (pacx_bucket_scan, pacx_band_solve_bucket / pacx_rate_solve_bucket) in plain Python
integers (test helper).  A hop h is n_ch consecutive channel-frames; levels are integers in 1 / 65536 byte:

    x_h   = sum over the hop's channel-frames of (n_bytes > 0 ? n_bytes + 4 : 0)
    L_h   = F_h + (x_h << 16),  F_0 = start,  F_h+1 = max(0, L_h - drain)

scan() walks the hops one after the other; quadratic() states every L_h without a recursion; then() / apply() are the
composition rule the kernel's scan rests on; solve() is band_model.solve's / abr_model.solve's bisection with the
bucket's peak as a second condition; the two refusals are the strings pacfile.encode_stream_abr_buffered raises.
"""
from fractions import Fraction

Q = 16
SIZE_MAX = 1 << 40
FIELDS = ("total", "peak_q16", "peak_hop", "first_over", "end_q16")


def hop_bytes(n_bytes, n_ch):
    """x_h of every hop, Python ints"""
    nb = [int(v) for v in n_bytes]
    assert n_ch >= 1 and len(nb) % n_ch == 0
    return [sum(v + 4 for v in nb[h * n_ch:(h + 1) * n_ch] if v > 0) for h in range(len(nb) // n_ch)]


def scan(n_bytes, n_ch, bucket):
    """-> dict total, peak_q16, peak_hop, first_over, end_q16 and level, the list of every L_h"""
    drain, size, start = (int(v) for v in bucket)
    level, f = [], start
    for x in hop_bytes(n_bytes, n_ch):
        level.append(f + (x << Q))
        f = max(0, level[-1] - drain)
    peak = max([start] + level)
    return {"total": sum(hop_bytes(n_bytes, n_ch)), "peak_q16": peak,
            "peak_hop": level.index(peak) if peak > start else -1,
            "first_over": next((h for h, v in enumerate(level) if v > size << Q), -1), "end_q16": f, "level": level}


def quadratic(x, drain, start):
    """every L_h without a recursion: never emptied, start + all the bytes so far - the drain of h hops; emptied last
    before hop a, the bytes of the hops a ... h - the drain of h - a hops; the level is the largest of these"""
    X = [int(v) << Q for v in x]
    return [max([start + sum(X[:h + 1]) - drain * h] + [sum(X[a:h + 1]) - drain * (h - a) for a in range(h + 1)])
            for h in range(len(X))]


def hop_map(x, drain):
    """one hop as the map F -> max(lo, F + s): the pair (s, lo)"""
    return (int(x) << Q) - drain, 0


def then(a, b):
    """a, then b"""
    return a[0] + b[0], max(b[1], a[1] + b[0])


def apply(m, f):
    return max(m[1], f + m[0])


def drain_q16(kbps_per_channel, n_ch, sample_rate, hop=1024):
    """what leaves per hop, rounded down: never more than the rate itself"""
    per_hop = Fraction(kbps_per_channel) * 1000 * n_ch * hop / (8 * sample_rate)          # bytes
    return (per_hop * (1 << Q)).numerator // (per_hop * (1 << Q)).denominator


def solve(evaluate, n_ch, limit, bucket, t_lo=-30 * 64, t_hi=30 * 64):
    """evaluate(t) -> band_model.evaluate's / abr_model.evaluate's tuple (total, per channel-frame, n_bytes, capped) at
    the grid target t, or just n_bytes.  -> dict t, met, total, n_bytes, per_cf, capped, bucket (scan's dict at t) and
    path: (t, total, peak_q16, fits) of every probe in order"""
    size = int(bucket[1])

    def probe(t):
        got = evaluate(t)
        n_bytes = got[2] if isinstance(got, tuple) else got
        s = scan(n_bytes, n_ch, bucket)
        return got, s, s["total"] <= limit and s["peak_q16"] <= size << Q

    path = []

    def fits(t):
        _, s, ok = probe(t)
        path.append((t, s["total"], s["peak_q16"], ok))
        return ok

    if not fits(t_hi):
        t, met = t_hi, 0
    else:
        lo, hi, met = t_lo - 1, t_hi, 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fits(mid):
                hi = mid
            else:
                lo = mid
        t = hi
    got, s, _ = probe(t)
    whole = isinstance(got, tuple)
    return {"t": t, "met": met, "total": s["total"], "n_bytes": got[2] if whole else got,
            "per_cf": got[1] if whole else None, "capped": got[3] if whole else None, "bucket": s, "path": path}


def refusal(sol, limit, bucket, header_len, hi_db):
    """what encode_stream_abr_buffered says of a solve() that is not met: the size at the highest target if that does
    not fit, else the first block above the buffer, its level in whole bytes rounded up, and the buffer"""
    assert not sol["met"]
    total, s = sol["total"], sol["bucket"]
    if total > limit:
        return (f"a body of {limit} bytes cannot be reached: at the highest target, {hi_db:g} dB, it takes {total} bytes "
                f"({header_len + total} with the header), the smallest size this range of targets gives")
    over = s["first_over"]
    level = -(-s["level"][over] // (1 << Q))
    return (f"a buffer of {int(bucket[1])} bytes cannot be met: at the highest target, {hi_db:g} dB, the body fits its "
            f"limit ({total} of {limit} bytes) but block {over} brings the level to {level} bytes, the first block "
            f"above the buffer")
