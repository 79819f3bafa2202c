"""The buffered solve for a stream in chunks (include/pacx_bucket_kept.h: pacx_bucket_scan_targets, pacx_bucket_tree_begin /
pacx_bucket_tree_step) in plain Python integers (test helper), over bucket_model.scan.

    decide()           the one decision of the solves (rate_dev.h, solve_decide) on a dict lo, hi, mid, phase, done, met
    begin(), targets() the state before the first probe; a pass's targets, the heap-ordered nodes of the depth-L tree
    no_hop(), fold()   the scan of no hop; a piece's scan (from the level the scans before it ended at) folded in
    scan_pieces()      bucket_model.scan of a row cut at the given hops, by fold()
    step()             up to L decisions on the scans of a pass's targets, and the probes read on the way
    passes()           ceil((P - 1) / L), P the pairs of the plain solve
    solve()            the whole solve pass by pass: bucket_model.solve's t, met, total, bucket and probes
"""
import bucket_model as bk

FIELDS = bk.FIELDS
LEVELS_MAX, TARGETS = 5, 31


def decide(s, fits):
    """-> the state after the decision that the probe at s["mid"] fits or not"""
    s = dict(s)
    if s["done"]:
        return s
    if s["phase"] == 0:
        if not fits:
            s["done"] = 1
            return s
        s["met"], s["phase"] = 1, 1
    if fits:
        s["hi"] = s["mid"]
    else:
        s["lo"] = s["mid"]
    if s["hi"] - s["lo"] > 1:
        s["mid"] = (s["lo"] + s["hi"]) // 2
    else:
        s["mid"], s["done"] = s["hi"], 1
    return s


def begin(t_lo, t_hi):
    return {"lo": t_lo - 1, "hi": t_hi, "mid": t_hi, "phase": 0, "done": 0, "met": 0}


def targets(s, levels):
    """the 2^levels - 1 targets of the next pass in heap order: slot 0 the state's probe, slots 2k + 1 and 2k + 2 the
    probe after the decision at slot k with fits False / True; a slot below the solve's end repeats the target found"""
    n = (1 << levels) - 1
    node = [None] * n
    node[0] = s
    for k in range(n):
        for fits in (False, True):
            if 2 * k + 1 + fits < n:
                node[2 * k + 1 + fits] = decide(node[k], fits)
    return [v["mid"] for v in node]


def passes(t_lo, t_hi, levels):
    pairs = 2 + (t_hi - t_lo + 1).bit_length()                         # 2 + ceil(log2(t_hi - t_lo + 2))
    return -(-(pairs - 1) // levels)


def no_hop(start):
    return {"total": 0, "peak_q16": start, "peak_hop": -1, "first_over": -1, "end_q16": start}


def fold(acc, piece, hop_off):
    """acc, then a piece scanned from acc["end_q16"], its hops numbered from 0"""
    out = dict(acc)
    out["total"] += piece["total"]
    if piece["peak_hop"] >= 0 and piece["peak_q16"] > acc["peak_q16"]:
        out["peak_q16"], out["peak_hop"] = piece["peak_q16"], piece["peak_hop"] + hop_off
    if acc["first_over"] < 0 and piece["first_over"] >= 0:
        out["first_over"] = piece["first_over"] + hop_off
    out["end_q16"] = piece["end_q16"]
    return out


def scan_pieces(n_bytes, n_ch, bucket, cuts):
    """the scan of a row in the pieces [cuts[i], cuts[i + 1]) of its hops -> the five fields"""
    drain, size, start = (int(v) for v in bucket)
    n_hops = len(n_bytes) // n_ch
    edges = [0] + [int(c) for c in cuts] + [n_hops]
    acc = no_hop(start)
    for a, b in zip(edges[:-1], edges[1:]):
        piece = bk.scan(n_bytes[a * n_ch:b * n_ch], n_ch, (drain, size, acc["end_q16"]))
        acc = fold(acc, piece, a)
    return acc


def step(s, kept, acc, limit, size, levels):
    """acc[k]: the scan of the whole stream at slot k's target.  -> (state, the scan kept, the slots read in order)"""
    k, read = 0, []
    for _ in range(levels):
        if s["done"]:
            break
        fits = acc[k]["total"] <= limit and acc[k]["peak_q16"] <= size << bk.Q
        first = s["phase"] == 0
        read.append(k)
        s = decide(s, fits)
        if fits or first:
            kept = dict(acc[k])
        k = 2 * k + 1 + (1 if fits else 0)
    return s, kept, read


def solve(evaluate, n_ch, limit, bucket, t_lo, t_hi, levels, cuts=()):
    """bucket_model.solve through the tree: evaluate(t) -> n_bytes (or the models' tuple) at the grid target t.
    -> dict t, met, total, bucket (the five fields), path (the targets decided on, in order), passes, evaluated (the
    number of scans taken)"""
    size, start = int(bucket[1]), int(bucket[2])
    s, kept, path, evaluated = begin(t_lo, t_hi), no_hop(start), [], 0
    for _ in range(passes(t_lo, t_hi, levels)):
        tt = targets(s, levels)
        acc = []
        for t in tt:
            got = evaluate(t)
            acc.append(scan_pieces(got[2] if isinstance(got, tuple) else got, n_ch, bucket, cuts))
        evaluated += len(tt)
        s, kept, read = step(s, kept, acc, limit, size, levels)
        path += [tt[k] for k in read]
    assert s["done"]
    return {"t": s["mid"], "met": s["met"], "total": kept["total"], "bucket": kept, "path": path,
            "passes": passes(t_lo, t_hi, levels), "evaluated": evaluated}
