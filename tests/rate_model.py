"""Coding to a target noise-to-mask ratio, stated in NumPy over the oracle (test helper).

The definition (include/pacx.h, pacx_encode_pack_nmr_batch), for one unit -- a long block or a short sub-block --
on the quantities the constant-rate encoder already has (oracle.pac_oracle.encode_channel: lines X not multiplied by
2^overallScale, the overall scale, the band SMRs; masked_threshold T):

    cap = bit_budget(...) with the cap rate in place of the stream's, J = max(floor(cap / 32), 0)
    ok(B): alloc = bit_alloc(float(B), ...); per band scale_factor + mantissa_vec as encode_channel makes them, then
           dequantize_vec; Xh = dequantised / 2^overall (0 in a band without bits); NMR_b of nmr_model.band_values;
           max_b NMR_b <= target
    not ok(32 J): budget 32 J, capped;  else bisection lo = -1, hi = J on ok(32 mid), budget 32 hi

analysis() does the part that does not depend on target or budgets once per stream; search() and encode() work on it.
"""
import struct

import numpy as np

import nmr_model as nm
from oracle import pac_oracle as po

HOP, SHORT, SUB, STEP = nm.HOP, nm.SHORT, nm.SUB, 32


class Unit:
    """one long block or short sub-block: x (lines), overall, smr, thr, bands, flags, short"""

    def __init__(self, x, overall, smr, thr, bands, flags, short):
        self.x, self.overall, self.smr, self.thr = x, int(overall), smr, thr
        self.bands, self.flags, self.short = bands, flags, short
        self.xs = x * (1 << self.overall)
        self.peak = np.array([np.max(np.abs(self.xs[bands.lowerLine[b]:bands.upperLine[b] + 1]))
                              for b in range(bands.nBands)])


def analysis(pcm, sample_rate, block_switching, n_scale_bits=4, n_mant_size_bits=12):
    """-> dict: p (oracle params), flags per block, dropped per block, units [block][ch] = list of 1 or 8 Unit (None
    for a dropped hop), and the two field widths the stream is coded with"""
    pcm = np.asarray(pcm)
    n_ch = pcm.shape[1]
    p = po.make_params(sample_rate, n_ch, 128, HOP, n_scale_bits, n_mant_size_bits)
    buf = nm.fractions(pcm)
    flags = nm.block_flags(buf, block_switching)
    drop = nm.dropped(buf, flags)
    units = []
    for f, (last_t, cur_t, next_t) in enumerate(flags):
        if drop[f]:
            units.append(None)
            continue
        row = []
        for ch in range(n_ch):
            full = buf[ch, f * HOP:(f + 2) * HOP]
            if not cur_t:
                st = {}
                overall = po.encode_channel(full, p, last_t, cur_t, next_t, stages=st)[3]
                row.append([Unit(st["mdct"], overall, st["smr"], po.masked_threshold(full, HOP, sample_rate), p.sfBands,
                                 (last_t, cur_t, next_t), False)])
                continue
            subs = []
            p.nMDCTLines = p.nSamplesPerBlock = SHORT
            try:
                for sub in nm.sub_blocks(full):
                    st = {}
                    overall = po.encode_channel(sub, p, last_t, cur_t, next_t, stages=st)[3]
                    subs.append(Unit(st["mdct"], overall, st["smr"], po.masked_threshold(sub, SHORT, sample_rate),
                                     p.sfBandsShort, (last_t, cur_t, next_t), True))
            finally:
                p.nMDCTLines = p.nSamplesPerBlock = HOP
            row.append(subs)
        units.append(row)
    return {"p": p, "flags": flags, "dropped": drop, "units": units, "n_ch": n_ch, "sample_rate": sample_rate,
            "n_scale_bits": n_scale_bits, "n_mant_size_bits": n_mant_size_bits}


def widths(a):
    """(nScaleBits, nMantSizeBits) of an analysis"""
    return a.get("n_scale_bits", 4), a.get("n_mant_size_bits", 12)


def code_unit(p, u, budget):
    """(sf, alloc, dense mantissas, overall) of the unit with this BitAlloc budget, and Xh"""
    bands = u.bands
    alloc = po.bit_alloc(float(budget), min(1 << p.nMantSizeBits, 16), bands.nBands, bands.nLines, u.smr)
    sf = np.empty(bands.nBands, dtype=np.int32)
    mant, xh = [], np.zeros(len(u.x))
    for b in range(bands.nBands):
        lo, hi = bands.lowerLine[b], bands.upperLine[b] + 1
        sf[b] = po.scale_factor(u.peak[b], p.nScaleBits, alloc[b])
        if alloc[b]:
            m = po.mantissa_vec(u.xs[lo:hi], sf[b], p.nScaleBits, alloc[b])
            mant.append(m)
            xh[lo:hi] = po.dequantize_vec(sf[b], m, p.nScaleBits, alloc[b])
    mant = np.concatenate(mant).astype(np.int32) if mant else np.zeros(0, np.int32)
    return (sf, alloc, mant, u.overall), xh / (1. * (1 << u.overall))


def worst_nmr(p, u, budget):
    return float(np.max(nm.band_values(u.x, code_unit(p, u, budget)[1], u.thr, u.bands)[2]))


def cap_steps(a, u, max_kbps):
    """J of a unit: the budget rule with the cap rate, in steps of 32 bits"""
    pc = po.make_params(a["sample_rate"], a["n_ch"], max_kbps, HOP, *widths(a))
    if u.short:
        pc.nMDCTLines = pc.nSamplesPerBlock = SHORT
    return max(int(np.floor(po.bit_budget(pc, *u.flags) / STEP)), 0)


def search_unit(a, u, target, max_kbps, trace=None):
    """-> (budget, capped, margin): margin = the smallest |max_b NMR_b - target| over the evaluations made.  trace, if
    a list, receives (budget, worst NMR) of every evaluation in order."""
    p = a["p"]
    margin = np.inf

    def ok(steps):
        nonlocal margin
        w = worst_nmr(p, u, STEP * steps)
        margin = min(margin, abs(w - target))
        if trace is not None:
            trace.append((STEP * steps, w))
        return w <= target

    j = cap_steps(a, u, max_kbps)
    if not ok(j):
        return STEP * j, True, margin
    lo, hi = -1, j
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return STEP * hi, False, margin


def search(a, target, max_kbps):
    """-> budget int32 [blocks, nCh, 8] (0 for dropped hops and unused slots), capped bool [blocks, nCh, 8],
    margin float [blocks, nCh, 8] (inf where there is no unit), live bool [blocks, nCh, 8]"""
    shape = (len(a["flags"]), a["n_ch"], SUB)
    budget, capped = np.zeros(shape, np.int32), np.zeros(shape, bool)
    margin, live = np.full(shape, np.inf), np.zeros(shape, bool)
    for f, row in enumerate(a["units"]):
        if row is None:
            continue
        for ch, us in enumerate(row):
            for j, u in enumerate(us):
                budget[f, ch, j], capped[f, ch, j], margin[f, ch, j] = search_unit(a, u, target, max_kbps)
                live[f, ch, j] = True
    return budget, capped, margin, live


def encode(a, budget, num_samples):
    """the .pac stream of the analysed PCM with these budgets ([blocks, nCh, 8]): pac_header + pack_channel_block"""
    p = a["p"]
    out = [po.pac_header(p, num_samples)]
    for f, row in enumerate(a["units"]):
        if row is None:
            continue
        for ch, us in enumerate(row):
            parts = [code_unit(p, u, budget[f, ch, j])[0] for j, u in enumerate(us)]
            n_bytes, payload = po.pack_channel_block(p, a["flags"][f], parts)
            out.append(struct.pack('<L', int(n_bytes)))
            out.append(payload)
    return b''.join(out)


def kbps_per_channel(a, data):
    """records of the stream (length prefixes included) over the duration of the blocks submitted"""
    recs, _ = nm.records(data)
    body = sum(n + 4 for _, n in recs)
    return 8.0 * body / (len(a["flags"]) * HOP / float(a["sample_rate"])) / a["n_ch"] / 1000.0
