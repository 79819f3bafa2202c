"""Bits handed to the bands one by one against a noise-to-mask target, stated in NumPy over rate_model (test helper).

The definition (include/pacx.h, pacx_band_curve_batch / pacx_band_pick / pacx_band_solve /
pacx_encode_pack_alloc_batch).  Units, cap and J are rate_model's.

  Candidates: i = 0 ... 15 means bits(i) = 0 for i = 0, else i + 1; n_cand = maxMantBits = min(2^nMantSizeBits, 16).
  The curve, per unit and band b:
    nmr[b][i] = NMR_b (nmr_model.band_values) with band b coded at bits(i): po.scale_factor of the band's maximum,
                po.mantissa_vec -> po.dequantize_vec -> / 2^overall (Xh = 0 for 0 bits); +inf for i >= n_cand
    cap       = 32 J (rate_model.cap_steps);  cap_alloc = po.bit_alloc(float(32 J), ...)
  Arrays: nmr [n_cf, band_stride, 16] (slot sb * nb + b, NaN where there is no band), cap [n_cf, 8] (-1 where there is
  no unit), cap_alloc [n_cf, band_stride].

  pick(unit, T): a_b = bits(i*), i* the first i in ascending order with nmr[b][i] <= T; none (or NaN): bits(n_cand - 1),
    the band missed.  Any band missed or sum_b a_b lines_b > cap: capped; a capped unit whose sum exceeds cap takes
    cap_alloc, one whose sum fits keeps its a_b.
  bits(unit) = nScaleBits + sum_b (nMantSizeBits + nScaleBits + a_b lines_b)
  bytes(cf, T) = 0 for a dropped hop, else ((sum of bits(unit)) + 4 + 7) >> 3;  total(T) = sum of (bytes + 4), bytes > 0
  The solve is abr_model.solve's decision with this total.

curve() needs the analysis of rate_model; pick / frame / evaluate / total / solve / margins work on the arrays alone
(the GPU's included: with_arrays()); encode() codes the analysed PCM with an allocation.
"""
import struct

import numpy as np

import nmr_model as nm
import rate_model as rm
from oracle import pac_oracle as po

SUB, GRID, CAND = rm.SUB, 64, 16
PAYLOAD_STRIDE = 2192


def bits_of(i):
    return 0 if i == 0 else i + 1


BITS = np.array([bits_of(i) for i in range(CAND)])


def max_mant(p):
    return min(1 << p.nMantSizeBits, 16)


def unit_curve(p, u):
    """nmr [nBands, 16] of one unit"""
    bands, n_cand = u.bands, max_mant(p)
    out = np.full((bands.nBands, CAND), np.inf)
    for i in range(n_cand):
        bits = bits_of(i)
        xh = np.zeros(len(u.x))
        if bits:
            for b in range(bands.nBands):
                lo, hi = bands.lowerLine[b], bands.upperLine[b] + 1
                sf = po.scale_factor(u.peak[b], p.nScaleBits, bits)
                xh[lo:hi] = po.dequantize_vec(sf, po.mantissa_vec(u.xs[lo:hi], sf, p.nScaleBits, bits), p.nScaleBits, bits)
        out[:, i] = nm.band_values(u.x, xh / (1. * (1 << u.overall)), u.thr, bands)[2]
    return out


def tables(p):
    """what the array functions need beside the arrays"""
    return {"lines_long": np.asarray(p.sfBands.nLines, np.int64), "lines_short": np.asarray(p.sfBandsShort.nLines, np.int64),
            "n_scale_bits": p.nScaleBits, "n_mant_size_bits": p.nMantSizeBits, "n_cand": max_mant(p),
            "band_stride": max(p.sfBands.nBands, SUB * p.sfBandsShort.nBands)}


def curve(a, max_kbps):
    """-> dict nmr, cap, cap_alloc and tables()"""
    p, n_ch = a["p"], a["n_ch"]
    c = tables(p)
    n_cf = len(a["flags"]) * n_ch
    c["nmr"] = np.full((n_cf, c["band_stride"], CAND), np.nan)
    c["cap"] = np.full((n_cf, SUB), -1, np.int32)
    c["cap_alloc"] = np.zeros((n_cf, c["band_stride"]), np.int32)
    for f, units in enumerate(a["units"]):
        if units is None:
            continue
        for ch, us in enumerate(units):
            cf = f * n_ch + ch
            for sb, u in enumerate(us):
                nb = u.bands.nBands
                J = rm.cap_steps(a, u, max_kbps)
                c["cap"][cf, sb] = rm.STEP * J
                c["nmr"][cf, sb * nb:(sb + 1) * nb] = unit_curve(p, u)
                c["cap_alloc"][cf, sb * nb:(sb + 1) * nb] = po.bit_alloc(float(rm.STEP * J), max_mant(p), nb,
                                                                         u.bands.nLines, u.smr)
    return c


def with_arrays(c, nmr, cap, cap_alloc):
    """the same tables with other arrays (the GPU's)"""
    d = dict(c)
    d["nmr"], d["cap"], d["cap_alloc"] = np.asarray(nmr), np.asarray(cap), np.asarray(cap_alloc)
    return d


def layout(c):
    """(unit [n_cf, band_stride]: the sub-block of every band slot, -1 where no live unit has one; lines of the slot)"""
    cap = np.asarray(c["cap"])
    n_cf, stride = len(cap), c["band_stride"]
    nbl, nbs = len(c["lines_long"]), len(c["lines_short"])
    slot = np.arange(stride)
    short = cap[:, 1] >= 0 if n_cf else np.zeros(0, bool)
    unit_s = np.where(slot < SUB * nbs, slot // nbs, -1)
    lines_s = np.where(slot < SUB * nbs, np.tile(c["lines_short"], SUB + stride)[:stride], 0)
    unit_l = np.where(slot < nbl, 0, -1)
    lines_l = np.zeros(stride, np.int64)
    lines_l[:nbl] = c["lines_long"]
    unit = np.where(short[:, None], unit_s[None, :], unit_l[None, :])
    lines = np.where(short[:, None], lines_s[None, :], lines_l[None, :])
    live = (unit >= 0) & (np.take_along_axis(cap, np.maximum(unit, 0), axis=1) >= 0)
    return np.where(live, unit, -1), np.where(live, lines, 0)


def pick(nmr, lines, cap, cap_alloc, T, n_cand):
    """one unit: nmr [nb, 16], lines [nb], cap, cap_alloc [nb] -> (alloc [nb], capped, missed, over)"""
    a, missed = np.zeros(len(nmr), np.int64), False
    for b, row in enumerate(nmr):
        for i in range(n_cand):                              # ascending: the first pass, not a bisection's
            if row[i] <= T:
                a[b] = bits_of(i)
                break
        else:
            a[b], missed = bits_of(n_cand - 1), True
    over = int(np.sum(a * lines)) > cap
    if over:
        a = np.asarray(cap_alloc, np.int64).copy()
    return a, bool(missed or over), missed, over


def frame(c, cf, T):
    """one channel-frame, unit by unit -> (bit_alloc [band_stride], bytes, capped)"""
    unit, lines = layout(c)
    alloc, total, capped, units = np.zeros(c["band_stride"], np.int32), 0, False, 0
    for sb in range(SUB):
        if c["cap"][cf, sb] < 0:
            continue
        at = np.nonzero(unit[cf] == sb)[0]
        a, cap, _, _ = pick(c["nmr"][cf, at], lines[cf, at], int(c["cap"][cf, sb]), c["cap_alloc"][cf, at], T, c["n_cand"])
        alloc[at] = a
        total += c["n_scale_bits"] + int(np.sum(c["n_mant_size_bits"] + c["n_scale_bits"] + a * lines[cf, at]))
        capped, units = capped or cap, units + 1
    return alloc, ((total + 4 + 7) >> 3) if units else 0, capped


def evaluate(c, t, detail=False):
    """every channel-frame at T = t / 64, all bands at once: -> (total, bit_alloc [n_cf, band_stride], n_bytes [n_cf],
    capped [n_cf]); detail: also missed, over [n_cf, 8] per unit"""
    T = t / GRID
    nmr, cap = np.asarray(c["nmr"]), np.asarray(c["cap"]).astype(np.int64)
    n_cf, n_cand = len(cap), c["n_cand"]
    unit, lines = layout(c)
    live = unit >= 0
    with np.errstate(invalid="ignore"):
        ok = nmr[:, :, :n_cand] <= T
    hit = ok.any(axis=2)
    a = np.where(hit, BITS[np.argmax(ok, axis=2)], bits_of(n_cand - 1))
    a = np.where(live, a, 0)
    missed, over = np.zeros((n_cf, SUB), bool), np.zeros((n_cf, SUB), bool)
    for sb in range(SUB):
        mine = unit == sb
        missed[:, sb] = (mine & ~hit).any(axis=1)
        over[:, sb] = (np.sum(np.where(mine, a * lines, 0), axis=1) > cap[:, sb]) & (cap[:, sb] >= 0)
        a = np.where(mine & over[:, sb][:, None], np.asarray(c["cap_alloc"]), a)
    units = (cap >= 0).sum(axis=1)
    bits = np.sum(np.where(live, c["n_mant_size_bits"] + c["n_scale_bits"] + a * lines, 0), axis=1) + \
        units * c["n_scale_bits"]
    n_bytes = np.where(units > 0, (bits + 4 + 7) >> 3, 0)
    out = (int(np.sum(n_bytes[n_bytes > 0] + 4)), a.astype(np.int32), n_bytes.astype(np.int32),
           (missed | over).any(axis=1))
    return out + (missed, over) if detail else out


def total(c, t):
    return evaluate(c, t)[0]


def total_slow(c, t):
    n = [frame(c, cf, t / GRID)[1] for cf in range(len(c["cap"]))]
    return sum(b + 4 for b in n if b > 0)


def solve(c, limit, t_lo=-30 * GRID, t_hi=30 * GRID):
    """abr_model.solve's decision on this total -> dict t, met, total, bit_alloc, n_bytes, capped, path"""
    path = [(t_hi, total(c, t_hi))]
    if path[0][1] > limit:
        t, met = t_hi, 0
    else:
        lo, hi, met = t_lo - 1, t_hi, 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            path.append((mid, total(c, mid)))
            if path[-1][1] <= limit:
                hi = mid
            else:
                lo = mid
        t = hi
    tot, alloc, n_bytes, capped = evaluate(c, t)
    return {"t": t, "met": met, "total": tot, "bit_alloc": alloc, "n_bytes": n_bytes, "capped": capped, "path": path}


def margins(c, T):
    """[n_cf, 8]: the smallest |nmr - T| over the bands and candidates of every unit, inf where there is none"""
    unit, _ = layout(c)
    d = np.abs(np.asarray(c["nmr"])[:, :, :c["n_cand"]] - T)
    d = np.where(np.isnan(d), np.inf, d).min(axis=2)
    out = np.full((len(unit), SUB), np.inf)
    for sb in range(SUB):
        out[:, sb] = np.where(unit == sb, d, np.inf).min(axis=1)
    return out


def sanitise(c, alloc):
    """a caller's allocation as it is coded: below 2 -> 0, above maxMantBits -> maxMantBits"""
    a = np.asarray(alloc).astype(np.int64)
    return np.where(a < 2, 0, np.minimum(a, c["n_cand"])).astype(np.int32)


def code_unit(p, u, alloc):
    """(sf, alloc, dense mantissas, overall) of the unit with this allocation"""
    bands = u.bands
    alloc = [int(v) for v in alloc]                        # Python ints: 2 ** (15 + 16) must not wrap in an int32
    sf, mant = np.empty(bands.nBands, dtype=np.int32), []
    for b in range(bands.nBands):
        lo, hi = bands.lowerLine[b], bands.upperLine[b] + 1
        sf[b] = po.scale_factor(u.peak[b], p.nScaleBits, alloc[b])
        if alloc[b]:
            mant.append(po.mantissa_vec(u.xs[lo:hi], sf[b], p.nScaleBits, alloc[b]))
    mant = np.concatenate(mant).astype(np.int32) if mant else np.zeros(0, np.int32)
    return sf, np.asarray(alloc, dtype=int), mant, u.overall


def encode(a, alloc, num_samples):
    """the .pac stream of the analysed PCM with this allocation ([n_cf, band_stride], sanitised here); a record that
    would leave its slot of PAYLOAD_STRIDE bytes is coded without mantissa bits"""
    p, n_ch = a["p"], a["n_ch"]
    alloc = sanitise(tables(p), alloc)
    out = [po.pac_header(p, num_samples)]
    for f, row in enumerate(a["units"]):
        if row is None:
            continue
        for ch, us in enumerate(row):
            mine = alloc[f * n_ch + ch]
            nb = us[0].bands.nBands
            parts = [code_unit(p, u, mine[j * nb:(j + 1) * nb]) for j, u in enumerate(us)]
            n_bytes, payload = po.pack_channel_block(p, a["flags"][f], parts)
            if n_bytes > PAYLOAD_STRIDE:
                parts = [code_unit(p, u, np.zeros(nb, np.int32)) for u in us]
                n_bytes, payload = po.pack_channel_block(p, a["flags"][f], parts)
            out.append(struct.pack('<L', int(n_bytes)))
            out.append(payload)
    return b''.join(out)


def synthetic(n_cf, seed, sample_rate=44100, p_short=0.3, p_drop=0.1, p_nan=0.02, p_dead=0.01, cap_scale=1.0):
    """a curve no encoder made, on the band tables of a sample rate: mixed long / short / dropped channel-frames; rows
    that fall from about +30 to -60 dB over the sizes under +-5 dB of noise (so some rise somewhere), a few NaN and a
    few rows of nothing but NaN (bands that miss every target); caps
    around cap_scale x what 9 bits a line would take; random cap_alloc within the cap"""
    rng = np.random.default_rng(seed)
    c = tables(po.make_params(sample_rate, 1, 128))
    nbl, nbs, stride = len(c["lines_long"]), len(c["lines_short"]), c["band_stride"]
    c["nmr"] = np.full((n_cf, stride, CAND), np.nan)
    c["cap"] = np.full((n_cf, SUB), -1, np.int32)
    c["cap_alloc"] = np.zeros((n_cf, stride), np.int32)
    kind = rng.choice(3, n_cf, p=[1 - p_short - p_drop, p_short, p_drop])
    for cf in range(n_cf):
        if kind[cf] == 2:
            continue
        nb, lines = (nbs, c["lines_short"]) if kind[cf] == 1 else (nbl, c["lines_long"])
        for sb in range(SUB if kind[cf] == 1 else 1):
            rows = 30.0 - 6.0 * np.arange(CAND)[None, :] + rng.uniform(-20, 10, (nb, 1)) + rng.uniform(-5, 5, (nb, CAND))
            rows[rng.random((nb, CAND)) < p_nan] = np.nan
            rows[rng.random(nb) < p_dead] = np.nan
            rows[:, c["n_cand"]:] = np.inf
            c["nmr"][cf, sb * nb:(sb + 1) * nb] = rows
            cap = 32 * int(cap_scale * rng.uniform(0.5, 1.5) * 9 * lines.sum() / 32)
            c["cap"][cf, sb] = cap
            ca = rng.integers(0, 8, nb)
            ca = np.where(ca < 2, 0, ca)
            while np.sum(ca * lines) > cap and ca.any():
                ca[np.argmax(ca)] = 0
            c["cap_alloc"][cf, sb * nb:(sb + 1) * nb] = ca
    return c
