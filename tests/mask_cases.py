"""Blocks built to sit ON the inequalities of the masked-threshold kernels (csrc/k_psy.hip): the masker pruning of the
long side chain, the batch screen and the per-masker chunk screen of k_mask.  NumPy and the oracle only; seeds fixed.

A tone at (fractional) bin k is  a cos(2 pi k (n + 1/2) / N + phi).  cases() returns the records; what each was built
for is DATA in `prop`, asserted from the oracle in tests/test_mask_cases.py and named by the GPU test when it fails.

Families
  a  full peak lists: 512 peaks (the side chain's list holds exactly 8 x 64), all <= 40 dB (every one prunable), all
     above 40 dB (none prunable: eight full masker batches), the int16 rendering (>= 500), the even-bin comb whose last
     peak is bin 1024 (compared with its left neighbour only), a peak at bin 1.
  b  n tones above 40 dB and nothing else that can survive the pruning: every other peak (Hann side lobes, dither) is
     dominated under the loosest reading of the bounds the kernel may use, with 0.01 dB to spare -- so the mask kernel
     walks exactly n maskers, n = 63, 64, 65, 128, 129 (batch edges), whatever the kernel's float estimates are.
     n = 1 cannot be had that way (a masker reaches 27 dB/Bark and the axis is 24.6 Bark long: one tone would have to
     stand 330 dB above the dither): that block has one peak and no other, on floor_block().
  c  dominance margins: delta = S_p - S_q + 27 |z_q - z_p| bisected on p's amplitude to -5e-3, -2e-4, +2e-4, +5e-3 dB,
     p below q / p above q (both <= 40 dB), adjacent in the peak list / >= 64 ordinals apart / p first / p last
     (the last two on floor_block(), where no dither peak can stand before or after p).
     The tones stand where the kernel's bin-wide Bark bounds are tightest (the lower one half way between its two
     bins, the upper one on its bin): bound_slack() says how far the kernel is from dropping p at delta = 0.
     (p above q and >= 64 ordinals apart cannot be made visible: 64 peaks span >= 0.4 Bark only above 15 kHz, where
     the threshold in quiet lies 30 dB and more above any masker of 40 dB.)
  d  chunk-screen edges: one tone plus dither, amplitude bisected until the threshold exceeds the threshold in quiet
     in one chunk of 64 lines ONLY at its first (last) line, by eps = 1e-4, 5e-3, 2e-2 dB, and mirror cases that stay
     eps below it; below the masker at a chunk's last line (quiet flat) and first line (13.8 kHz, where quiet rises
     faster than 27 dB/Bark), above the masker at a chunk's first line, and in a short sub-block (2 chunks).
     (Above a masker only a chunk's FIRST line can be the only one: from line 63 on the threshold in quiet falls by
     less than 0.4 dB/Bark, which only the curve of a masker above 112 dB follows, 90 dB higher up.)
  e  loud maskers (float64 only): above 113.6 dB the upper slope is positive; alone, and in one batch with quiet ones.
  f  short frames: a sub-block with 64 peaks, silent sub-blocks, a one-tone sub-block, all in one frame; a silent
     long frame.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import pac_oracle as po

SR = 44100
N_LONG, N_SHORT = 2048, 256
DELTAS = (-5e-3, -2e-4, 2e-4, 5e-3)
EPSILONS = (1e-4, 5e-3, 2e-2)
BATCH_NS = (63, 64, 65, 128, 129)      # and 1, built apart
SPL_BAND = 2e-3      # the kernel's float SPL estimate lies within 1e-3 dB of the exact one and is widened by 1e-3 dB
BARK_MARGIN = 1e-9
SPARE = 0.01


def tone(k, a, phi=0.0, n=N_LONG):
    return a * np.cos(2.0 * np.pi * k * (np.arange(n) + 0.5) / n + phi)


def sub_block(frame, sb):
    return frame[448 + 128 * sb:448 + 128 * sb + N_SHORT]


def peak_bins(inten):
    """bins the reference's peak picker takes: strict local maxima of inten[1:], the last one against its left only"""
    up = inten[1:] > inten[:-1]
    down = np.append(inten[1:-1] > inten[2:], True)
    return np.nonzero(up & down)[0] + 1


def analyse(x, sr):
    """the oracle's view of one block: intensities, peak bins, peak frequencies, SPLs and Bark values"""
    inten = po.sidechain_intensity(np.asarray(x, dtype=np.float64))
    freqs = np.fft.rfftfreq(len(x), d=1 / sr)
    f, spl = po.find_peaks(inten, freqs)
    f, spl = np.array(f, dtype=np.float64), np.array(spl, dtype=np.float64)
    bins = peak_bins(inten)
    assert len(bins) == len(f)
    return SimpleNamespace(inten=inten, bins=bins, f=f, spl=spl, z=po.bark_of(f), freqs=freqs)


def one_peak(inten, freqs, b):
    """find_peaks' frequency and SPL of the peak at bin b (the same operations on the same two bins)"""
    pair = inten[b - 1:b + 1]
    return np.sum(freqs[b - 1:b + 1] * pair) / np.sum(pair), float(po.spl_of(np.sum(pair)))


# ------------------------------------------------------------------ what the kernel may drop
def pruning_partition(an, sr):
    """What a long side chain MAY drop, stated on the oracle's numbers.  A masker p of at most 40 dB may go when
    another masker q has S_q - S_p >= 27 |z_q - z_p|: q's curve is then nowhere below p's.  The kernel decides on
    bounds -- S within SPL_BAND, z between the Bark values of the masker's two bins +- BARK_MARGIN -- so for every
    peak this returns
      dropped[p]: dominated even with every bound read against it, SPARE to spare: it is dropped for certain;
      kept[p]:    above 40 dB, or not dominated even with every bound read in its favour by SPARE: kept for certain.
    A peak in neither set is the kernel's to decide."""
    n = len(an.freqs)
    zb = po.bark_of(np.arange(n) * (sr / (2.0 * (n - 1))))
    zlo, zhi = zb[an.bins - 1] - BARK_MARGIN, zb[an.bins] + BARK_MARGIN
    s = an.spl
    gap_wide = np.where(an.bins[None, :] < an.bins[:, None], zhi[:, None] - zlo[None, :], zhi[None, :] - zlo[:, None])
    gap_tight = np.abs(an.z[:, None] - an.z[None, :])
    off = ~np.eye(len(s), dtype=bool)
    worst = np.max(np.where(off, (s[None, :] - SPL_BAND) - 27.0 * gap_wide, -np.inf), axis=1, initial=-np.inf)
    best = np.max(np.where(off, (s[None, :] + SPL_BAND) - 27.0 * gap_tight, -np.inf), axis=1, initial=-np.inf)
    dropped = (s + SPL_BAND + SPARE <= 40.0) & (worst >= s + SPL_BAND + SPARE)
    kept = (s > 40.0) | (best < s - SPL_BAND - SPARE)
    return dropped, kept


def threshold(an, n_lines, sr, without=()):
    """the oracle's masked threshold from an analysed block, the maskers with ordinals `without` left out"""
    z, quiet = line_tables(n_lines, sr)
    curves = [po.masker_curve_spl(f, s, z) for i, (f, s) in enumerate(zip(an.f, an.spl)) if i not in without]
    return np.amax(curves + [quiet], axis=0)


def ordinal(an, b):
    """where the peak at bin b stands in the peak list"""
    (at,) = np.nonzero(an.bins == b)[0]
    return int(at)


def bound_slack(an, sr, p):
    """How far the bounds are from proving peak p dominated, in dB: the kernel's rule with exact SPLs and the Bark
    values of the maskers' bins.  The bounds are a bin wide each (27 dB/Bark x the Bark width of ~half a bin of p and
    of q at best: 0.2 dB at 14 kHz, 0.45 dB at 4 kHz, 5 dB at 200 Hz), so a peak with delta = 0 is this far from being
    dropped, and an error in the rule shows in the threshold once it exceeds the slack."""
    n = len(an.freqs)
    zb = po.bark_of(np.arange(n) * (sr / (2.0 * (n - 1))))
    zlo, zhi = zb[an.bins - 1], zb[an.bins]
    reach = an.spl - 27.0 * np.where(an.bins < an.bins[p], zhi[p] - zlo, zhi - zlo[p])
    reach[p] = -np.inf
    return an.spl[p] - np.max(reach)


def delta_of(an, p, q):
    """S_p - S_q + 27 |z_q - z_p| of peak ordinals p, q: positive, and p's curve passes q's somewhere"""
    return an.spl[p] - an.spl[q] + 27.0 * abs(an.z[q] - an.z[p])


# ------------------------------------------------------------------ records
def record(name, family, x, sr=SR, short=False, i16=False, **prop):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape == (N_LONG,)
    return SimpleNamespace(name=name, family=family, x=x, sr=sr, short=short, i16=i16, prop=prop)


def as_int16(x):
    return np.rint(x * 32768.0).astype(np.int16)


def rendered(case):
    """the block as the int16 path sees it: rounded codes back as fractions"""
    return po.pcm16_to_fraction(as_int16(case.x))


def blocks_of(case, x=None):
    """the blocks the side chain analyses: the long block, or the eight sub-blocks of a short frame"""
    x = case.x if x is None else x
    return [sub_block(x, sb) for sb in range(8)] if case.short else [x]


def bisect(fn, lo, hi, target, turns=80):
    """fn increasing on [lo, hi]: the argument at which it takes `target`"""
    assert fn(lo) < target < fn(hi), (fn(lo), target, fn(hi))
    for _ in range(turns):
        mid = 0.5 * (lo + hi)
        if fn(mid) < target:
            lo = mid
        else:
            hi = mid
    return hi


# ------------------------------------------------------------------ a: full peak lists
def comb(bins, level, seed, dither, n=N_LONG, own_phase=()):
    rng = np.random.default_rng(seed)
    x = dither * rng.standard_normal(n)
    for k in bins:
        phi = np.pi * (k // 2) if k not in own_phase else 0.25 * np.pi
        x += tone(k, level * (1.0 + 0.2 * rng.random()), phi, n)
    return x


def family_a():
    odd, even = range(1, 1024, 2), range(2, 1025, 2)
    low = comb(odd, 0.0008, 15, 1e-6)
    return [
        record("a_full_low", "a", low, n_peaks=512, first_bin=1, last_bin=1023, all_below_40=True),
        record("a_full_high", "a", comb(odd, 0.008, 12, 1e-6), n_peaks=512, first_bin=1, last_bin=1023,
               all_below_40=False),
        record("a_full_i16", "a", low, i16=True, n_peaks_min=500),
        record("a_full_even", "a", comb(even, 0.0008, 13, 1e-6, own_phase=(1024,)), n_peaks=512, first_bin=2,
               last_bin=1024, all_below_40=True),
    ]


# ------------------------------------------------------------------ b: batch edges
def spread_bins(n, sr):
    """n tone positions (fractional bins) from bin 2.3 up, no two closer than 6 bins or than an equal share of the
    Bark axis: every bin then has a tone within 3 bins or half a share"""
    k = np.arange(2.3, 1021.0, 0.01)
    z = po.bark_of(k * sr / N_LONG)

    def count(share):
        dens = np.minimum(1.0 / 6.0, np.gradient(z, k) / share)
        return np.concatenate(([0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(k))))

    lo, hi = 0.01, 10.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if count(mid)[-1] > n - 0.5:
            lo = mid
        else:
            hi = mid
    c = count(hi)
    return np.interp(np.arange(n) * (c[-1] / (n - 0.5)), c, k)


def family_b():
    out = []
    for n in BATCH_NS:
        rng = np.random.default_rng(200 + n)
        x = 1e-5 * rng.standard_normal(N_LONG)
        for k in spread_bins(n, SR):
            x += tone(k, 0.0062 * (1.0 + 0.1 * rng.random()), rng.uniform(0, 2 * np.pi))
        out.append(record(f"b_kept_{n}", "b", x, i16=True, n_kept=n))
    # n = 1: no dither can be dominated over 24.6 Bark by one tone, so the block has no other peak at all
    out.insert(0, record("b_kept_1", "b", floor_block(0.005) + tone(200, 0.02, 0.3), n_kept=1, n_peaks=1))
    return out


# ------------------------------------------------------------------ what the blocks stand on
def dither(seed, level=1e-5, n=N_LONG):
    return level * np.random.default_rng(seed).standard_normal(n)


def floor_block(level, fillers=(), filler_level=0.0):
    """A block WITHOUT peaks to build on where the peak list itself is the point: level * exp(-|n - centre|) has a
    spectrum that falls strictly from bin 0 to bin 1024 (about 1/k^4, every step signal-decided), and a tone on an
    integer bin occupies exactly three bins under the Hann window -- no side lobes.  So the peaks of such a block are
    the tones put on it and nothing else; `fillers` are integer bins that get a quiet tone each, to fill the list."""
    x = level * np.exp(-np.abs(np.arange(N_LONG) - 1023.5))
    for i, k in enumerate(fillers):
        x += tone(k, filler_level * (1.0 + 0.05 * (i % 7)), 0.37 * i)
    return x


# ------------------------------------------------------------------ c: dominance margins
def dominance_cases(tag, sr, base, kq, aq, kp, deltas=DELTAS, **extra):
    freqs = np.fft.rfftfreq(N_LONG, d=1 / sr)

    def block(ap):
        return base + tone(kq, aq, 0.3) + tone(kp, ap, 1.1)

    def near(inten, k):
        lo = int(np.floor(k))
        return lo + int(np.argmax(inten[lo:lo + 2]))

    def delta(ap):
        inten = po.sidechain_intensity(block(ap))
        bp, bq = near(inten, kp), near(inten, kq)
        (fq, sq), (fp, sp) = one_peak(inten, freqs, bq), one_peak(inten, freqs, bp)
        return sp - sq + 27.0 * abs(po.bark_of(fq) - po.bark_of(fp)), bp, bq

    out = []
    for d in deltas:
        ap = bisect(lambda a: delta(a)[0], aq * 1e-7, aq, d)
        _, bp, bq = delta(ap)
        out.append(record(f"c_{tag}_{d:+.0e}", "c", block(ap), sr=sr, delta=d, p_bin=bp, q_bin=bq, **extra))
    return out


def family_c():
    """apart: least distance of p and q in the peak list; p_ordinal: where p stands in it (-1: last)"""
    out = []
    out += dominance_cases("below_adjacent", SR, dither(31), 200.4, 0.0025, 194.51, apart=1)
    out += dominance_cases("above_adjacent", SR, dither(32), 199.51, 0.0016, 205.4, apart=1)
    out += dominance_cases("below_far", SR, dither(33), 640.4, 0.6, 379.51, apart=64)
    out += dominance_cases("p_first", SR, floor_block(0.05, range(24, 400, 4), 2e-4), 14, 0.0213, 10, apart=1,
                           p_ordinal=0)
    out += dominance_cases("p_last", SR, floor_block(0.005, range(20, 280, 4), 2e-4), 286, 0.0016, 300, apart=1,
                           p_ordinal=-1)
    out += dominance_cases("below_adjacent_48k", 48000, dither(36), 200.4, 0.0025, 194.51, deltas=(-2e-4, 2e-4),
                           apart=1)
    return out


# ------------------------------------------------------------------ d: chunk-screen edges
def line_tables(n_lines, sr):
    f = (sr / (2.0 * n_lines)) * (np.arange(n_lines) + 0.5)
    return po.bark_of(f), po.thresh_quiet(f.copy())


def tone_block(n, k, a, seed):
    rng = np.random.default_rng(seed)
    return 1e-5 * rng.standard_normal(n) + tone(k, a, 0.7, n)


def tone_excess(x, sr, k):
    """masker curve of the tone at bin ~k minus the threshold in quiet, per line"""
    n = len(x)
    inten = po.sidechain_intensity(x)
    freqs = np.fft.rfftfreq(n, d=1 / sr)
    b = int(np.floor(k)) + int(np.argmax(inten[int(np.floor(k)):int(np.floor(k)) + 2]))
    f, spl = one_peak(inten, freqs, b)
    z, quiet = line_tables(n // 2, sr)
    return po.masker_curve_spl(f, spl, z) - quiet, b


def screen_cases(tag, sr, k, line, seed, short=False, epsilons=EPSILONS, lo=1e-4, hi=0.9):
    n = N_SHORT if short else N_LONG
    out = []
    for eps in epsilons:
        for sign in (1.0, -1.0):
            a = bisect(lambda v: tone_excess(tone_block(n, k, v, seed), sr, k)[0][line], lo, hi, sign * eps)
            x = tone_block(n, k, a, seed)
            frame = x
            if short:
                frame = np.zeros(N_LONG)
                frame[448:448 + N_SHORT] = x
            out.append(record(f"d_{tag}_{sign * eps:+.0e}", "d", frame, sr=sr, short=short, eps=sign * eps,
                              line=line, chunk=line // 64, tone_bin=tone_excess(x, sr, k)[1], sub_block=0))
    return out


def family_d():
    out = []
    out += screen_cases("below_last", SR, 180.3, 127, 41)
    out += screen_cases("below_first", SR, 760.3, 640, 42)
    out += screen_cases("above_first", SR, 120.3, 192, 43)
    out += screen_cases("short_above_first", SR, 20.3, 64, 44, short=True)
    out += screen_cases("above_first_48k", 48000, 120.3, 192, 45, epsilons=(5e-3,))
    return out


# ------------------------------------------------------------------ e: loud maskers
def family_e():
    rng = np.random.default_rng(51)
    alone = 1e-3 * rng.standard_normal(N_LONG) + tone(200.3, 12.0, 0.4)
    mixed = 1e-3 * rng.standard_normal(N_LONG) + tone(20.3, 12.0, 0.4)
    for i, k in enumerate((45.4, 70.3, 110.6, 160.2, 230.7)):
        mixed += tone(k, 0.004 * (1 + i), 0.9 * i)
    return [record("e_loud_alone", "e", alone, loud_bin=200, min_spl=113.6),
            record("e_loud_in_batch", "e", mixed, loud_bin=20, min_spl=113.6, quiet_tones=5)]


# ------------------------------------------------------------------ f: short frames, silence
def family_f():
    rng = np.random.default_rng(61)
    frame = np.zeros(N_LONG)
    full = comb(range(1, 128, 2), 0.004, 64, 1e-5, n=N_SHORT)
    frame[448:448 + N_SHORT] = full                              # sub-block 0 full, 1 its second half + dither
    frame[448 + N_SHORT:448 + N_SHORT + 128] = 1e-5 * rng.standard_normal(128)
    lone = 1e-5 * rng.standard_normal(N_SHORT) + tone(30.3, 0.1, 0.2, N_SHORT)
    frame[448 + 128 * 5:448 + 128 * 5 + N_SHORT] = lone          # 3 and 7 silent, 5 one tone, 4 and 6 its halves
    return [record("f_short_mixed", "f", frame, short=True, i16=True, full_sub_block=0, silent_sub_blocks=(3, 7),
                   tone_sub_block=5),
            record("f_long_silent", "f", np.zeros(N_LONG), i16=True, n_peaks=0)]


@functools.lru_cache(maxsize=None)
def cases():
    out = family_a() + family_b() + family_c() + family_d() + family_e() + family_f()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def planted(case):
    """[(what, MDCT line)] of the places a case was built around, for the message of a failing comparison (bin b of
    the side chain's FFT lies between lines b - 1 and b)"""
    at = []
    for key in ("p_bin", "q_bin", "tone_bin", "loud_bin", "first_bin", "last_bin"):
        if key in case.prop:
            b = case.prop[key]
            at.append((f"{key} {case.prop[key]}", min(b, (128 if case.short else 1024) - 1)))
    if "line" in case.prop:
        at.append((f"chunk {case.prop['chunk']} crossing, eps {case.prop['eps']:+.0e}", case.prop["line"]))
    return at


def nearest_planted(case, line):
    at = planted(case)
    if not at:
        return f"{case.name}: line {line}; built for {case.prop}"
    what, where = min(at, key=lambda t: abs(t[1] - line))
    return f"{case.name}: line {line}, nearest planted: {what} at line {where}; built for {case.prop}"


def by_name(name):
    return next(c for c in cases() if c.name == name)
