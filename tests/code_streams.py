"""Hand-written code sets as .pac streams: well-formed records no encode of real audio reaches.

The suite's decode tests only ever see what BitAlloc wrote at 96-128 kb/s.  This module DRAWS the codes of every
record -- flags, overall scales, allocations, scale factors, mantissas -- within what the format defines (allocation 0
or 2..min(2^nMantSizeBits, 16), scale factor and overall scale below 2^nScaleBits), writes them with the oracle's own
writer (make_params, pac_header, pack_channel_block, BitWriter) and keeps them in the engine's layout, so that
Encoder.unpack can be compared with them field by field and Encoder.pack / Encoder.decode be fed with them.  Nothing
here is malformed: every case is a file the oracle's decoder takes.

    case(name) -> Case: the file, the records, the codes (see Case)
    decode_float(pac) -> the oracle's decode_stream with the samples BEFORE the PCM quantiser, the peak of the
                         blocks that overlap at every sample, and the blocks

CPU only, seeded, no tests in it (tests/test_code_streams.py, tests/test_gpu_code_streams.py).

Seeds.  A GPU sample may differ from the oracle's by the IMDCT's rounding, 1e-12 of the block peak, and a sample
that close to a step of the 16-bit quantiser would flip a PCM code with nothing wrong.  SEEDS holds, per case, the
first seed from 0 at which no sample of the oracle's output lies within 1e-10 * max(1, peak) of a step (a hundred times
the bar) and at which the case's census holds; test_code_streams asserts both with zero exceptions.
"""
import functools
import struct

import numpy as np

from oracle import pac_oracle as po

HOP, SUB, SHORT = 1024, 8, po.SHORT_LINES

# name -> (hops, channels, sample rate, (nScaleBits, nMantSizeBits), recipe)
SPECS = {
    "mixed":          (6, 2, 48000, (4, 12), "mixed"),
    "flags8":         (8, 1, 48000, (4, 12), "flags8"),
    "max_long":       (3, 1, 48000, (4, 12), "max_long"),
    "max_short":      (3, 1, 48000, (4, 12), "max_short"),
    "max_long_sr32":  (3, 1, 32000, (4, 12), "max_long"),
    "max_short_sr32": (3, 1, 32000, (4, 12), "max_short"),
    "empty_blocks":   (4, 2, 48000, (4, 12), "empty"),
    "empty_one_band": (4, 2, 48000, (4, 12), "one_band"),
    "sign_only":      (4, 2, 48000, (4, 12), "sign_only"),
    "loud":           (4, 2, 48000, (4, 12), "loud"),
    "quiet":          (4, 2, 48000, (4, 12), "quiet"),
    "ch1":            (3, 1, 48000, (4, 12), "random"),
    "ch3":            (3, 3, 48000, (4, 12), "random"),
    "one_hop":        (1, 2, 48000, (4, 12), "random"),
    "no_hops":        (0, 2, 48000, (4, 12), "random"),
    "sr32":           (3, 2, 32000, (4, 12), "random"),
    "sr441":          (3, 2, 44100, (4, 12), "random"),
    "sr96":           (3, 2, 96000, (4, 12), "random"),
    "w3_4":           (4, 2, 48000, (3, 4), "random"),
    "w2_5":           (4, 2, 48000, (2, 5), "random"),
    "w4_16":          (4, 2, 48000, (4, 16), "w4_16"),
}
NAMES = tuple(SPECS)

SEEDS = {name: 0 for name in SPECS}
SEEDS.update({"mixed": 3, "flags8": 1, "loud": 3, "w4_16": 1})           # find_seed(name) of every case


class Case:
    """One stream.  n_cf = hops * channels channel-frames in stream order (hop major).
      pac, header_len     the file and where its body starts
      p                   the oracle's params of the header
      records, sizes      payload bytes of every record and their lengths (int32 [n_cf])
      flags               uint8 [n_cf]: last | cur << 1 | next << 2 of every channel-frame
      frame_flags         uint8 [hops] where the channels of every hop share their flags, else None
      overall             int32 [n_cf, 8], zero beyond entry 0 for a long block
      scale_factor, bit_alloc   int32 [n_cf, band_stride]: a long block's bands, or eight rows of nb_short
      mantissa            int32 [n_cf, 1024], line-indexed (a short frame: eight rows of 128 lines)
    """


def max_alloc(n_mant_size_bits):
    """the largest allocation a size field of that width carries (code + 1), capped at 16"""
    return min(1 << n_mant_size_bits, 16)


def longest_record(sample_rate, widths=(4, 12), short=False):
    """bytes of the record with every band at the largest allocation, by oracle.block_bits and the size rule of
    oracle.pack_channel_block"""
    p = po.make_params(sample_rate, 1, 128, HOP, *widths)
    bands = p.sfBandsShort if short else p.sfBands
    bits = po.block_bits(p, [max_alloc(widths[1])] * bands.nBands, short)
    return int(((SUB if short else 1) * bits + 4 + 7) // 8)


def _draw_unit(rng, bands, n_scale_bits, top, recipe):
    """header codes of one long block / short sub-block -> (overall, alloc [nb], sf [nb])"""
    nb = bands.nBands
    hi = 1 << n_scale_bits
    overall = int(rng.integers(0, hi))
    sf = rng.integers(0, hi, nb)
    alloc = rng.choice(np.concatenate(([0], np.arange(2, top + 1))), nb)
    if recipe in ("max_long", "max_short"):
        alloc[:] = top
    elif recipe in ("empty", "one_band"):
        alloc[:] = 0
    elif recipe == "sign_only":
        alloc = rng.integers(2, top + 1, nb)
    elif recipe == "loud":
        alloc = rng.integers(2, top + 1, nb)
        overall, sf = 0, np.zeros(nb, int)
    elif recipe == "quiet":
        alloc[:] = 2
        overall, sf = hi - 1, np.full(nb, hi - 1)
    return overall, alloc.astype(int), np.asarray(sf).astype(int)


def _draw_mantissas(rng, bands, alloc, n_lines, recipe):
    mant = np.zeros(n_lines, np.int64)
    for b in range(bands.nBands):
        a = int(alloc[b])
        if not a:
            continue
        lo, n = int(bands.lowerLine[b]), int(bands.nLines[b])
        if recipe == "sign_only":
            m = np.full(n, 1 << (a - 1))
        elif recipe == "loud":
            m = ((1 << (a - 1)) - 1) | (rng.integers(0, 2, n) << (a - 1))
        else:
            m = rng.integers(0, 1 << a, n)
        mant[lo:lo + n] = m
    return mant


def _hop_flags(rng, name, recipe, hops, n_ch):
    """uint8 [hops, n_ch]"""
    if recipe == "mixed":
        fl = rng.integers(0, 8, (hops, n_ch))
        fl[0] = (0, 2)                                   # a long and a short block side by side
        return fl.astype(np.uint8)
    if recipe == "flags8":
        one = np.arange(8)
    elif recipe == "max_long":
        one = np.zeros(hops, int)
    elif recipe == "max_short":
        one = np.full(hops, 2)
    elif recipe == "w4_16":
        one = np.array([2, 0, 6, 1])                     # the longest short frame, the longest long block, two drawn
    else:
        one = rng.integers(0, 8, hops)
        if recipe in ("empty", "one_band"):
            one = np.array([0, 2, 5, 3])
        elif hops >= 2:
            one[0] &= ~2                                 # a long and a short frame in every stream of two hops or more
            one[1] |= 2
    return np.repeat(one[:hops, None], n_ch, axis=1).astype(np.uint8)


def _build(name, seed):
    hops, n_ch, sr, (n_scale, n_msb), recipe = SPECS[name]
    rng = np.random.default_rng([seed, NAMES.index(name)])
    p = po.make_params(sr, n_ch, 128, HOP, n_scale, n_msb)
    top = max_alloc(n_msb)
    nb_l, nb_s = p.sfBands.nBands, p.sfBandsShort.nBands
    stride = max(nb_l, SUB * nb_s)
    n_cf = hops * n_ch
    c = Case()
    c.name, c.seed, c.p, c.hops, c.n_ch, c.sample_rate, c.widths = name, seed, p, hops, n_ch, sr, (n_scale, n_msb)
    c.band_stride = stride
    hop_flags = _hop_flags(rng, name, recipe, hops, n_ch)
    c.flags = hop_flags.reshape(-1).copy()
    c.frame_flags = hop_flags[:, 0].copy() if (hop_flags == hop_flags[:, :1]).all() else None
    c.overall = np.zeros((n_cf, SUB), np.int32)
    c.scale_factor = np.zeros((n_cf, stride), np.int32)
    c.bit_alloc = np.zeros((n_cf, stride), np.int32)
    c.mantissa = np.zeros((n_cf, HOP), np.int32)
    c.records, c.parts = [], []
    out = [po.pac_header(p, hops * HOP)]
    c.header_len = len(out[0])
    for cf in range(n_cf):
        fl = int(c.flags[cf])
        cur = (fl >> 1) & 1
        bands, nb, n_lines = (p.sfBandsShort, nb_s, SHORT) if cur else (p.sfBands, nb_l, HOP)
        how = recipe
        if recipe == "w4_16":
            how = ("max_short", "max_long", "random", "random")[cf // n_ch]
        parts = []
        for s in range(SUB if cur else 1):
            overall, alloc, sf = _draw_unit(rng, bands, n_scale, top, how)
            if recipe == "one_band" and s == (cf % SUB if cur else 0):
                alloc[int(rng.integers(0, nb))] = 2          # the whole record codes one band, at two bits
            mant = _draw_mantissas(rng, bands, alloc, n_lines, how)
            c.overall[cf, s] = overall
            c.scale_factor[cf, s * nb:(s + 1) * nb] = sf
            c.bit_alloc[cf, s * nb:(s + 1) * nb] = alloc
            c.mantissa[cf, s * n_lines:(s + 1) * n_lines] = mant
            coded = np.zeros(n_lines, bool)
            for b in np.flatnonzero(alloc):
                coded[bands.lowerLine[b]:bands.upperLine[b] + 1] = True
            parts.append((sf, alloc, mant[coded], overall))
        n_bytes, payload = po.pack_channel_block(p, (fl & 1, cur, (fl >> 2) & 1), parts)
        assert n_bytes == len(payload)
        c.records.append(payload)
        c.parts.append(parts)
        out += [struct.pack("<L", n_bytes), payload]
    c.sizes = np.array([len(r) for r in c.records], np.int32)
    c.pac = b"".join(out)
    return c


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """the case `name` at its fixed seed (SEEDS); another seed only for the search that fixed them"""
    return _build(name, SEEDS[name] if seed is None else seed)


# ------------------------------------------------------------------------------ the oracle's decoder, restated
def decode_float(data):
    """oracle.decode_stream (coder/pacfile.py:231-298) up to, not including, the PCM conversion.
    -> samples float64 [n, nCh] (fraction_to_pcm16 of them is decode_stream's array), peak float64 [n, nCh]: the
    larger max |block| of the two blocks that overlap at the sample (one at the stream's ends), blocks float64
    [n_cf, 2048]: every channel-frame's block before overlap-and-add, short frames assembled from their eight
    sub-blocks at n = 448 + 128 j."""
    p, _, pos = po.parse_header(data)
    n_ch, hop = p.nChannels, p.nMDCTLines
    ola = [np.zeros(hop) for _ in range(n_ch)]
    last_peak = [0.0] * n_ch
    samples, peaks, blocks = [], [], []
    while pos < len(data):
        hop_out, hop_peak = [], []
        for ch in range(n_ch):
            n_bytes = struct.unpack("<L", data[pos:pos + 4])[0]
            br = po.BitReader(data[pos + 4:pos + 4 + n_bytes])
            pos += 4 + n_bytes
            last_t, cur_t, next_t = br.get(1), br.get(1), br.get(1)
            if not cur_t:
                block = po.decode_any_block(p, *po.parse_block_body(br, p, False), last_t, cur_t, next_t)
            else:
                block = np.zeros(2 * hop)
                p.nMDCTLines = p.nSamplesPerBlock = SHORT
                try:
                    pad = hop // 2 - SHORT // 2
                    for n in range(pad, 2 * hop - SHORT - pad, SHORT):
                        block[n:n + 2 * SHORT] += po.decode_block(p, *po.parse_block_body(br, p, True),
                                                                  last_t, cur_t, next_t)
                finally:
                    p.nMDCTLines = p.nSamplesPerBlock = hop
            blocks.append(block)
            pk = float(np.max(np.abs(block)))
            hop_out.append(np.add(ola[ch], block[:hop]))
            hop_peak.append(np.full(hop, max(last_peak[ch], pk)))
            ola[ch], last_peak[ch] = block[hop:], pk
        samples.append(np.stack(hop_out, axis=1))
        peaks.append(np.stack(hop_peak, axis=1))
    samples.append(np.stack(ola, axis=1))
    peaks.append(np.stack([np.full(hop, v) for v in last_peak], axis=1))
    return np.concatenate(samples), np.concatenate(peaks), np.array(blocks).reshape(-1, 2 * hop)


def census(c):
    """what a case's records hold: the sets of allocations, scale factors, overall scales (of the bands and blocks the
    records code), flag values and record lengths mod 4"""
    units = [u for parts in c.parts for u in parts]
    return {"alloc": set(int(a) for (_, alloc, _, _) in units for a in alloc),
            "scale_factor": set(int(v) for (sf, _, _, _) in units for v in sf),
            "overall": set(int(ov) for (_, _, _, ov) in units),
            "flags": set(int(f) for f in c.flags),
            "mod4": set(int(n) % 4 for n in c.sizes)}


def census_complete(c):
    """`mixed` alone: every allocation, scale factor and overall scale of the widths, every alignment"""
    got = census(c)
    n_scale, n_msb = c.widths
    return got["alloc"] == {0} | set(range(2, max_alloc(n_msb) + 1)) and got["mod4"] == {0, 1, 2, 3} and \
        got["scale_factor"] == set(range(1 << n_scale)) == got["overall"]


def find_seed(name, limit=1000):
    """how SEEDS was filled: the first seed without a tie (and, for `mixed`, with the full census)"""
    for seed in range(limit):
        c = _build(name, seed)
        samples, peak, _ = decode_float(c.pac)
        if tie_exceptions(samples, peak) == 0 and (name != "mixed" or census_complete(c)):
            return seed
    raise RuntimeError(f"{name}: no clean seed below {limit}")


def tie_exceptions(samples, peak):
    """samples within 1e-10 * max(1, peak) of a step of the 16-bit quantiser: the count the tie condition wants zero"""
    w = 1e-10 * np.maximum(1.0, peak)
    return int(np.sum(po.fraction_to_pcm16(samples + w) != po.fraction_to_pcm16(samples - w)))
