"""The noise-to-mask ratio of a .pac stream, stated in NumPy over the oracle (test helper).

Definition (include/pacx.h, pacx_nmr_batch), for one coded block -- 1024 lines and the long band table, or a
128-line sub-block and the short table:
    X   = MDCT lines of the original block with the window its flags select (not times 2^overallScale)
    Xh  = the lines the decoder hands to the IMDCT: dequantised, after the SBR reconstruction, / 2^overallScale
    T   = getMaskedThreshold of the original block, dB SPL
    n   = 4 (X - Xh)^2,  m = 10^((T - 96) / 10)
    NMR_b = 10 log10((mean_b n + eps) / mean_b m),  eps = 2^-52
Lines beyond the last band are ignored; slots no band uses and blocks without a payload are NaN.

Also the hop-to-record map of the reference's writer: which of the n + 2 blocks the driver submits for n hops
(every hop, the last hop again, Close) reach the file.
"""
import struct

import numpy as np

from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv

HOP, SHORT, SUB = 1024, 128, 8
EPS = 2.0 ** -52


def fractions(pcm):
    """[nCh, (n_hops + 3) * HOP] signed fractions: zeros, the hops, the last hop again, zeros (block f of the
    driver is hops f, f + 1 of this)"""
    pcm = np.asarray(pcm)
    n, n_ch = pcm.shape
    assert n % HOP == 0
    n_hops = n // HOP
    buf = np.zeros((n_ch, (n_hops + 3) * HOP))
    for ch in range(n_ch):
        buf[ch, HOP:HOP + n] = po.pcm16_to_fraction(pcm[:, ch])
    if n_hops:
        buf[:, HOP + n:2 * HOP + n] = buf[:, n:HOP + n]
    return buf


def block_flags(buf, block_switching):
    """(last, cur, next) of every block the driver submits (coder/pacfile.py:717-741 and Close): the detector sees
    hop h followed by zeros -- the second half of its look-ahead buffer is never filled"""
    n_hops = buf.shape[1] // HOP - 3
    tr = [bool(po.transient_detect(np.concatenate((buf[:, (h + 1) * HOP:(h + 2) * HOP], np.zeros((buf.shape[0], HOP))),
                                                   axis=1))) if block_switching else False for h in range(n_hops)]
    flags, last_t, cur_t = [], False, False
    for h in range(n_hops + 1):
        nxt = tr[h] if h < n_hops else False
        flags.append((last_t, cur_t, nxt))
        last_t, cur_t = cur_t, nxt
    flags.append((False, False, False))
    return flags


def sub_blocks(full):
    """the eight 256-sample sub-blocks of a short-coded block (coder/pacfile.py:526-527)"""
    pad = HOP // 2 - SHORT // 2
    return [full[n:n + 2 * SHORT] for n in range(pad, 2 * HOP - SHORT - pad, SHORT)]


def dropped(buf, flags):
    """short-coded blocks with an all-zero sub-block in some channel: absent from the file (coder/pacfile.py:530-533)"""
    out = []
    for f, (_, cur_t, _) in enumerate(flags):
        full = buf[:, f * HOP:(f + 2) * HOP]
        out.append(bool(cur_t) and any(np.all(s == 0) for ch in range(full.shape[0]) for s in sub_blocks(full[ch])))
    return out


def record_map(pcm, block_switching):
    """(flags, first record of every block or -1, records in the file)"""
    buf = fractions(pcm)
    flags = block_flags(buf, block_switching)
    drop = dropped(buf, flags)
    n_ch = buf.shape[0]
    rec, at = [], 0
    for d in drop:
        rec.append(-1 if d else at)
        at += 0 if d else n_ch
    return flags, rec, at


def header_fields(data):
    """the '<LHLLHHHH' fields of a .pac header: sample rate, channels, samples, lines, nScaleBits, nMantSizeBits,
    useSBR, useVQ"""
    fmt = '<LHLLHHHH'
    return struct.unpack(fmt, data[4:4 + struct.calcsize(fmt)])


def records(data):
    """payload (offset, size) of every record of a .pac, and the header's (sample rate, channels, useSBR, useVQ)"""
    fmt = '<LHLLHHHH'
    (sr, n_ch, _, n_lines, _, _, use_sbr, use_vq) = header_fields(data)
    assert n_lines == HOP
    pos = 4 + struct.calcsize(fmt)
    pos += 4 + 2 * struct.unpack('<L', data[pos:pos + 4])[0]
    out = []
    while pos < len(data):
        n = struct.unpack('<L', data[pos:pos + 4])[0]
        out.append((pos + 4, n))
        pos += 4 + n
    return out, (sr, n_ch, bool(use_sbr), bool(use_vq))


def decoded_lines(br, p, cur_t):
    """(lines before / 2^overall, overall) of the next (sub-)block of a payload: the decoders up to the IMDCT"""
    if p.useVQ:
        bands = p.sfBandsShort if cur_t else p.sfBands
        overall = br.get(p.nScaleBits)
        alloc = [a + 1 if a else 0 for a in (br.get(p.nMantSizeBits) for _ in range(bands.nBands))]
        sbr = bool(p.useSBR and not cur_t and np.any(np.array(alloc)[np.array(p.omittedBands, dtype=int)] != 0))
        lines = pv.decode_lines_vq(br, p, alloc, cur_t, sbr)
        if sbr:
            lines = pv.sbr_reconstruct(lines, p)
        return lines, overall
    bands = p.sfBandsShort if cur_t else p.sfBands
    sf, alloc, mant, overall = po.parse_block_body(br, p, cur_t)
    lines = np.zeros(p.nMDCTLines)
    for b in range(bands.nBands):
        lo, hi = bands.lowerLine[b], bands.upperLine[b] + 1
        if alloc[b]:
            lines[lo:hi] = po.dequantize_vec(sf[b], mant[lo:hi], p.nScaleBits, alloc[b])
    return lines, overall


def band_values(x, xh, thr, bands):
    """(N_b, M_b, NMR_b) of one (sub-)block"""
    n = 4.0 * (x - xh) ** 2
    m = np.power(10.0, (thr - 96.0) / 10.0)
    nn = np.array([np.mean(n[bands.lowerLine[b]:bands.upperLine[b] + 1]) for b in range(bands.nBands)])
    mm = np.array([np.mean(m[bands.lowerLine[b]:bands.upperLine[b] + 1]) for b in range(bands.nBands)])
    return nn, mm, 10.0 * np.log10((nn + EPS) / mm)


def model(pcm, data, block_switching):
    """NMR of the .pac bytes `data` against the PCM they were made from.  -> dict: nmr_db, noise, mask
    [blocks, nCh, band_stride], short [blocks], xmax / xhmax [blocks, nCh, 8] (max |X| and max |Xh| of every
    (sub-)block: what the tests' line bars are relative to), flags, record."""
    data = bytes(data)
    recs, (sr, n_ch, use_sbr, use_vq) = records(data)
    p = po.make_params(sr, n_ch, 128, HOP, *header_fields(data)[4:6])      # the widths the stream itself declares
    p.useVQ, p.useSBR = use_vq, use_sbr
    p.omittedBands = list(po.omitted_bands(p.sfBands)) if use_sbr else []
    buf = fractions(pcm)
    flags, rec, n_rec = record_map(pcm, block_switching)
    assert n_rec == len(recs), (n_rec, len(recs))
    stride = max(p.sfBands.nBands, SUB * p.sfBandsShort.nBands)
    shape = (len(flags), n_ch, stride)
    out = {k: np.full(shape, np.nan) for k in ("nmr_db", "noise", "mask")}
    out["xmax"] = np.full((len(flags), n_ch, SUB), np.nan)
    out["xhmax"] = np.full((len(flags), n_ch, SUB), np.nan)       # max |decoded lines| / 2^overall likewise
    out["short"] = np.array([bool(f[1]) for f in flags])
    out["flags"], out["record"] = flags, rec
    for f, (last_t, cur_t, next_t) in enumerate(flags):
        if rec[f] < 0:
            continue
        for ch in range(n_ch):
            o, n = recs[rec[f] + ch]
            br = po.BitReader(data[o:o + n] + b'\0' * 8)
            assert (br.get(1), br.get(1), br.get(1)) == (int(last_t), int(cur_t), int(next_t)), f
            full = buf[ch, f * HOP:(f + 2) * HOP]
            if not cur_t:
                xh, overall = decoded_lines(br, p, False)
                x = po.mdct_forward(po.apply_window(full, last_t, cur_t, next_t), HOP, HOP)[:HOP]
                thr = po.masked_threshold(full, HOP, sr)
                vals = band_values(x, xh / (1. * (1 << overall)), thr, p.sfBands)
                for k, v in zip(("noise", "mask", "nmr_db"), vals):
                    out[k][f, ch, :len(v)] = v
                out["xmax"][f, ch, 0] = np.max(np.abs(x))
                out["xhmax"][f, ch, 0] = np.max(np.abs(xh)) / (1 << overall)
                continue
            nbs = p.sfBandsShort.nBands
            p.nMDCTLines = p.nSamplesPerBlock = SHORT
            try:
                for j, sub in enumerate(sub_blocks(full)):
                    xh, overall = decoded_lines(br, p, True)
                    x = po.mdct_forward(po.apply_window(sub, last_t, cur_t, next_t), SHORT, SHORT)[:SHORT]
                    thr = po.masked_threshold(sub, SHORT, sr)
                    vals = band_values(x, xh / (1. * (1 << overall)), thr, p.sfBandsShort)
                    for k, v in zip(("noise", "mask", "nmr_db"), vals):
                        out[k][f, ch, j * nbs:(j + 1) * nbs] = v
                    out["xmax"][f, ch, j] = np.max(np.abs(x))
                    out["xhmax"][f, ch, j] = np.max(np.abs(xh)) / (1 << overall)
            finally:
                p.nMDCTLines = p.nSamplesPerBlock = HOP
    return out


def band_line_counts(sr, short):
    """lines per band slot of a block's row: long [nBands], short [8 * nBandsShort]"""
    bands = po.band_table(SHORT if short else HOP, sr)
    n = np.asarray(bands.nLines, dtype=np.int64)
    return np.tile(n, SUB) if short else n
