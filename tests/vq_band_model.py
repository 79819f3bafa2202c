"""The band curve of the gain-shape coder and its second pass, stated in NumPy over the oracle (test helper).

The definition (include/pacx.h, pacx_vq_band_curve_batch / pacx_encode_vq_alloc_batch).  Units, cap, J and the arrays'
layout are band_model's (gain-shape without SBR: the front end, the overall scale and the SMRs are the scalar coder's),
and so are the pick, the totals and the solve, which work on the arrays alone -- they are reused, not restated.

  The curve, per unit and band b (lines x = X 2^overall of the band, n of them), candidate i, bits(i) as band_model's:
    i = 0:  Xh = 0
    else:   pv.quantize_gain_shape(x, bits(i) n) -> the fields through po.BitWriter and back through po.BitReader ->
            pv.dequantize_gain_shape(reader, bits(i) n, n) = Xh 2^overall
    nmr[b][i] = NMR_b of nmr_model.band_values(X, Xh, T, bands)
  and three rules:
    -inf   a band whose lines are all zero (gain 0: quantize_gain_shape writes nothing whatever it is offered, the
           encoder drops its allocation to 0) holds -inf at every candidate below n_cand: a pick gives it 0 bits;
    +inf   a candidate at which the oracle fails on some band of a channel-frame (an exception, as the reference's own
           coder raises or never returns there: PACX_ST_VQ_UNDEFINED) is +inf for every band of that channel-frame;
           and every candidate from n_cand on, as in the scalar curve;
    cap_alloc   po.bit_alloc(float(32 J), ...) with the all-zero bands set to 0, so that a unit coded with it writes
           exactly the length predicted from it.

  encode_stream_alloc(): the analysed PCM coded with a given allocation (sanitised as band_model.sanitise) over the
  oracle's own block writer, pv.pack_channel_block_vq.
"""
import os
import struct

import numpy as np

import band_model as bm
import nmr_model as nm
import rate_model as rm
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv

SUB, CAND = bm.SUB, bm.CAND
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "vq_band.npz")
# the fixture's stream: 4 hops of a golden excerpt, block switching on -> 6 written blocks, 12 channel-frames, at least
# one of them short-coded and one long-coded (make_vq_band.py checks that), capped at 320 kb/s per channel
STREAM = ("castanet", 25, 29)
CAP_KBPS = 320


def fixture_stream():
    """(pcm int16 [4096, 2], sample rate) of the fixture"""
    name, h0, h1 = STREAM
    ex = np.load(os.path.join(GOLDEN, f"excerpt_{name}.npz"))
    return np.ascontiguousarray(ex["pcm"][h0 * 1024:h1 * 1024]), int(ex["sr"])


def is_zero_band(u, b):
    lo, hi = u.bands.lowerLine[b], u.bands.upperLine[b] + 1
    return np.linalg.norm(u.xs[lo:hi]) == 0                  # quantize_gain_shape's own test


def code_band(x, n_bits):
    """one band through the coder, the bit writer, the bit reader and the decoder
    -> (Xh 2^overall [len(x)], bits written, the fields, their widths)"""
    n = len(x)
    idx, widths = pv.quantize_gain_shape(x, int(n_bits))
    written = int(sum(widths))
    if written == 0:
        return np.zeros(n), 0, idx, widths
    bw = po.BitWriter((written + 7) // 8 + 8)
    for v, w in zip(idx, widths):
        bw.put(v, w)
    br = po.BitReader(bw.bytes())
    xh = pv.dequantize_gain_shape(br, int(n_bits), n)
    assert br.pos == written, (br.pos, written)              # the decoder reads what the coder wrote, to the bit
    return np.asarray(xh, dtype=np.float64), written, idx, widths


def unit_curve(p, u):
    """-> (nmr [nBands, 16] before the +inf rule of a failing candidate, written [nBands, 16] bits, failed [16])"""
    bands, n_cand = u.bands, bm.max_mant(p)
    nb = bands.nBands
    nmr = np.full((nb, CAND), np.inf)
    written = np.zeros((nb, CAND), np.int64)
    failed = np.zeros(CAND, bool)
    zero = np.array([is_zero_band(u, b) for b in range(nb)])
    for i in range(n_cand):
        bits = bm.bits_of(i)
        xh = np.zeros(len(u.x))
        if bits:
            try:
                for b in range(nb):
                    lo, hi = bands.lowerLine[b], bands.upperLine[b] + 1
                    xh[lo:hi], written[b, i], _, _ = code_band(u.xs[lo:hi], bits * int(bands.nLines[b]))
            except Exception:                                # the reference's coder fails here: no defined payload
                failed[i] = True
                continue
        nmr[:, i] = nm.band_values(u.x, xh / (1. * (1 << u.overall)), u.thr, bands)[2]
    nmr[zero, :n_cand] = -np.inf
    return nmr, written, failed


def cap_alloc_of(p, u, J):
    a = np.asarray(po.bit_alloc(float(rm.STEP * J), bm.max_mant(p), u.bands.nBands, u.bands.nLines, u.smr), np.int64)
    a[[is_zero_band(u, b) for b in range(u.bands.nBands)]] = 0
    return a


def curve(a, max_kbps, only=None):
    """-> band_model.curve()'s dict (nmr, cap, cap_alloc and tables()) for the gain-shape coder, plus written
    [n_cf, band_stride, 16]: the bits every band wrote at every size.  only: a set of (cf, sb) to compute; the other
    units keep NaN / -1 / 0."""
    p, n_ch = a["p"], a["n_ch"]
    c = bm.tables(p)
    n_cf = len(a["flags"]) * n_ch
    c["nmr"] = np.full((n_cf, c["band_stride"], CAND), np.nan)
    c["cap"] = np.full((n_cf, SUB), -1, np.int32)
    c["cap_alloc"] = np.zeros((n_cf, c["band_stride"]), np.int32)
    c["written"] = np.zeros((n_cf, c["band_stride"], CAND), np.int64)
    for f, units in enumerate(a["units"]):
        if units is None:
            continue
        for ch, us in enumerate(units):
            cf = f * n_ch + ch
            failed = np.zeros(CAND, bool)
            for sb, u in enumerate(us):
                if only is not None and (cf, sb) not in only:
                    continue
                nb = u.bands.nBands
                J = rm.cap_steps(a, u, max_kbps)
                c["cap"][cf, sb] = rm.STEP * J
                nmr, written, bad = unit_curve(p, u)
                c["nmr"][cf, sb * nb:(sb + 1) * nb] = nmr
                c["written"][cf, sb * nb:(sb + 1) * nb] = written
                c["cap_alloc"][cf, sb * nb:(sb + 1) * nb] = cap_alloc_of(p, u, J)
                failed |= bad
            live = ~np.isnan(c["nmr"][cf, :, 0])
            for i in np.nonzero(failed)[0]:
                c["nmr"][cf, live, i] = np.inf               # every band of the channel-frame
    return c


def code_unit(p, u, alloc):
    """(final allocation, fields, widths, overall) of a unit with this allocation, as pv.encode_channel_vq makes them"""
    bands = u.bands
    alloc = np.array([int(v) for v in alloc], dtype=int)
    all_idx, all_bits = [], []
    for b in range(bands.nBands):
        if alloc[b]:
            lo, hi = bands.lowerLine[b], bands.upperLine[b] + 1
            idx, bits = pv.quantize_gain_shape(u.xs[lo:hi], int(alloc[b] * bands.nLines[b]))
            if sum(bits) == 0:
                alloc[b] = 0
            else:
                all_idx.append(idx)
                all_bits.append(bits)
    return alloc, all_idx, all_bits, u.overall


def params_vq(a):
    p = po.make_params(a["sample_rate"], a["n_ch"], 128, rm.HOP, *rm.widths(a))
    p.useVQ = True
    return p


def encode_stream_alloc(a, alloc, num_samples):
    """the gain-shape .pac stream (no SBR) of the analysed PCM with this allocation ([n_cf, band_stride], sanitised
    here; a record that would leave its slot is coded without bits) -> (bytes, final allocation [n_cf, band_stride],
    n_bytes [n_cf])"""
    n_ch = a["n_ch"]
    p = params_vq(a)
    alloc = bm.sanitise(bm.tables(p), alloc)
    final = np.zeros_like(alloc)
    n_bytes_all = np.zeros(len(alloc), np.int32)
    out = [po.pac_header(p, num_samples)]
    for f, row in enumerate(a["units"]):
        if row is None:
            continue
        for ch, us in enumerate(row):
            cf = f * n_ch + ch
            mine = alloc[cf]
            nb = us[0].bands.nBands
            parts = [code_unit(p, u, mine[j * nb:(j + 1) * nb]) for j, u in enumerate(us)]
            n_bytes, payload = pv.pack_channel_block_vq(p, a["flags"][f], parts)
            if n_bytes > bm.PAYLOAD_STRIDE:
                parts = [code_unit(p, u, np.zeros(nb, np.int32)) for u in us]
                n_bytes, payload = pv.pack_channel_block_vq(p, a["flags"][f], parts)
            for j, part in enumerate(parts):
                final[cf, j * nb:(j + 1) * nb] = part[0]
            n_bytes_all[cf] = n_bytes
            out.append(struct.pack('<L', int(n_bytes)))
            out.append(payload)
    return b''.join(out), final, n_bytes_all


def load_fixture():
    """the committed curve of fixture_stream() as a band_model curve dict"""
    z = np.load(FIXTURE)
    assert tuple(z["stream"]) == STREAM[1:] and str(z["excerpt"]) == STREAM[0] and int(z["cap_kbps"]) == CAP_KBPS
    pcm, sr = fixture_stream()
    c = bm.tables(po.make_params(sr, pcm.shape[1], 128))
    c["nmr"], c["cap"], c["cap_alloc"], c["written"] = z["nmr"], z["cap"], z["cap_alloc"], z["written"]
    return c
