"""How good is an encode: per-band noise-to-mask ratios (NMR) of a .pac stream, computed on the GPU.

The reference judges an encode by eye (test_sbr.py / test_blockswitch.py plot spectrograms).  Here every coded
band of every block gets the standard number of a perceptual coder: the coding noise in the band against the
masked threshold the encoder's own psychoacoustic model computed for it,

    NMR_b = 10 log10((mean 4 (X - Xh)^2 + eps) / mean 10^((T - 96) / 10))        (include/pacx.h, pacx_nmr_batch)

with X the original's MDCT lines, Xh the lines the decoder hands to the IMDCT and T getMaskedThreshold of the
original block.  Above 0 dB the noise of the band is predicted to be audible.

    pac, rep = encode_stream_report(pcm, 48000, 96)          # the bytes of pacfile.encode_stream + a Report
    rep = nmr_of_file(pcm, pac_bytes)                        # a .pac made elsewhere, e.g. by the reference itself
    rep.percentile(50), rep.share_audible(), rep.nmr_db[hop, ch, band]

Both work through the stream in chunks of at most chunk_hops blocks: PCM in, payloads decoded to lines by the
existing decoders, pacx_nmr_batch, pacx_nmr_summary; the summary accumulates on the device across chunks and
only the three band arrays (3 x band_stride doubles per channel-block) come back per chunk.
"""
import numpy as np

from . import _lib

HOP = 1024
_NO_PAYLOAD = _lib.ST_ZERO_SUBBLOCK | _lib.ST_VQ_UNDEFINED | _lib.ST_MALFORMED | _lib.ST_REF_RAISES
_LO, _STEP, _BINS = _lib.NMR_HIST_LO, _lib.NMR_HIST_STEP, _lib.NMR_HIST_BINS


class Summary:
    """Counts, counts above 0 dB, maxima and 0.5 dB histograms of NMR values per band index, long blocks (kind 0)
    and short sub-blocks (kind 1) apart: the host's view of pacx_nmr_summary's words.

      count, audible  int64 [2, 32];   max  float64 [2, 32] (NaN: no value);
      hist            int64 [2, 32, BINS + 2]: [0] below -120 dB, [1 + i] the bin from -120 + i/2 dB, [-1] from +40 dB."""

    def __init__(self, count, audible, maximum, hist):
        self.count, self.audible = np.asarray(count, np.int64), np.asarray(audible, np.int64)
        self.max, self.hist = np.asarray(maximum, np.float64), np.asarray(hist, np.int64)

    @classmethod
    def from_words(cls, words):
        """words: uint64 [2, 32, NMR_SUMMARY_WORDS] as the library keeps them (an int64 array holding them is fine)"""
        w = np.ascontiguousarray(words).view(np.uint64).reshape(2, _lib.NMR_MAX_BANDS, _lib.NMR_SUMMARY_WORDS)
        key = w[:, :, _lib.NMR_MAX]
        bits = np.where(key >> np.uint64(63), key & np.uint64(0x7FFFFFFFFFFFFFFF), ~key)     # the ordered key undone
        maximum = np.where(key == 0, np.nan, bits.astype(np.uint64).view(np.float64))
        return cls(w[:, :, _lib.NMR_COUNT].astype(np.int64), w[:, :, _lib.NMR_AUDIBLE].astype(np.int64), maximum,
                   w[:, :, _lib.NMR_HIST:].astype(np.int64))

    @classmethod
    def from_values(cls, nmr_db, short, n_bands_long, n_bands_short):
        """The same summary from the band arrays, on the host: nmr_db [hops, nCh, band_stride], short bool [hops]."""
        nmr_db, short = np.asarray(nmr_db, np.float64), np.asarray(short, bool)
        nb = _lib.NMR_MAX_BANDS
        count, audible = np.zeros((2, nb), np.int64), np.zeros((2, nb), np.int64)
        maximum, hist = np.full((2, nb), np.nan), np.zeros((2, nb, _BINS + 2), np.int64)
        for kind, (sel, n_b, per) in enumerate(((~short, n_bands_long, 1), (short, n_bands_short, _lib.SUB))):
            rows = nmr_db[sel]
            if not rows.size:
                continue
            vals = rows[:, :, :per * n_b].reshape(-1, per, n_b)
            for b in range(n_b):
                v = vals[:, :, b].ravel()
                v = v[~np.isnan(v)]
                if not v.size:
                    continue
                count[kind, b], audible[kind, b], maximum[kind, b] = v.size, np.count_nonzero(v > 0.0), v.max()
                pos = np.floor((v - _LO) / _STEP)
                idx = np.where(pos < 0, 0, np.where(pos >= _BINS, _BINS + 1, 1 + np.clip(pos, 0, _BINS - 1))).astype(np.int64)
                hist[kind, b] = np.bincount(idx, minlength=_BINS + 2)
        return cls(count, audible, maximum, hist)

    def __eq__(self, other):
        return (np.array_equal(self.count, other.count) and np.array_equal(self.audible, other.audible) and
                np.array_equal(self.hist, other.hist) and np.array_equal(self.max, other.max, equal_nan=True))

    def _pick(self, arr, kind, band):
        a = arr if kind is None else arr[kind:kind + 1]
        return a if band is None else a[:, band:band + 1]

    def share_audible(self, kind=None, band=None):
        """share of the values above 0 dB (NaN without values); kind 0 / 1: long blocks / short sub-blocks only"""
        n = int(self._pick(self.count, kind, band).sum())
        return float(self._pick(self.audible, kind, band).sum()) / n if n else float("nan")

    def maximum(self, kind=None, band=None):
        m = self._pick(self.max, kind, band)
        return float(np.nanmax(m)) if np.any(~np.isnan(m)) else float("nan")

    def percentile(self, q, kind=None, band=None):
        """The q-th percentile (0..100) of the values, read from the histogram: the value of rank ceil(q/100 n) lies
        in the bin this finds, and the answer is placed inside that bin by its rank -- within one bin width (0.5 dB)
        of the order statistic.  A rank in the underflow bin gives -120 dB, one in the overflow bin the maximum."""
        h = self._pick(self.hist, kind, band).reshape(-1, _BINS + 2).sum(axis=0)
        n = int(h.sum())
        if not n:
            return float("nan")
        rank = min(max(int(np.ceil(q / 100.0 * n)), 1), n)
        cum = np.cumsum(h)
        i = int(np.searchsorted(cum, rank))
        if i == 0:
            return _LO
        if i == _BINS + 1:
            return self.maximum(kind, band)
        before = int(cum[i - 1])
        return _LO + _STEP * ((i - 1) + (rank - before - 0.5) / int(h[i]))


class Report:
    """NMR of a stream, per block the driver writes (every hop, the last hop a second time, the Close block):

      nmr_db, noise, mask  float64 [hops, nCh, band_stride]: NMR_b in dB, N_b, M_b; a short-coded block holds
                           8 x n_bands_short values (sub-block j at [j * n_bands_short ...]); unused slots are NaN, and
                           so is a block without a payload (a dropped short-coded hop, PACX_ST_REF_RAISES, a record
                           the decoder reports as malformed or undefined);
      short                bool [hops]: coded as eight short sub-blocks;
      record               int64 [hops]: index of the block's first record in the file, -1 for a dropped hop;
      summary              Summary (from the device when the report was computed there, else from the arrays).

    Constructible from arrays alone (no GPU): Report(nmr_db, noise, mask, short, n_bands_long, n_bands_short)."""

    def __init__(self, nmr_db, noise, mask, short, n_bands_long, n_bands_short, summary=None, record=None):
        self.nmr_db, self.noise, self.mask = (np.asarray(a, np.float64) for a in (nmr_db, noise, mask))
        self.short = np.asarray(short, bool)
        self.n_bands_long, self.n_bands_short = int(n_bands_long), int(n_bands_short)
        assert self.nmr_db.ndim == 3 and self.nmr_db.shape == self.noise.shape == self.mask.shape
        assert self.short.shape == (self.nmr_db.shape[0],)
        self.record = None if record is None else np.asarray(record, np.int64)
        self.summary = summary if summary is not None else self.host_summary()

    def host_summary(self):
        return Summary.from_values(self.nmr_db, self.short, self.n_bands_long, self.n_bands_short)

    def percentile(self, q, kind=None, band=None):
        return self.summary.percentile(q, kind, band)

    def median(self, kind=None, band=None):
        return self.summary.percentile(50, kind, band)

    def share_audible(self, kind=None, band=None):
        return self.summary.share_audible(kind, band)

    def maximum(self, kind=None, band=None):
        return self.summary.maximum(kind, band)


# ------------------------------------------------------------------------------------------- the hop-to-record map
def flags_from_transients(tr):
    """Flag bytes (last | cur << 1 | next << 2) of the n + 2 blocks the driver writes for n hops, from the
    detector's decision per hop (coder/pacfile.py:717-741: the decision about hop h is `next` of block h, `cur`
    of block h + 1, `last` of block h + 2; the pass after EOF detects nothing and Close writes 0, 0, 0)."""
    tr = (np.asarray(tr) != 0).astype(np.uint8)
    n = len(tr)
    ext = np.concatenate((np.zeros(2, np.uint8), tr, np.zeros(2, np.uint8)))
    flags = ext[:n + 2] | (ext[1:n + 3] << 1) | (ext[2:n + 4] << 2)
    if n + 2:
        flags[-1] = 0
    return flags.astype(np.uint8)


def padded_stream(pcm, hop=HOP):
    """int16 [nCh, (n_hops + 3) * hop]: zeros, the hops, the last hop again, zeros -- block f of the driver is
    hops f, f + 1 of this (pacfile.device_stream's layout, on the host)."""
    n, n_ch = pcm.shape
    n_hops = n // hop
    buf = np.zeros((n_ch, (n_hops + 3) * hop), dtype=np.int16)
    buf[:, hop:hop + n] = pcm.T
    if n_hops:
        buf[:, hop + n:2 * hop + n] = pcm[n - hop:].T
    return buf


def dropped_blocks(buf, flags, hop=HOP):
    """bool per block: short-coded with an all-zero 256-sample sub-block in some channel -- the reference writes
    nothing for such a hop (coder/pacfile.py:530-533).  -32768 reads as -0.0 (coder/pcmfile.py:89-99)."""
    n_blocks = len(flags)
    out = np.zeros(n_blocks, bool)
    for f in np.nonzero(np.asarray(flags) & _lib.FLAG_CUR)[0]:
        full = np.abs(buf[:, f * hop:(f + 2) * hop].astype(np.int32)) & 32767
        for j in range(_lib.SUB):
            at = hop // 2 - 64 + 128 * j
            if np.any(np.all(full[:, at:at + 256] == 0, axis=1)):
                out[f] = True
                break
    return out


def record_map(flags, dropped, n_channels):
    """index of the first record of every block (-1: dropped) and the number of records the file must hold"""
    rec = np.full(len(flags), -1, np.int64)
    kept = ~np.asarray(dropped, bool)
    rec[kept] = np.arange(int(kept.sum()), dtype=np.int64) * n_channels
    return rec, int(kept.sum()) * n_channels


# ------------------------------------------------------------------------------------------------- the chunk loop
class _Accumulator:
    def __init__(self, enc, n_blocks, n_ch):
        import torch
        self.enc, self.n_ch = enc, n_ch
        shape = (n_blocks, n_ch, enc.band_stride)
        self.arrays = {k: np.empty(shape, np.float64) for k in ("nmr_db", "noise", "mask")}
        self.words = torch.zeros((2, _lib.NMR_MAX_BANDS, _lib.NMR_SUMMARY_WORDS), dtype=torch.int64, device=enc.device)

    def chunk(self, f0, view, flags, payload, n_bytes, status):
        """decode the chunk's payloads (slot layout) to lines, NMR against the original in `view`, add to the summary"""
        import torch
        enc, n_ch = self.enc, self.n_ch
        if enc.use_vq:
            dec = enc.decode_vq(payload, n_bytes, n_ch, want_lines=True, want_pcm=False)
            lines, overall, dec_status = dec["lines"], dec["overall"], dec["status"]
        else:
            codes = enc.unpack(payload, n_bytes)
            extra = {}
            enc.decode(codes, n_ch, want_pcm=False, extra=extra)
            lines, overall, dec_status = extra["lines"], codes["overall"], codes["status"] | extra["status"]
        status = (status | dec_status) & _NO_PAYLOAD
        status = torch.where(n_bytes > 0, status, torch.full_like(status, _lib.ST_ZERO_SUBBLOCK))
        r = enc.nmr(view, flags, lines, overall, status)
        enc.nmr_summary(r["nmr_db"], n_ch, flags, self.words)
        n = view.n_frames
        for k, a in self.arrays.items():
            a[f0:f0 + n] = r[k].cpu().numpy().reshape(n, n_ch, -1)

    def report(self, enc, flags, record):
        short = (np.asarray(flags) & _lib.FLAG_CUR) != 0
        return Report(self.arrays["nmr_db"], self.arrays["noise"], self.arrays["mask"], short, enc.sfBands.nBands,
                      enc.sfBandsShort.nBands, Summary.from_words(self.words.cpu().numpy()), record)


def _transients(enc, buf, n_hops, chunk_hops):
    """the detector's decision per hop, chunk by chunk on the GPU (pacx_transient_flags)"""
    import ctypes
    import torch
    from .engine import _ptr
    tr = np.zeros(n_hops, np.uint8)
    n_ch = buf.shape[0]
    for h0 in range(0, n_hops, chunk_hops):
        n = min(chunk_hops, n_hops - h0)
        dev = torch.as_tensor(np.ascontiguousarray(buf[:, (h0 + 1) * HOP:(h0 + 1 + n) * HOP]), device=enc.device)
        hops = _lib.PacxPcm(dev.data_ptr(), _lib.PCM_I16, n_ch, n, HOP, n * HOP, 1)
        out = torch.empty(n, dtype=torch.uint8, device=enc.device)
        enc._call("pacx_transient_flags", ctypes.byref(hops), _ptr(out), None, enc._stream())
        tr[h0:h0 + n] = out.cpu().numpy()
    return tr


def _chunk_view(enc, buf, f0, n):
    import torch
    from .engine import PcmView
    planar = torch.as_tensor(np.ascontiguousarray(buf[:, f0 * HOP:(f0 + n + 1) * HOP]), device=enc.device)
    return PcmView.stream(planar, HOP)


def _check_stream(pcm, n_lines):
    if int(n_lines) != HOP:
        raise NotImplementedError("the NMR report covers streams of nMDCTLines = 1024")
    pcm = np.ascontiguousarray(pcm)
    if pcm.ndim != 2 or pcm.dtype != np.int16 or len(pcm) % HOP:
        raise ValueError("pcm: int16 [n, nCh], n a multiple of 1024")
    return pcm


def encode_stream_report(pcm, sample_rate, kbps_per_channel, block_switching=False, header_samples=None,
                         n_scale_bits=4, n_mant_size_bits=12, use_vq=False, use_sbr=False, chunk_hops=4096, n_lines=1024):
    """pacfile.encode_stream with a Report: -> (.pac bytes, Report).  The bytes are encode_stream's for the same
    arguments; the report is computed from the payloads just written (unpacked / decoded to lines by the existing
    decoders).  At most chunk_hops blocks are on the device at a time."""
    import torch
    from . import context, pacfile
    from .audiofile import CodingParams
    pcm = _check_stream(pcm, n_lines)
    chunk_hops = max(1, int(chunk_hops or 4096))
    cp = CodingParams()
    cp.sampleRate, cp.nChannels = int(sample_rate), pcm.shape[1]
    cp.numSamples = len(pcm) if header_samples is None else int(header_samples)
    cp.nMDCTLines = cp.nSamplesPerBlock = HOP
    cp.nScaleBits, cp.nMantSizeBits = n_scale_bits, n_mant_size_bits
    cp.targetBitsPerSample = kbps_per_channel / (cp.sampleRate / 1000)
    cp.useSBR, cp.useVQ = bool(use_sbr), bool(use_vq)
    parts = [pacfile.header_bytes(cp)]
    enc = context.encoder_for_params(cp)
    n_ch, n_hops = pcm.shape[1], len(pcm) // HOP
    buf = padded_stream(pcm)
    n_blocks = n_hops + 2
    flags = flags_from_transients(_transients(enc, buf, n_hops, chunk_hops)) if block_switching \
        else np.zeros(n_blocks, np.uint8)
    acc = _Accumulator(enc, n_blocks, n_ch)
    written = np.zeros(n_blocks, bool)
    for f0 in range(0, n_blocks, chunk_hops):
        n = min(chunk_hops, n_blocks - f0)
        view = _chunk_view(enc, buf, f0, n)
        fl = torch.as_tensor(flags[f0:f0 + n], device=enc.device) if block_switching else None
        if use_vq:
            out = enc.encode_vq(view, fl)
        else:
            out = enc.encode_pack(view, fl)
            pacfile._raise_like_reference(out)
        body, total = enc.gather_body(out["payload"], out["n_bytes"])
        parts.append(body[:int(total.item())].cpu().numpy().tobytes())
        written[f0:f0 + n] = out["n_bytes"].view(n, n_ch)[:, 0].cpu().numpy() > 0
        acc.chunk(f0, view, fl, out["payload"], out["n_bytes"], out["status"])
    record, _ = record_map(flags, ~written, n_ch)
    return b"".join(parts), acc.report(enc, flags, record)


def encode_stream_to_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel=320, block_switching=False,
                         header_samples=None, allocation="budget"):
    """pacfile.encode_stream_nmr with a Report: -> (.pac bytes, Report, info).  The report is nmr_of_file's of the
    finished bytes.  info, for the n + 2 blocks the driver submits:
      budget   int32 [blocks, nCh, 8]: the BitAlloc budget of every long block ([..., 0]) / short sub-block, bits
               (allocation "budget" only);
      bit_alloc int32 [blocks, nCh, band_stride]: the mantissa size of every band as coded;
      capped   bool  [blocks, nCh]: some unit of the block reached the cap (PACX_ST_RATE_CAP) and may miss the target;
      written  bool  [blocks]: the block is in the file (a dropped short-coded hop is not);
      kbps_per_channel: the records of the file, their length prefixes included, over the duration of the blocks
                        submitted;
      allocation: "budget" or "band", as given (pacfile.encode_stream_nmr)."""
    return _stream_to_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching, header_samples,
                          allocation, False)


def _stream_to_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching, header_samples, allocation,
                   use_vq):
    """encode_stream_to_nmr, and with use_vq encode_stream_vq_to_nmr"""
    from . import pacfile
    data, out, enc = pacfile._encode_stream_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching,
                                                header_samples, allocation, use_vq=use_vq)
    n_ch = np.asarray(pcm).shape[1]
    n_bytes = out["n_bytes"].cpu().numpy().reshape(-1, n_ch)
    n_blocks = len(n_bytes)
    body = int(np.sum(n_bytes[n_bytes > 0] + 4))
    info = {
        "allocation": allocation,
        "bit_alloc": out["bit_alloc"].cpu().numpy().reshape(n_blocks, n_ch, -1),
        "capped": out["capped"].cpu().numpy().reshape(n_blocks, n_ch) if "capped" in out else
        (out["status"].cpu().numpy().reshape(n_blocks, n_ch) & _lib.ST_RATE_CAP) != 0,
        "written": n_bytes[:, 0] > 0,
        "kbps_per_channel": 8.0 * body / (n_blocks * HOP / float(sample_rate)) / n_ch / 1000.0,
    }
    if "budget" in out:
        info["budget"] = out["budget"].cpu().numpy().reshape(n_blocks, n_ch, _lib.SUB)
    return data, nmr_of_file(pcm, data, block_switching=bool(block_switching)), info


def encode_stream_to_rate(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, max_kbps_per_channel=320,
                          block_switching=False, header_samples=None, nmr_range_db=(-30, 30), allocation="budget",
                          segment_hops=None, peak_kbps_per_channel=None):
    """pacfile.encode_stream_abr with a Report: -> (.pac bytes, Report, info).  A list for kbps_per_channel or for
    max_bytes gives a list of such triples, all solved from one rate curve.  info, for the n + 2 blocks the driver
    submits, is encode_stream_to_nmr's (budget, bit_alloc, capped, written, kbps_per_channel: achieved, allocation) and
      target_nmr_db  the target found;   limit_bytes, total_bytes  the body limit and the body written;
      n_bytes        int32 [blocks, nCh]: the record lengths the solve predicted (the ones written).
    segment_hops (pacfile.encode_stream_abr; with a list of rates: one curve, one segmented solve per rate): info gains
      segments       dict of arrays per segment: first_block, blocks, limit_bytes, total_bytes, target_nmr_db;
    target_nmr_db becomes float64 [blocks], every block's segment's target, limit_bytes and total_bytes the sums over
    the segments.
    peak_kbps_per_channel (with segment_hops; pacfile.encode_stream_abr): the size is the stream's again, limit_bytes
    and total_bytes are the stream's, segments["limit_bytes"] holds the peaks, and
      segments       gains floor_nmr_db (the lowest target at which the segment fits its peak) and pinned (bool: its
                     target is above the stream's);
      stream_target_nmr_db  the one target of every segment that is not pinned."""
    return _stream_to_rate(pcm, sample_rate, kbps_per_channel, max_bytes, max_kbps_per_channel, block_switching,
                           header_samples, nmr_range_db, allocation, segment_hops, peak_kbps_per_channel, False)


def _stream_to_rate(pcm, sample_rate, kbps_per_channel, max_bytes, max_kbps_per_channel, block_switching, header_samples,
                    nmr_range_db, allocation, segment_hops, peak_kbps_per_channel, use_vq):
    """encode_stream_to_rate, and with use_vq encode_stream_vq_to_rate"""
    from . import pacfile
    many = isinstance(kbps_per_channel, (list, tuple)) or isinstance(max_bytes, (list, tuple))
    if many:
        if kbps_per_channel is not None and max_bytes is not None:
            raise ValueError("give exactly one of kbps_per_channel and max_bytes")
        sizes = [(k, None) for k in kbps_per_channel] if kbps_per_channel is not None else [(None, b) for b in max_bytes]
    else:
        sizes = [(kbps_per_channel, max_bytes)]
    done, enc = pacfile._encode_stream_abr(pcm, sample_rate, sizes, max_kbps_per_channel, block_switching,
                                           header_samples, nmr_range_db, allocation, segment_hops,
                                           peak_kbps_per_channel, use_vq=use_vq)
    n_ch = np.asarray(pcm).shape[1]
    res = []
    for data, sol, out, limit in done:
        n_bytes = out["n_bytes"].cpu().numpy().reshape(-1, n_ch)
        n_blocks = len(n_bytes)
        target, total, segments = sol["target_nmr_db"], sol["total_bytes"], sol.get("segments")
        if segments is not None:
            segments = dict(segments, total_bytes=total, target_nmr_db=target)
            target, total = np.repeat(target, segments["blocks"]), int(total.sum())
            if "pinned" in sol:
                segments.update(floor_nmr_db=sol["floor_nmr_db"], pinned=sol["pinned"])
        info = {
            "allocation": allocation,
            "target_nmr_db": target,
            "limit_bytes": limit,
            "total_bytes": total,
            "n_bytes": sol["n_bytes"].cpu().numpy().reshape(n_blocks, n_ch),
            "bit_alloc": out["bit_alloc"].cpu().numpy().reshape(n_blocks, n_ch, -1),
            "capped": sol["capped"].cpu().numpy().reshape(n_blocks, n_ch),
            "written": n_bytes[:, 0] > 0,
            "kbps_per_channel": 8.0 * int(np.sum(n_bytes[n_bytes > 0] + 4)) / (n_blocks * HOP / float(sample_rate)) /
            n_ch / 1000.0,
        }
        if "budget" in sol:
            info["budget"] = sol["budget"].cpu().numpy().reshape(n_blocks, n_ch, _lib.SUB)
        if segments is not None:
            info["segments"] = segments
        if "stream_target_nmr_db" in sol:
            info["stream_target_nmr_db"] = sol["stream_target_nmr_db"]
        res.append((data, nmr_of_file(pcm, data, block_switching=bool(block_switching)), info))
    return res if many else res[0]


def encode_stream_vq_to_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel=320, block_switching=False,
                            header_samples=None):
    """pacfile.encode_stream_vq_nmr with a Report: -> (.pac bytes, Report, info).  The report is nmr_of_file's of the
    finished gain-shape bytes; info is encode_stream_to_nmr's with allocation = "band" (bit_alloc: the final
    allocation, 0 in a band whose lines are all zero)."""
    return _stream_to_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching, header_samples,
                          "band", True)


def encode_stream_vq_to_rate(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, max_kbps_per_channel=320,
                             block_switching=False, header_samples=None, nmr_range_db=(-30, 30), segment_hops=None,
                             peak_kbps_per_channel=None):
    """pacfile.encode_stream_vq_abr with a Report: -> (.pac bytes, Report, info), or a list of them for a list of
    sizes (one gain-shape curve, one solve and one second pass per size).  info is encode_stream_to_rate's with
    allocation = "band"."""
    return _stream_to_rate(pcm, sample_rate, kbps_per_channel, max_bytes, max_kbps_per_channel, block_switching,
                           header_samples, nmr_range_db, "band", segment_hops, peak_kbps_per_channel, True)


def _rates_kbps(hop_bytes, n_ch, block_seconds):
    """(mean, maximum) kb/s per channel of the blocks whose body bytes are hop_bytes"""
    if len(hop_bytes) == 0:
        return 0.0, 0.0
    per_block = 8.0 * np.asarray(hop_bytes, np.float64) / block_seconds / n_ch / 1000.0
    return float(per_block.mean()), float(per_block.max())


def _stream_to_buffer(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel, start_bytes,
                      max_kbps_per_channel, block_switching, header_samples, nmr_range_db, allocation, use_vq,
                      pinned=None):
    """pacfile._encode_stream_buffered and the scan of what it wrote (pinned: the scan that also gives the level
    through every block) -> (.pac bytes, encode_stream_to_buffer's info, the solve's dict, the scan's)"""
    from . import pacfile
    data, sol, out, limit, b, enc = pacfile._encode_stream_buffered(
        pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel, start_bytes, max_kbps_per_channel,
        block_switching, header_samples, nmr_range_db, allocation, use_vq, pinned)
    n_ch = np.asarray(pcm).shape[1]
    n_bytes = out["n_bytes"].cpu().numpy().reshape(-1, n_ch)
    scan = (enc.bucket_scan if pinned is None else enc.bucket_through)(out["n_bytes"], n_ch, b, want_level=True)
    mean, most = _rates_kbps(np.where(n_bytes > 0, n_bytes + 4, 0).sum(axis=1), n_ch, HOP / float(sample_rate))
    info = {
        "allocation": allocation,
        "target_nmr_db": sol["target_nmr_db"],
        "limit_bytes": limit,
        "total_bytes": scan["total"],
        "bucket": b,
        "n_bytes": sol["n_bytes"].cpu().numpy().reshape(-1, n_ch),
        "level_bytes": scan["level"].cpu().numpy() / 2.0 ** _lib.BUCKET_Q,
        "peak_bytes": scan["peak_bytes"],
        "peak_block": scan["peak_hop"],
        "end_bytes": scan["end_bytes"],
        "mean_kbps_per_channel": mean,
        "max_kbps_per_channel_seen": most,
    }
    return data, info, sol, scan


def encode_stream_to_buffer(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel=None, start_bytes=0,
                            max_kbps_per_channel=320, block_switching=False, header_samples=None, nmr_range_db=(-30, 30),
                            allocation="budget", use_vq=False):
    """pacfile.encode_stream_abr_buffered with what the buffer saw: -> (.pac bytes, info).  info, for the n + 2 blocks
    the driver submits:
      target_nmr_db  the target found;   limit_bytes, total_bytes  the body limit and the body written;
      bucket         the pacfile.Bucket of the call;
      n_bytes        int32 [blocks, nCh]: the record lengths the solve predicted (the ones written);
      level_bytes    float64 [blocks]: the buffer's level right after every block's records arrive (a dropped hop
                     brings none and only drains);
      peak_bytes, peak_block  the highest of them and the first block that reaches it (-1: the start level);
      end_bytes      the level after the last block has drained;
      mean_kbps_per_channel, max_kbps_per_channel_seen  the body over the duration of the blocks, and the largest block
                     at the rate of its own duration;
      allocation     as given."""
    data, info, _, _ = _stream_to_buffer(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel,
                                         start_bytes, max_kbps_per_channel, block_switching, header_samples,
                                         nmr_range_db, allocation, use_vq)
    return data, info


def encode_stream_to_buffer_pinned(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel=None,
                                   start_bytes=0, max_kbps_per_channel=320, block_switching=False, header_samples=None,
                                   nmr_range_db=(-30, 30), allocation="budget", use_vq=False, pin_step_db=1.0,
                                   max_phases=8):
    """pacfile.encode_stream_abr_pinned with what the buffer saw: -> (.pac bytes, info).  info is
    encode_stream_to_buffer's (target_nmr_db: the stream's level, the target of every free block) and
      block_target_nmr_db  float64 [blocks]: the target of every block;
      phase_of             int32 [blocks]: the phase that pinned the block, -1: free;
      phases, open         the bisections run, and whether the last phase allowed still pinned a block;
      through_bytes        float64 [blocks]: the highest level any stretch of blocks containing the block reaches."""
    data, info, sol, scan = _stream_to_buffer(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel,
                                              start_bytes, max_kbps_per_channel, block_switching, header_samples,
                                              nmr_range_db, allocation, use_vq, (pin_step_db, max_phases))
    info.update({
        "block_target_nmr_db": sol["target_t"].cpu().numpy().astype(np.float64) / _lib.RATE_TARGET_GRID,
        "phase_of": sol["phase_of"].cpu().numpy(),
        "phases": sol["phases"],
        "open": sol["open"],
        "through_bytes": scan["through"].cpu().numpy() / 2.0 ** _lib.BUCKET_Q,
    })
    return data, info


def buffer_report(pac_bytes, kbps_per_channel, buffer_bytes, start_bytes=0):
    """Whether a finished .pac, made anywhere, plays through a leaky bucket (pacfile.bucket: kbps_per_channel leaves a
    buffer of buffer_bytes per block; the channels, sample rate and block size are the file's): the header is parsed
    (pacfile.parse_header), the record sizes are read on the device (Encoder.index_body) and the level is their
    Encoder.bucket_scan.  -> dict
      bucket       the pacfile.Bucket;   blocks  the blocks in the file;   total_bytes  its body;
      level_bytes  float64 [blocks]: the level right after every block's records arrive;
      peak_bytes, peak_block, end_bytes, first_over (the first block above the buffer, -1: none) and fits (bool);
      mean_kbps_per_channel, max_kbps_per_channel_seen  as encode_stream_to_buffer gives them.
    A hop the encoder dropped (a short-coded hop with an all-zero sub-block) leaves no record in a body, so the report
    runs over the records present: the dropped hop's share of draining is missing and every level here is AT OR ABOVE
    the true one -- a stream that fits by this report fits.  ValueError for a body whose record chain breaks or does
    not hold whole blocks."""
    import torch
    from . import context, pacfile
    data = bytes(pac_bytes)
    cp, pos = pacfile.parse_header(data)
    n_ch = cp.nChannels
    b = pacfile.bucket(kbps_per_channel, n_ch, cp.sampleRate, buffer_bytes, start_bytes, hop=cp.nMDCTLines)
    enc = context.encoder_for_params(cp)
    body = torch.as_tensor(np.frombuffer(data, np.uint8)[pos:].copy(), device=enc.device)
    if body.numel():
        _, sizes, result = enc.index_body(body, n_ch)
        records, used, broke = (int(v) for v in result.cpu().numpy())
    else:
        sizes, records, used, broke = torch.zeros((0,), dtype=torch.int32, device=enc.device), 0, 0, -1
    if broke >= 0 or used != body.numel():
        raise ValueError(f"the body's record chain breaks at byte {broke if broke >= 0 else used} of {body.numel()}: "
                         f"{records} records in whole blocks of {n_ch} were read")
    scan = enc.bucket_scan(sizes[:records], n_ch, b, want_level=True)
    hop_bytes = (sizes[:records].view(-1, n_ch).to(torch.int64) + 4).sum(dim=1).cpu().numpy()
    mean, most = _rates_kbps(hop_bytes, n_ch, cp.nMDCTLines / float(cp.sampleRate))
    return {
        "bucket": b,
        "blocks": records // n_ch,
        "total_bytes": scan["total"],
        "level_bytes": scan["level"].cpu().numpy() / 2.0 ** _lib.BUCKET_Q,
        "peak_bytes": scan["peak_bytes"],
        "peak_block": scan["peak_hop"],
        "end_bytes": scan["end_bytes"],
        "first_over": scan["first_over"],
        "fits": scan["first_over"] < 0,
        "mean_kbps_per_channel": mean,
        "max_kbps_per_channel_seen": most,
    }


def rate_curve(pcm, sample_rate, max_kbps_per_channel=320, block_switching=False):
    """The rate-distortion curve of every long block / short sub-block of a stream, for plotting rate against
    quality: -> dict of NumPy arrays for the n + 2 blocks the driver submits,
      worst  float64 [blocks, nCh, row]: max_b NMR_b (dB) with BitAlloc budget 32 j, sub-block sb of a short-coded
             block at [sb * sub_stride + j]; NaN where there is no unit or no such budget;
      bits   int32 [blocks, nCh, row]: the bits of the unit in the file with that budget;
      steps  int32 [blocks, nCh, 8]: the largest j of every unit (the cap rate's budget), -1 where there is none
    and the ints row, sub_stride."""
    from . import pacfile
    cp, enc, view, flags = pacfile._rate_stream_setup(pcm, sample_rate, max_kbps_per_channel, block_switching, None)
    c = enc.rate_curve(view, flags, cp.targetBitsPerSample)
    n_ch = cp.nChannels
    return {"worst": c["worst"].cpu().numpy().reshape(-1, n_ch, c["row"]),
            "bits": c["bits"].cpu().numpy().reshape(-1, n_ch, c["row"]),
            "steps": c["steps"].cpu().numpy().reshape(-1, n_ch, _lib.SUB), "row": c["row"], "sub_stride": c["sub_stride"]}


def band_curve(pcm, sample_rate, max_kbps_per_channel=320, block_switching=False):
    """The noise-to-mask ratio of every band of a stream at every mantissa size, for plotting: -> dict of NumPy
    arrays for the n + 2 blocks the driver submits,
      nmr        float64 [blocks, nCh, band_stride, 16]: NMR_b (dB) with candidate i = 0 bits for i = 0, else i + 1;
                 sub-block sb of a short-coded block at [sb * nBandsShort + b]; NaN where there is no band, +inf
                 beyond the widest mantissa;
      cap        int32 [blocks, nCh, 8]: the mantissa bits the cap rate allows every unit, -1 where there is none;
      cap_alloc  int32 [blocks, nCh, band_stride]: BitAlloc's allocation at that budget."""
    from . import pacfile
    cp, enc, view, flags = pacfile._rate_stream_setup(pcm, sample_rate, max_kbps_per_channel, block_switching, None)
    c = enc.band_curve(view, flags, cp.targetBitsPerSample)
    n_ch = cp.nChannels
    return {"nmr": c["nmr"].cpu().numpy().reshape(-1, n_ch, enc.band_stride, _lib.BAND_CAND),
            "cap": c["cap"].cpu().numpy().reshape(-1, n_ch, _lib.SUB),
            "cap_alloc": c["cap_alloc"].cpu().numpy().reshape(-1, n_ch, enc.band_stride)}


def stream_rate_profile(pcm, sample_rate, chunk_hops=4096, max_kbps_per_channel=320, block_switching=False,
                        nmr_range_db=(-30, 30), use_vq=False, allocation="band"):
    """The body size of a stream at every target of a range, for plotting size against quality, from one analysis
    pass in chunks of chunk_hops blocks (pacfile.encode_stream_abr_chunked's first pass; pcm as there): ->
    (targets_db float64 [G], total_bytes int64 [G]), the grid of 1/64 dB over nmr_range_db and what
    encode_stream_nmr(target, allocation="band") -- use_vq: encode_stream_vq_nmr -- takes for its body there.
    allocation="budget" (not with use_vq): what encode_stream_nmr(target, allocation="budget") takes instead."""
    from . import pacfile
    pacfile._check_allocation(allocation)
    _, _, make = pacfile._abr_chunked_setup(pcm, sample_rate, chunk_hops, max_kbps_per_channel, block_switching, None,
                                            nmr_range_db, use_vq, allocation)
    hr = make()
    profile = hr.analyse(pcm)
    hr.s_k.synchronize()                               # the pass runs on the encoder's kernel stream
    total = profile.cpu().numpy()
    return float(hr.lo) + np.arange(len(total)) / float(_lib.RATE_TARGET_GRID), total


def nmr_of_file(pcm, pac_bytes, block_switching=None, chunk_hops=4096):
    """Report of a .pac made elsewhere (by the reference itself, say) against the PCM it was made from.  The
    hop-to-record map is re-derived the way the writer makes it: the transient detector gives the flags, a
    short-coded hop with an all-zero sub-block is absent from the file, the last hop is written twice and Close
    adds a block of zeros.  block_switching None: a file none of whose records carries a flag and that holds
    every block was written without block switching.  ValueError when a record's flag bits or the number of
    records disagree with the map (the PCM is not what the file was made from)."""
    import torch
    from . import context, pacfile
    data = bytes(pac_bytes)
    cp, pos = pacfile.parse_header(data)
    pcm = _check_stream(pcm, cp.nMDCTLines)
    if pcm.shape[1] != cp.nChannels:
        raise ValueError(f"the file has {cp.nChannels} channels, the PCM {pcm.shape[1]}")
    chunk_hops = max(1, int(chunk_hops or 4096))
    enc = context.encoder_for_params(cp)
    n_ch, n_hops = cp.nChannels, len(pcm) // HOP
    n_blocks = n_hops + 2
    offs, sizes = pacfile.record_chain(data, pos, enc.payload_stride)
    raw = np.frombuffer(data, np.uint8)
    first = raw[np.asarray(offs, np.int64)] if offs else np.zeros(0, np.uint8)
    rec_flags = ((first >> 7) & 1) | (((first >> 6) & 1) << 1) | (((first >> 5) & 1) << 2)      # last | cur | next, MSB first
    buf = padded_stream(pcm)
    if block_switching is None:
        block_switching = bool(rec_flags.any()) or len(offs) != n_blocks * n_ch
    flags = flags_from_transients(_transients(enc, buf, n_hops, chunk_hops)) if block_switching \
        else np.zeros(n_blocks, np.uint8)
    dropped = dropped_blocks(buf, flags)
    record, n_records = record_map(flags, dropped, n_ch)
    if len(offs) != n_records:
        raise ValueError(f"the file holds {len(offs)} records, this PCM gives {n_records}")
    want = np.repeat(flags[~dropped], n_ch)
    if not np.array_equal(rec_flags, want):
        bad = int(np.nonzero(rec_flags != want)[0][0])
        raise ValueError(f"record {bad} carries the flags {int(rec_flags[bad])}, this PCM gives {int(want[bad])}")
    acc = _Accumulator(enc, n_blocks, n_ch)
    slot = enc.payload_stride
    for f0 in range(0, n_blocks, chunk_hops):
        n = min(chunk_hops, n_blocks - f0)
        payload = np.zeros((n * n_ch, slot), np.uint8)
        n_bytes = np.zeros(n * n_ch, np.int32)
        for i in range(n):
            r = record[f0 + i]
            if r < 0:
                continue
            for ch in range(n_ch):
                o, s = offs[r + ch], sizes[r + ch]
                payload[i * n_ch + ch, :s] = raw[o:o + s]
                n_bytes[i * n_ch + ch] = s
        view = _chunk_view(enc, buf, f0, n)
        fl = torch.as_tensor(flags[f0:f0 + n], device=enc.device) if block_switching else None
        acc.chunk(f0, view, fl, torch.as_tensor(payload, device=enc.device), torch.as_tensor(n_bytes, device=enc.device),
                  torch.zeros(n * n_ch, dtype=torch.int32, device=enc.device))
    return acc.report(enc, flags, record)
