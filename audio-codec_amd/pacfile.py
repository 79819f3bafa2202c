"""pacfile.py mirror (coder/pacfile.py): the .pac block API in front of the GPU
path: scalar mantissas, or the gain-shape coder with or without SBR
(codingParams.useVQ / useSBR, the reference driver's own settings).

  PACFile.WriteFileHeader / WriteDataBlock / Close / Encode keep the
  reference's signatures and write the same bytes (one GPU call per block:
  drop-in, not fast);
  encode_stream() is the batched path: every hop of a stream in one
  pacx_encode_batch + pacx_pack_batch + pacx_gather_body.
"""
from collections import namedtuple
from fractions import Fraction
from math import floor
from struct import pack

import numpy as np

from . import _lib, codec, context, curves
from .audiofile import AudioFile
from .engine import Encoder, PcmView
from .pcmfile import codes_to_fraction
from .psychoac import AssignMDCTLinesFromFreqLimits, ScaleFactorBands

BYTESIZE = 8
_ST_VQ_UNDEFINED = 8          # include/pacx.h
_ST_MALFORMED = 32
_PARTIAL = "Only read a partial block of coded PACFile data"     # coder/pacfile.py:203-205
_VQ_UNDEFINED = "stream holds a gain-shape block the reference's decoder fails on (PACX_ST_VQ_UNDEFINED)"


def omitted_bands(sfBands, factor=2):
    """coder/sbr.py:6-9."""
    return np.where(sfBands.lowerLine >= sfBands.upperLine[-1] // factor)[0]


def header_bytes(cp):
    """coder/pacfile.py:306-333 (mutates cp.numSamples exactly as the reference does)."""
    if not cp.numSamples % cp.nMDCTLines:
        cp.numSamples += cp.nMDCTLines - cp.numSamples % cp.nMDCTLines
    cp.numSamples += cp.nMDCTLines
    out = b"PAC " + pack("<LHLLHHHH", cp.sampleRate, cp.nChannels, cp.numSamples, cp.nMDCTLines,
                         cp.nScaleBits, cp.nMantSizeBits, int(cp.useSBR), int(cp.useVQ))
    cp.sfBands = ScaleFactorBands(AssignMDCTLinesFromFreqLimits(cp.nMDCTLines, cp.sampleRate))
    cp.sfBandsShort = ScaleFactorBands(AssignMDCTLinesFromFreqLimits(128, cp.sampleRate))
    cp.omittedBands = omitted_bands(cp.sfBands) if cp.useSBR else []
    out += pack("<L", cp.sfBands.nBands)
    out += pack("<" + str(cp.sfBands.nBands) + "H", *(cp.sfBands.nLines.tolist()))
    return out


def _raise_like_reference(out):
    """Scalar mantissas in an SBR file: the reference raises TypeError on the first long block
    whose omitted band receives bits (coder/codec.py:541-546 -> coder/quantize.py:73-74); the
    kernels flag those channel-blocks (PACX_ST_REF_RAISES, include/pacx.h)."""
    if out["status"].numel() and int(out["status"].max().item()) & _lib.ST_REF_RAISES:
        raise TypeError(_lib.REF_SCALAR_SBR_ERROR)


_SBR_INDEX = ("index 1024 is out of bounds for axis 0 with size 1024 (Decode_SBR, coder/codec.py:173-176: the "
              "cut lies in the lower half of the spectrum; PACX_ST_VQ_UNDEFINED)")


def _decode_scalar(enc, cp, codes, **want):
    """Scalar-mantissa blocks through PACFile.Decode's routing (coder/pacfile.py:645-668).  In an SBR file a
    long block with a coded omitted band is Decode_SBR's (scalar branch, coder/codec.py:117-134) -- a block no
    encoder of the reference writes (it raises there, _raise_like_reference) but its reader and decoder take;
    where Decode_SBR raises IndexError (band tables of rates above 48 kHz) so does this."""
    if not getattr(cp, "useSBR", False):
        return enc.decode(codes, cp.nChannels, **want)
    extra = {}
    out = enc.decode(codes, cp.nChannels, extra=extra, **want)
    if extra["status"].numel() and int(extra["status"].max().item()) & _ST_VQ_UNDEFINED:
        raise IndexError(_SBR_INDEX)
    return out


class PACFile(AudioFile):
    tag = b"PAC "

    def WriteFileHeader(self, codingParams):
        self.fp.write(header_bytes(codingParams))
        codingParams.priorBlock = [np.zeros(codingParams.nMDCTLines, dtype=np.float64)
                                   for _ in range(codingParams.nChannels)]

    def _write_block_any_size(self, data, cp, lastTrans, curTrans, nextTrans):
        """WriteDataBlock for nMDCTLines other than 1024 (scalar mantissas): the reference's own sequence
        (coder/pacfile.py:449-610) with its Encode calls going to the function-level mirrors (codec.Encode composes
        a block of any length from GPU-backed pieces; 128-line sub-blocks take the tuned kernels) and the bit
        packing (:404-447, 552-565) restated on the host.  A correctness path: the batched entry points are built
        for the driver's 1024 lines."""
        long_n = cp.nMDCTLines
        full = [np.concatenate((cp.priorBlock[ch], data[ch])) for ch in range(cp.nChannels)]
        cp.priorBlock = data
        if not curTrans:
            parts = [[p] for p in zip(*self.Encode(full, cp, lastTrans, curTrans, nextTrans))]
            bands = cp.sfBands
        else:
            short = 128                                               # coder/pacfile.py:490
            pad = long_n // 2 - short // 2
            parts = [[] for _ in range(cp.nChannels)]
            long_bands, cp.sfBands = cp.sfBands, None                 # the 128-line blocks' handle: default long layout
            cp.nSamplesPerBlock = cp.nMDCTLines = short
            try:
                for n in range(pad, 2 * long_n - short - pad, short):
                    sub = [f[n:n + 2 * short] for f in full]
                    if any(np.all(x == 0) for x in sub):
                        return                                        # the whole hop is dropped (:530-533)
                    for ch, p in enumerate(zip(*self.Encode(sub, cp, lastTrans, curTrans, nextTrans))):
                        parts[ch].append(p)
            finally:
                cp.nSamplesPerBlock = cp.nMDCTLines = long_n
                cp.sfBands = long_bands
            bands = cp.sfBandsShort
        for ch in range(cp.nChannels):
            bits = codec._Bits()
            for f in (lastTrans, curTrans, nextTrans):
                bits.put(int(bool(f)), 1)
            n_bits = 4                                                # the size rule of :552-565
            for (sf, ba, mant, ov) in parts[ch]:
                bits.put(int(ov), cp.nScaleBits)
                n_bits += cp.nScaleBits
                at = 0
                for b in range(bands.nBands):
                    a = int(ba[b])
                    bits.put(a - 1 if a else 0, cp.nMantSizeBits)
                    bits.put(int(sf[b]), cp.nScaleBits)
                    n_bits += cp.nMantSizeBits + cp.nScaleBits
                    if a:
                        for j in range(int(bands.nLines[b])):
                            bits.put(int(mant[at + j]), a)
                        at += int(bands.nLines[b])
                        n_bits += a * int(bands.nLines[b])
            n_bytes = n_bits // 8 if n_bits % 8 == 0 else n_bits // 8 + 1
            blob = bits.tobytes()
            blob = blob[:n_bytes] + b"\0" * (n_bytes - len(blob))
            self.fp.write(pack("<L", n_bytes))
            self.fp.write(blob)

    def _read_block_any_size(self, cp):
        """ReadDataBlock for nMDCTLines other than 1024 (scalar mantissas): coder/pacfile.py:177-298 with the
        fields parsed on the host and the blocks decoded through the function-level mirrors."""
        long_n = cp.nMDCTLines
        data = []
        for ch in range(cp.nChannels):
            s = self.fp.read(4)
            if not s:
                if cp.overlapAndAdd:
                    tail, cp.overlapAndAdd = cp.overlapAndAdd, 0
                    return tail
                return None
            n = int.from_bytes(s, "little") if len(s) == 4 else -1
            blob = self.fp.read(n) if n > 0 else b""
            if n < 1 or len(blob) < n:
                raise RuntimeError(_PARTIAL)
            acc, pos = int.from_bytes(blob, "big"), [0]
            total = 8 * len(blob)

            def get(width):
                if pos[0] + width > total:
                    raise RuntimeError(_PARTIAL)
                v = (acc >> (total - pos[0] - width)) & ((1 << width) - 1) if width else 0
                pos[0] += width
                return v

            def one(cur):
                bands = cp.sfBandsShort if cur else cp.sfBands
                ov = get(cp.nScaleBits)
                ba, sf = [], []
                mant = np.zeros(cp.nMDCTLines, np.int32)
                for b in range(bands.nBands):
                    a = get(cp.nMantSizeBits)
                    a = a + 1 if a else 0
                    ba.append(a)
                    sf.append(get(cp.nScaleBits))
                    if a:
                        lo = int(bands.lowerLine[b])
                        for j in range(int(bands.nLines[b])):
                            mant[lo + j] = get(a)
                if cur:
                    cp.sfBands = None                                 # the 128-line blocks' handle: default long layout
                return self.Decode(sf, ba, mant, ov, None, cp, last, cur, nxt)

            last, cur, nxt = get(1), get(1), get(1)
            if not cur:
                block = one(False)
            else:
                short = 128
                block = np.zeros(2 * long_n)
                pad = long_n // 2 - short // 2
                long_bands = cp.sfBands
                cp.nSamplesPerBlock = cp.nMDCTLines = short
                try:
                    for k in range(pad, 2 * long_n - short - pad, short):
                        block[k:k + 2 * short] += one(True)
                finally:
                    cp.nSamplesPerBlock = cp.nMDCTLines = long_n
                    cp.sfBands = long_bands
            data.append(np.add(cp.overlapAndAdd[ch], block[:long_n]))
            cp.overlapAndAdd[ch] = block[long_n:]
        return data

    def WriteDataBlock(self, data, codingParams, lastTrans=False, curTrans=False, nextTrans=False):
        """coder/pacfile.py:449-610: prior || data per channel, encode, pack, write."""
        import torch
        cp = codingParams
        if cp.nMDCTLines != 1024 and not getattr(cp, "useVQ", False) and not getattr(cp, "useSBR", False):
            return self._write_block_any_size(data, cp, lastTrans, curTrans, nextTrans)
        enc = context.encoder_for_params(cp)
        blk = np.stack([np.concatenate((cp.priorBlock[ch], data[ch])) for ch in range(cp.nChannels)])
        cp.priorBlock = data
        pcm = PcmView.frames(torch.as_tensor(blk[None], device=enc.device))
        flags = [(bool(lastTrans), bool(curTrans), bool(nextTrans))]
        if getattr(cp, "useVQ", False):
            out = enc.encode_vq(pcm, flags)
            payload, n_bytes = out["payload"], out["n_bytes"]
        else:
            out = enc.encode(pcm, flags)
            _raise_like_reference(out)
            payload, n_bytes = enc.pack(out, cp.nChannels)
        n_bytes = n_bytes.cpu().numpy()
        if not n_bytes.any():
            return                                  # hop dropped (coder/pacfile.py:530-533)
        payload = payload.cpu().numpy()
        for ch in range(cp.nChannels):
            self.fp.write(pack("<L", int(n_bytes[ch])))
            self.fp.write(payload[ch, :n_bytes[ch]].tobytes())

    def Close(self, codingParams):
        """coder/pacfile.py:612-625: one block of zeros flushes the last hop."""
        if self.fp.mode == "wb":
            self.WriteDataBlock([np.zeros(codingParams.nMDCTLines) for _ in range(codingParams.nChannels)],
                                codingParams)
        self.fp.close()

    def Encode(self, data, codingParams, lastTrans=False, curTrans=False, nextTrans=False):
        """coder/pacfile.py:627-643."""
        if getattr(codingParams, "useSBR", False) and not curTrans:
            return codec.Encode_SBR(data, codingParams, lastTrans, curTrans, nextTrans)
        return codec.Encode(data, codingParams, lastTrans, curTrans, nextTrans)

    def Decode(self, scaleFactor, bitAlloc, mantissa, overallScaleFactor, pb, codingParams,
               lastTrans=False, curTrans=False, nextTrans=False):
        """coder/pacfile.py:645-668: Decode_SBR for a long block of an SBR file that codes an
        omitted band, codec.Decode otherwise."""
        cp = codingParams
        if getattr(cp, "useSBR", False) and not curTrans and len(getattr(cp, "omittedBands", [])) and \
                np.any(np.array(bitAlloc)[np.array(cp.omittedBands)] != 0):
            return codec.Decode_SBR(scaleFactor, bitAlloc, mantissa, overallScaleFactor, pb, cp,
                                    lastTrans, curTrans, nextTrans)
        return codec.Decode(scaleFactor, bitAlloc, mantissa, overallScaleFactor, pb, cp,
                            lastTrans, curTrans, nextTrans)

    def ReadFileHeader(self):
        """coder/pacfile.py:136-175."""
        head = self.fp.read(4 + 22 + 4)
        n_bands = int.from_bytes(head[-4:], "little")
        head += self.fp.read(2 * n_bands)
        cp, _ = parse_header(head)
        cp.omittedBands = omitted_bands(cp.sfBands) if cp.useSBR else []
        cp.overlapAndAdd = [np.zeros(cp.nMDCTLines, dtype=np.float64) for _ in range(cp.nChannels)]
        return cp

    def ReadDataBlock(self, codingParams):
        """coder/pacfile.py:231-298: one hop of every channel as signed fractions
        (overlap-and-add done); at the end of the file the pending half-block once,
        then None.  Unpacking and codec.Decode run on the GPU."""
        import torch
        cp = codingParams
        if cp.nMDCTLines != 1024 and not getattr(cp, "useVQ", False) and not getattr(cp, "useSBR", False):
            return self._read_block_any_size(cp)
        enc = context.encoder_for_params(cp)
        payloads = []
        for ch in range(cp.nChannels):
            s = self.fp.read(4)
            if not s:
                if cp.overlapAndAdd:
                    tail, cp.overlapAndAdd = cp.overlapAndAdd, 0
                    return tail
                return None
            if len(s) < 4:
                raise RuntimeError(_PARTIAL)
            n = int.from_bytes(s, "little")
            if n < 1 or n > enc.payload_stride:
                raise RuntimeError(_PARTIAL + f" (record of {n} bytes)")
            blob = self.fp.read(n)
            if len(blob) < n:
                raise RuntimeError(_PARTIAL)
            payloads.append(blob)
        slot = enc.payload_stride
        buf = np.zeros((cp.nChannels, slot), dtype=np.uint8)
        for ch, blob in enumerate(payloads):
            buf[ch, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        sizes = torch.tensor([len(b) for b in payloads], dtype=torch.int32, device=enc.device)
        if getattr(cp, "useVQ", False):
            out = enc.decode_vq(torch.as_tensor(buf, device=enc.device), sizes, cp.nChannels,
                                want_blocks=True, want_pcm=False)
            if int(out["status"].max().item()) & _ST_MALFORMED:
                raise RuntimeError(_PARTIAL)
            blocks = out["blocks"].cpu().numpy()
        else:
            codes = enc.unpack(torch.as_tensor(buf, device=enc.device), sizes)
            if int(codes["status"].max().item()) & _ST_MALFORMED:
                raise RuntimeError(_PARTIAL)
            blocks = _decode_scalar(enc, cp, codes, want_blocks=True, want_pcm=False).cpu().numpy()
        data = []
        for ch in range(cp.nChannels):
            data.append(np.add(cp.overlapAndAdd[ch], blocks[ch][:cp.nMDCTLines]))
            cp.overlapAndAdd[ch] = blocks[ch][cp.nMDCTLines:]
        return data


def stream_flags(pcm, block_switching, hop=1024):
    """(last, cur, next) for every written hop of the driver loop
    (coder/pacfile.py:717-741) plus the Close block.  pcm: int16 [n_hops*hop, nCh].
    Detector and flag shifting run on the GPU (pacx_transient_flags), as in encode_stream."""
    n_hops = len(pcm) // hop
    flags = np.zeros((n_hops + 2, 3), dtype=np.uint8)
    if block_switching and n_hops:
        enc = context.any_encoder()
        _, packed = enc.transient_flags(device_stream(enc, np.ascontiguousarray(pcm), hop), n_hops, hop)
        packed = packed.cpu().numpy()
        flags[:, 0], flags[:, 1], flags[:, 2] = packed & 1, (packed >> 1) & 1, (packed >> 2) & 1
    return flags                                          # last row (Close) stays 0,0,0


def device_stream(enc, pcm, hop=1024):
    """Planar int16 device buffer [nCh, (n_hops+3)*hop]: zeros, the hops, the
    last hop again (the driver writes it twice), zeros (Close)."""
    import torch
    n, n_ch = pcm.shape
    n_hops = n // hop
    buf = np.zeros((n_ch, (n_hops + 3) * hop), dtype=np.int16)
    buf[:, hop:hop + n] = pcm.T
    if n_hops:
        buf[:, hop + n:2 * hop + n] = pcm[n - hop:].T
    return torch.as_tensor(buf, device=enc.device)


def _encode_stream_any_size(pcm, cp, block_switching):
    """the reference's driver loop (coder/pacfile.py:716-757) over the PACFile mirror, block by block: nMDCTLines other
    than 1024"""
    import io
    from .detect_transients import parTransientDetect
    hop, n_ch = cp.nMDCTLines, cp.nChannels
    f = PACFile("<memory>")
    f.fp = io.BytesIO()
    f.fp.mode = "wb"
    f.WriteFileHeader(cp)
    look = np.zeros((n_ch, 2 * hop))
    cur = last = False
    n_hops = len(pcm) // hop
    for h in range(n_hops + 1):
        if h < n_hops:
            data = np.stack([codes_to_fraction(pcm[h * hop:(h + 1) * hop, ch]) for ch in range(n_ch)])
            look = np.concatenate((np.copy(data), look[:, hop:]), axis=1)
            nxt = bool(parTransientDetect(look)) if block_switching else False
        else:
            nxt = False
        f.WriteDataBlock([look[ch, :hop] for ch in range(n_ch)], cp, lastTrans=last, curTrans=cur, nextTrans=nxt)
        last, cur = cur, nxt
    f.WriteDataBlock([np.zeros(hop) for _ in range(n_ch)], cp)          # Close (:612-625)
    return f.fp.getvalue()


def encode_stream(pcm, sample_rate, kbps_per_channel, block_switching=False, header_samples=None,
                  n_scale_bits=4, n_mant_size_bits=12, use_vq=False, use_sbr=False, chunk_hops=None, n_lines=1024):
    """Whole-stream batched encode -> .pac bytes identical to what the
    reference's driver (coder/pacfile.py:674-757) writes for the same PCM:
    scalar mantissas by default; use_vq (+ use_sbr) selects the gain-shape
    coder, and the driver's own settings are use_vq=True,
    use_sbr=(kbps < 128), block_switching=True (:703-705).  pcm: int16
    [n, nCh], n a multiple of 1024 (see pcmfile.wav_effective_stream for real
    WAV files)."""
    from .audiofile import CodingParams
    pcm = np.ascontiguousarray(pcm)
    hop = int(n_lines)
    assert pcm.ndim == 2 and len(pcm) % hop == 0
    cp = CodingParams()
    cp.sampleRate, cp.nChannels = int(sample_rate), pcm.shape[1]
    cp.numSamples = len(pcm) if header_samples is None else int(header_samples)
    cp.nMDCTLines = cp.nSamplesPerBlock = hop
    cp.nScaleBits, cp.nMantSizeBits = n_scale_bits, n_mant_size_bits
    cp.targetBitsPerSample = kbps_per_channel / (cp.sampleRate / 1000)
    cp.useSBR, cp.useVQ = bool(use_sbr), bool(use_vq)
    if hop != 1024:
        # function level: the driver loop block by block through the mirrors (scalar mantissas; a correctness path)
        if use_vq or use_sbr:
            raise NotImplementedError("gain-shape / SBR streams: nMDCTLines 1024")
        return _encode_stream_any_size(pcm, cp, block_switching)
    head = header_bytes(cp)
    enc = context.encoder_for_params(cp)
    if chunk_hops:
        # host memory to host memory in chunks: PCM in, kernels and bodies out overlap on three streams
        # (streaming.HostStreamEncoder); same bytes as the one-batch path below
        from .streaming import HostStreamEncoder
        hs = HostStreamEncoder(enc, pcm.shape[1], int(chunk_hops), block_switching=block_switching)
        parts = [bytes(b) for b in hs.encode(pcm)]
        if hs.reference_raises():
            raise TypeError(_lib.REF_SCALAR_SBR_ERROR)
        return head + b"".join(parts)
    planar = device_stream(enc, pcm, hop)
    view = PcmView.stream(planar, hop)
    if block_switching:
        _, flags = enc.transient_flags(planar, len(pcm) // hop, hop)     # detector + flag shifting on the GPU
    else:
        flags = None
    if use_vq:
        out = enc.encode_vq(view, flags)
        payload, n_bytes = out["payload"], out["n_bytes"]
    else:
        out = enc.encode_pack(view, flags)
        _raise_like_reference(out)
        payload, n_bytes = out["payload"], out["n_bytes"]
    body, total = enc.gather_body(payload, n_bytes)
    n = int(total.item())
    return head + body[:n].cpu().numpy().tobytes()


def _rate_coding_params(pcm, sample_rate, max_kbps_per_channel, header_samples, use_vq=False):
    """the CodingParams of the rate-control streams, the cap rate as the handle's: checks the PCM's shape and type (pcm:
    anything with ndim, dtype, shape and len) and the cap, touches no sample and no GPU"""
    from .audiofile import CodingParams
    hop = 1024
    if pcm.ndim != 2 or pcm.dtype != np.int16 or len(pcm) % hop:
        raise ValueError("pcm: int16 [n, nCh], n a multiple of 1024")
    cp = CodingParams()
    cp.sampleRate, cp.nChannels = int(sample_rate), pcm.shape[1]
    cp.numSamples = len(pcm) if header_samples is None else int(header_samples)
    cp.nMDCTLines = cp.nSamplesPerBlock = hop
    cp.nScaleBits, cp.nMantSizeBits = 4, 12
    # the header carries no rate and the budgets are the search's: the handle's own rate is not used
    cp.targetBitsPerSample = max_kbps_per_channel / (cp.sampleRate / 1000)
    if not 0.0 < cp.targetBitsPerSample <= 16.0:
        raise ValueError(f"max_kbps_per_channel = {max_kbps_per_channel} at {cp.sampleRate} Hz is "
                         f"{cp.targetBitsPerSample:.3g} bits per sample: the cap must lie in (0, 16] bits per sample "
                         f"(at most {16 * cp.sampleRate / 1000:g} kb/s here)")
    cp.useSBR, cp.useVQ = False, bool(use_vq)
    return cp


def _rate_stream_setup(pcm, sample_rate, max_kbps_per_channel, block_switching, header_samples, use_vq=False):
    """(CodingParams, encoder, PCM view, flags) of the one-batch scalar path with the cap rate as the handle's; use_vq:
    of the gain-shape path without SBR"""
    pcm = np.ascontiguousarray(pcm)
    hop = 1024
    cp = _rate_coding_params(pcm, sample_rate, max_kbps_per_channel, header_samples, use_vq)
    enc = context.encoder_for_params(cp)
    planar = device_stream(enc, pcm, hop)
    view = PcmView.stream(planar, hop)
    flags = enc.transient_flags(planar, len(pcm) // hop, hop)[1] if block_switching else None
    return cp, enc, view, flags


class _CurvePath:
    """What the rate-control streams call on a curve, for both kinds (curves.RATE, curves.BAND): an operation is the
    solver's method of that name behind the kind's prefix, the layout of the kept bytes the kind's.  A subclass says
    which encoder solves, how the curve is taken (curve, layout) and what the second pass is (encode)."""
    kind = None

    def __init__(self, enc):
        self.enc = self.solver = enc

    def _op(self, name, *args, **kw):
        return getattr(self.solver, f"{self.kind.prefix}_{name}")(*args, **kw)

    def solve(self, curve, flags, limit_bytes, lo, hi):
        """flags: as given to curve(); only rate_solve takes them"""
        return self._op("solve", curve, limit_bytes, lo, hi)

    def solve_segments(self, curve, seg_first, limit_bytes, lo, hi):
        return self._op("solve_segments", curve, seg_first, limit_bytes, lo, hi)

    def solve_peak(self, curve, seg_first, peak_bytes, limit_bytes, lo, hi):
        return self._op("solve_peak", curve, seg_first, peak_bytes, limit_bytes, lo, hi)

    def solve_bucket(self, curve, flags, n_channels, limit_bytes, bucket, lo, hi, pinned=None):
        """flags: as solve takes them; pinned = (pin_step_db, max_phases): the solve with a target per hop"""
        return self._op("solve_bucket" if pinned is None else "solve_bucket_pinned", curve, n_channels, limit_bytes,
                        bucket, lo, hi, *(pinned or ()))

    # what the chunked encode (streaming.HostStreamRateEncoder) calls per chunk: the curve, its profile, the pick at
    # known targets and the second pass on that pick
    def no_frames(self, max_bits_per_sample):
        """the curve of no frame at all"""
        width, head = self.layout(max_bits_per_sample)
        return self.kind.no_frames(width, self.solver.device, **head)

    def profile(self, curve, lo, hi, out=None):
        return self._op("profile", curve, lo, hi, out=out)

    def profile_segments(self, curve, seg_cf, first_off, lo, hi, out=None):
        return self._op("profile_segments", curve, seg_cf, first_off, lo, hi, out=out)

    def pick(self, curve, target_nmr_db):
        """on a curve, or on a curve kept as thresholds (kept_views, thresholds)"""
        return self._op("pick_thresholds" if self.kind.is_kept(curve) else "pick", curve, target_nmr_db)

    def pick_segments(self, curve, seg_cf, first_off, target_t):
        return self._op("pick_thresholds_segments" if self.kind.is_kept(curve) else "pick_segments", curve, seg_cf,
                        first_off, target_t)

    pick_kept, pick_kept_segments = pick, pick_segments

    def bytes_kept(self, kept, target_t, out=None):
        """the n_bytes of pick() on a kept curve at several grid targets at once"""
        return self._op("bytes_thresholds", kept, target_t, out=out)

    def second_pass(self, view, flags, pick):
        """pick: what a pick or a solve returned"""
        return self.encode(view, flags, pick[self.kind.per_cf.key])

    # the curve kept between the passes (HostStreamRateEncoder.keep_curves): its thresholds and the layout of a chunk's
    # kept arrays in one run of bytes
    def kept_bytes_per_cf(self, max_bits_per_sample):
        return self.kind.kept_bytes_per_cf(self.layout(max_bits_per_sample)[0])

    def kept_views(self, buf, n_cf, max_bits_per_sample):
        width, head = self.layout(max_bits_per_sample)
        return self.kind.kept_views(buf, n_cf, width, **head)

    def thresholds(self, curve, lo, hi, out=None):
        return self._op("thresholds", curve, lo, hi, out=out)


class _BandPath(_CurvePath):
    """allocation="band", for the scalar coder and for the gain-shape one: the curve and the second pass are the
    coder's own, the pick and the solves work on the arrays alone and run on a scalar handle -- for a gain-shape
    encoder its scalar sibling (context.scalar_sibling)."""
    kind = curves.BAND

    def __init__(self, enc):
        self.enc = enc
        self.solver = context.scalar_sibling(enc) if enc.use_vq else enc

    def layout(self, max_bits_per_sample):
        """(width, the extra keys of a dict of the kind) at this cap rate"""
        return self.solver.band_stride, {}

    def curve(self, view, flags, max_bits_per_sample):
        if self.enc.use_vq:
            return self.enc.vq_band_curve(view, flags, max_bits_per_sample)
        return self.enc.band_curve(view, flags, max_bits_per_sample)

    def encode(self, view, flags, bit_alloc):
        if self.enc.use_vq:
            return self.enc.encode_vq_alloc(view, flags, bit_alloc)
        return self.enc.encode_pack_alloc(view, flags, bit_alloc)


class _BudgetPath(_CurvePath):
    """allocation="budget": BitAlloc with one budget per block, read from the rate curve.  Scalar coder only."""
    kind = curves.RATE

    def layout(self, max_bits_per_sample):
        row, sub = self.enc.rate_curve_layout(max_bits_per_sample)
        return row, {"row": row, "sub_stride": sub}

    def curve(self, view, flags, max_bits_per_sample):
        return self.enc.rate_curve(view, flags, max_bits_per_sample)

    def solve(self, curve, flags, limit_bytes, lo, hi):
        return self.enc.rate_solve(curve, flags, limit_bytes, lo, hi)

    def solve_bucket(self, curve, flags, n_channels, limit_bytes, bucket, lo, hi, pinned=None):
        op = self.enc.rate_solve_bucket if pinned is None else self.enc.rate_solve_bucket_pinned
        return op(curve, flags, n_channels, limit_bytes, bucket, lo, hi, *(pinned or ()))

    def encode(self, view, flags, budget):
        return self.enc.encode_pack_budget(view, flags, budget)


_PATHS = {"band": _BandPath, "budget": _BudgetPath}


def _check_allocation(allocation):
    if allocation not in ("budget", "band"):
        raise ValueError(f"allocation = {allocation!r}: 'budget' (BitAlloc with a budget per block) or 'band' (the "
                         f"smallest mantissa size per band)")
    return allocation == "band"


def _encode_stream_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching, header_samples,
                       allocation="budget", use_vq=False):
    """(.pac bytes, the outputs of Encoder.encode_pack_nmr -- allocation "band": of Encoder.encode_pack_alloc, with the
    pick's capped mask as out["capped"] -- for the n + 2 blocks the driver writes, the encoder).  use_vq (allocation
    "band" only): the gain-shape coder, the outputs of Encoder.encode_vq_alloc"""
    band = _check_allocation(allocation)
    if use_vq and not band:
        raise NotImplementedError("gain-shape streams: allocation 'band' only")
    cp, enc, view, flags = _rate_stream_setup(pcm, sample_rate, max_kbps_per_channel, block_switching, header_samples,
                                              use_vq)
    if band:
        if not np.isfinite(float(target_nmr_db)):
            raise ValueError("target_nmr_db must be finite")
        path = _BandPath(enc)
        pick = path.pick(path.curve(view, flags, cp.targetBitsPerSample), float(target_nmr_db))
        out = path.second_pass(view, flags, pick)
        out["capped"] = pick["capped"]
    else:
        out = enc.encode_pack_nmr(view, flags, float(target_nmr_db), cp.targetBitsPerSample)
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    return header_bytes(cp) + body[:int(total.item())].cpu().numpy().tobytes(), out, enc


def encode_stream_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel=320, block_switching=False,
                      header_samples=None, use_vq=False, use_sbr=False, chunk_hops=None, n_lines=1024,
                      allocation="budget"):
    """Whole-stream encode at constant quality instead of constant rate -> .pac bytes: the smallest stream (by the
    bisection of include/pacx.h, pacx_encode_pack_nmr_batch) whose predicted noise stays at or below target_nmr_db
    of the masked threshold in every band of every block, no block above the budget of max_kbps_per_channel.  An
    ordinary scalar .pac: every decoder of encode_stream's output takes it.  Scalar mantissas, 1024 lines, one
    batch: gain-shape / SBR streams, other block sizes and the chunked host-to-host encoder are not covered.
    The cap is at most 16 bits per sample (the widest mantissa; it bounds the search, include/pacx.h): with the
    default 320 kb/s that needs a sample rate of 20 kHz or more, below it pass a smaller max_kbps_per_channel
    (ValueError otherwise).
    allocation="budget" hands the bits to the bands by BitAlloc with the budget the bisection finds per block;
    "band" gives every band the smallest mantissa size that keeps it at or below the target (pacx_band_curve_batch,
    pacx_band_pick, pacx_encode_pack_alloc_batch): the same guarantee in fewer bits, a true minimum wherever the cap
    is not reached."""
    # use_vq, use_sbr, chunk_hops, n_lines: encode_stream's keywords, taken here only so that a caller who switches
    # from encode_stream gets NotImplementedError for what this mode does not cover, not a TypeError
    _check_allocation(allocation)
    if use_vq or use_sbr or chunk_hops or int(n_lines) != 1024:
        raise NotImplementedError("constant-quality streams: scalar mantissas, nMDCTLines 1024, one batch")
    return _encode_stream_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching, header_samples,
                              allocation)[0]


def _abr_limit(cp, view, head, kbps_per_channel, max_bytes):
    """the body limit in bytes of one of the two ways to give a size"""
    if (kbps_per_channel is None) == (max_bytes is None):
        raise ValueError("give exactly one of kbps_per_channel and max_bytes")
    if max_bytes is not None:
        limit = int(max_bytes) - len(head)
    else:
        if not kbps_per_channel > 0:
            raise ValueError("kbps_per_channel must be positive")
        # all the blocks the driver writes, at this rate: tests/rate_model.kbps_per_channel's convention
        limit = int(np.floor(kbps_per_channel * 1000.0 * cp.nChannels * view.n_frames * 1024 / cp.sampleRate / 8.0))
    if limit < 0:
        raise ValueError(f"max_bytes = {max_bytes} is smaller than the file's header ({len(head)} bytes)")
    return limit


def segment_limits(kbps_per_channel, n_channels, sample_rate, blocks, segment_hops):
    """The segments of encode_stream_abr(segment_hops=...): `blocks` blocks cut into consecutive stretches of
    segment_hops blocks, the last may be shorter.  -> int64 arrays (first_block, blocks, limit_bytes) per segment,
    limit = floor(kbps * 1000 * nCh * blocks_in_segment * 1024 / sampleRate / 8): the whole-stream convention per
    segment, so the limits sum to at most the whole-stream limit.  Pure arithmetic."""
    hops, blocks = int(segment_hops), int(blocks)
    if hops != segment_hops or hops < 1:
        raise ValueError(f"segment_hops = {segment_hops!r}: a whole number of blocks, at least 1")
    if not kbps_per_channel > 0:
        raise ValueError("kbps_per_channel must be positive")
    first = np.arange(0, max(blocks, 1), hops, dtype=np.int64)
    count = np.minimum(first + hops, blocks) - first
    limit = np.array([int(np.floor(kbps_per_channel * 1000.0 * n_channels * int(c) * 1024 / sample_rate / 8.0))
                      for c in count], np.int64)
    return first, count.astype(np.int64), limit


def _abr_range(nmr_range_db):
    try:
        lo, hi = (float(v) for v in nmr_range_db)
    except (TypeError, ValueError):
        raise ValueError("nmr_range_db: (lowest, highest) target in dB") from None
    grid = _lib.RATE_TARGET_GRID
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi or lo * grid != np.floor(lo * grid) or \
            hi * grid != np.floor(hi * grid):
        raise ValueError(f"nmr_range_db = {nmr_range_db}: finite, lowest <= highest, multiples of 1/{grid} dB")
    return lo, hi


def _unreachable(limit, total, hi, head):
    """what an average-rate call says when even the highest target of its range does not fit"""
    return (f"a body of {limit} bytes cannot be reached: at the highest target, {hi:g} dB, it takes "
            f"{total} bytes ({len(head) + total} with the header), the "
            f"smallest size this range of targets gives")


def _segment_unreachable(s, first, count, seg_limit, total, hi):
    """what a segmented average-rate call says of the first segment that even the highest target does not fit"""
    return (f"segment {s} (from block {int(first[s])}, {int(count[s])} blocks) cannot be reached: "
            f"its limit is {int(seg_limit[s])} bytes and at the highest target, {hi:g} dB, it "
            f"takes {int(total)} bytes, the smallest size this range of targets "
            f"gives")


def _segment_over_peak(s, first, count, seg_limit, total, floor, hi, stream_target):
    """what a peak call says of the first segment beyond its peak at its final target"""
    unmet = (f"segment {s} (from block {int(first[s])}, {int(count[s])} blocks) exceeds its peak of "
             f"{int(seg_limit[s])} bytes: it takes {int(total)} bytes; ")
    unmet += (f"it cannot be reached at all: its floor is the highest target, {hi:g} dB, the smallest size "
              f"this range of targets gives") if floor == hi else \
        (f"it fits at its own floor, {floor:g} dB, but not at the stream's target, "
         f"{stream_target:g} dB (its bytes rise with the target there)")
    return unmet


def _check_segment_keywords(segment_hops, peak_kbps_per_channel, sizes):
    """segment_hops and peak_kbps_per_channel against the sizes [(kbps_per_channel, max_bytes)], before any GPU work"""
    peak = peak_kbps_per_channel is not None
    _check_peak(peak_kbps_per_channel, segment_hops)
    if segment_hops is not None:
        if not peak and any(b is not None for _, b in sizes):
            raise ValueError("segment_hops goes with kbps_per_channel: max_bytes is the size of a file, not of a segment")
        if not peak and any(k is None for k, _ in sizes):
            raise ValueError("give exactly one of kbps_per_channel and max_bytes")
        segment_limits(1.0, 1, 1, 1, segment_hops)              # a bad segment_hops before any GPU work
    return peak


def _check_peak(peak_kbps_per_channel, segment_hops):
    """the peak_kbps_per_channel keyword, before any GPU work"""
    if peak_kbps_per_channel is None:
        return
    if segment_hops is None:
        raise ValueError("peak_kbps_per_channel goes with segment_hops: a peak is the rate of a segment")
    if not peak_kbps_per_channel > 0:
        raise ValueError("peak_kbps_per_channel must be positive")


def _encode_stream_abr(pcm, sample_rate, sizes, max_kbps_per_channel, block_switching, header_samples, nmr_range_db,
                       allocation="budget", segment_hops=None, peak_kbps_per_channel=None, use_vq=False):
    """One curve, one solve + second pass per size.  sizes: list of (kbps_per_channel, max_bytes).
    -> list of (.pac bytes, solve dict, outputs of encode_pack_budget -- allocation "band": of encode_pack_alloc --,
    body limit), the encoder.  segment_hops: one segmented solve per size instead; the solve dict is
    Encoder.rate_solve_segments' / band_solve_segments' plus "segments" (first_block, blocks, limit_bytes per segment),
    the body limit the sum of the segments'.  peak_kbps_per_channel: one peak solve per size (Encoder.rate_solve_peak /
    band_solve_peak): the size is the stream's and the body limit, the segments' limit_bytes are the peaks.
    use_vq (allocation "band" only): the gain-shape coder -- Encoder.vq_band_curve, the solves on the scalar sibling,
    the outputs of encode_vq_alloc; the encoder returned is the gain-shape one."""
    band = _check_allocation(allocation)
    if use_vq and not band:
        raise NotImplementedError("gain-shape streams: allocation 'band' only")
    lo, hi = _abr_range(nmr_range_db)
    peak = _check_segment_keywords(segment_hops, peak_kbps_per_channel, sizes)
    cp, enc, view, flags = _rate_stream_setup(pcm, sample_rate, max_kbps_per_channel, block_switching, header_samples,
                                              use_vq)
    head = header_bytes(cp)
    limits = [None] * len(sizes) if segment_hops is not None and not peak else \
        [_abr_limit(cp, view, head, k, b) for k, b in sizes]
    path = _PATHS[allocation](enc)
    curve = path.curve(view, flags, cp.targetBitsPerSample)
    n_ch = cp.nChannels

    def unreachable(limit, total):
        return _unreachable(limit, total, hi, head)

    done = []
    for (kbps, _), limit in zip(sizes, limits):
        if segment_hops is None:        # the whole stream: the partition [0, n_cf] with its one limit, the plain method
            sol = path.solve(curve, flags, limit, lo, hi)
            unmet = None if sol["met"] else unreachable(limit, sol["total_bytes"])
        elif peak:                      # the stream's limit above the segments' peaks
            first, count, seg_limit = segment_limits(peak_kbps_per_channel, n_ch, cp.sampleRate, view.n_frames,
                                                     segment_hops)
            seg_first = np.append(first, view.n_frames) * n_ch
            sol = path.solve_peak(curve, seg_first, seg_limit, limit, lo, hi)
            s = int(np.argmin(sol["met"]))
            if not sol["stream_met"]:
                unmet = unreachable(limit, sol["stream_total_bytes"])
            elif sol["met"].all():
                unmet = None
            else:
                unmet = _segment_over_peak(s, first, count, seg_limit, sol["total_bytes"][s], sol["floor_nmr_db"][s], hi,
                                           sol["stream_target_nmr_db"])
            sol["segments"] = {"first_block": first, "blocks": count, "limit_bytes": seg_limit}
        else:
            first, count, seg_limit = segment_limits(kbps, n_ch, cp.sampleRate, view.n_frames, segment_hops)
            seg_first = np.append(first, view.n_frames) * n_ch
            sol = path.solve_segments(curve, seg_first, seg_limit, lo, hi)
            s = int(np.argmin(sol["met"]))
            unmet = None if sol["met"].all() else \
                _segment_unreachable(s, first, count, seg_limit, sol["total_bytes"][s], hi)
            sol["segments"] = {"first_block": first, "blocks": count, "limit_bytes": seg_limit}
            limit = int(seg_limit.sum())
        if unmet:
            raise ValueError(unmet)
        out = path.second_pass(view, flags, sol)
        body, total = enc.gather_body(out["payload"], out["n_bytes"])
        done.append((head + body[:int(total.item())].cpu().numpy().tobytes(), sol, out, limit))
    return done, enc


def encode_stream_abr(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, max_kbps_per_channel=320,
                      block_switching=False, header_samples=None, nmr_range_db=(-30, 30), use_vq=False, use_sbr=False,
                      chunk_hops=None, n_lines=1024, allocation="budget", segment_hops=None,
                      peak_kbps_per_channel=None):
    """Whole-stream encode to an average bit rate -> .pac bytes: the best constant quality that fits a size.  One
    target NMR for the whole stream, the smallest on the grid of 1/64 dB in nmr_range_db (by the bisection of
    include/pacx.h, pacx_rate_solve) at which the stream of encode_stream_nmr(target) stays within the size; the
    bytes are that call's.  Give exactly one size:
      kbps_per_channel  the body (records and their length prefixes) takes at most
                        floor(kbps * 1000 * nCh * blocks * 1024 / sampleRate / 8) bytes, blocks = the n + 2 blocks the
                        driver writes;
      max_bytes         the whole file, header included.
    max_kbps_per_channel caps every block as in encode_stream_nmr.  ValueError when even the highest target of the
    range does not fit; the message names the smallest size reachable.  The rate-distortion curve of every block is
    taken once (Encoder.rate_curve), the solve reads only that (Encoder.rate_solve), the second pass is
    Encoder.encode_pack_budget: quality.rate_curve gives the curve for several sizes.  Scalar mantissas, 1024 lines,
    one batch, as encode_stream_nmr.
    allocation="band": the stream of encode_stream_nmr(target, allocation="band") instead, on Encoder.band_curve,
    band_solve and encode_pack_alloc; wherever no block reaches its cap the target found is the lowest on the grid
    that fits (include/pacx.h).
    segment_hops=S (S >= 1, with kbps_per_channel only): an average bit rate per segment instead of per stream.  The
    n + 2 blocks the driver writes are cut into consecutive segments of S blocks (the last may be shorter), every
    segment gets the limit of segment_limits() -- the convention above for its own blocks -- and the lowest target on
    the grid at which its own records fit (pacx_rate_solve_segments / pacx_band_solve_segments: one curve, one solve
    for all segments, one second pass).  The records of a segment are those of encode_stream_nmr at that segment's
    target.  ValueError when a segment cannot be reached; the message names the first such segment, its first block,
    its limit and the bytes it takes at the highest target.
    peak_kbps_per_channel=P (P > 0, with segment_hops=S): constrained VBR -- the size, kbps_per_channel or max_bytes
    (a file size is meaningful here), is the whole stream's as without segments, and segment_limits(P, ...) gives every
    segment a peak.  Every segment that fits its peak at the stream's target takes the stream's target; one that does
    not is pinned to its floor, the lowest target at which it fits, and what it gives up the others spend
    (pacx_rate_solve_peak / pacx_band_solve_peak: one curve, one solve, one second pass).  ValueError when the stream's
    size cannot be reached (the message above) or a segment exceeds its peak at its final target; the message names
    the first such segment, its first block, its peak and its bytes, and says whether the segment cannot be reached at
    all or fits at its own floor but not at the stream's target (where its bytes are not monotone in the target)."""
    _check_allocation(allocation)
    if use_vq or use_sbr or chunk_hops or int(n_lines) != 1024:
        raise NotImplementedError("average-bit-rate streams: scalar mantissas, nMDCTLines 1024, one batch")
    done, _ = _encode_stream_abr(pcm, sample_rate, [(kbps_per_channel, max_bytes)], max_kbps_per_channel,
                                 block_switching, header_samples, nmr_range_db, allocation, segment_hops,
                                 peak_kbps_per_channel)
    return done[0][0]


Bucket = namedtuple("Bucket", "drain_q16 size_bytes start_q16")         # pacx_bucket (include/pacx_bucket.h)


def bucket(kbps_per_channel, n_channels, sample_rate, buffer_bytes, start_bytes=0, hop=1024):
    """The leaky bucket of a decoder or a transport that takes kbps_per_channel out of a buffer of buffer_bytes -> the
    pacx_bucket triple Bucket(drain_q16, size_bytes, start_q16), levels in 1 / 65536 byte (Encoder.bucket_scan,
    rate_solve_bucket, band_solve_bucket).  drain_q16 = floor(kbps * 1000 * nCh * hop * 65536 / (8 * sampleRate)), what
    leaves per block of `hop` samples, in exact rational arithmetic (kbps_per_channel: an int, a Fraction, a string as
    Fraction takes it, or a float, taken at its exact value): the floor never drains more than the rate does, so a
    stream that fits this bucket fits the real one.  start_bytes: the level before the first block, at most
    buffer_bytes.  Pure arithmetic."""
    try:
        kbps, start = Fraction(kbps_per_channel), Fraction(start_bytes)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError("kbps_per_channel and start_bytes are numbers") from None
    for name, v in (("n_channels", n_channels), ("sample_rate", sample_rate), ("hop", hop)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f"{name} = {v!r}: a whole number, at least 1")
    if kbps < 0:
        raise ValueError("kbps_per_channel must not be negative")
    if isinstance(buffer_bytes, bool) or int(buffer_bytes) != buffer_bytes or not 0 <= buffer_bytes <= _lib.BUCKET_SIZE_MAX:
        raise ValueError(f"buffer_bytes = {buffer_bytes!r}: a whole number of bytes in [0, 2^40]")
    if not 0 <= start <= buffer_bytes:
        raise ValueError(f"start_bytes = {start_bytes!r}: a level in [0, buffer_bytes]")
    one = 1 << _lib.BUCKET_Q
    drain = kbps * 1000 * int(n_channels) * int(hop) * one / (8 * int(sample_rate))
    if drain >= 1 << 63:
        raise ValueError(f"kbps_per_channel = {kbps_per_channel!r}: the drain of a block does not fit 64 bits")
    return Bucket(floor(drain), int(buffer_bytes), floor(start * one))


def _buffer_overflows(b, first_over, level_q16, limit, total, hi):
    """what a buffered average-rate call says when the size fits at the highest target of its range and the buffer
    does not: the first block above the buffer and its level, in whole bytes rounded up"""
    return (f"a buffer of {b.size_bytes} bytes cannot be met: at the highest target, {hi:g} dB, the body fits its "
            f"limit ({total} of {limit} bytes) but block {first_over} brings the level to "
            f"{-(-level_q16 >> _lib.BUCKET_Q)} bytes, the first block above the buffer")


def _encode_stream_buffered(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel, start_bytes,
                            max_kbps_per_channel, block_switching, header_samples, nmr_range_db, allocation, use_vq,
                            pinned=None):
    """encode_stream_abr_buffered, or with pinned = (pin_step_db, max_phases) encode_stream_abr_pinned -> (.pac bytes,
    the solve's dict, the second pass's outputs, the body limit, the bucket, the encoder)"""
    band = _check_allocation(allocation)
    if use_vq and not band:
        raise NotImplementedError("gain-shape streams: allocation 'band' only")
    lo, hi = _abr_range(nmr_range_db)
    if pinned is not None:
        Encoder._pin_args("encode_stream_abr_pinned", *pinned)
    if not kbps_per_channel > 0:
        raise ValueError("kbps_per_channel must be positive")
    pcm = np.ascontiguousarray(pcm)
    if pcm.ndim != 2:
        raise ValueError("pcm: int16 [samples, channels]")
    b = bucket(kbps_per_channel if drain_kbps_per_channel is None else drain_kbps_per_channel, pcm.shape[1],
               sample_rate, buffer_bytes, start_bytes)
    cp, enc, view, flags = _rate_stream_setup(pcm, sample_rate, max_kbps_per_channel, block_switching, header_samples,
                                              use_vq)
    head = header_bytes(cp)
    limit = _abr_limit(cp, view, head, kbps_per_channel, None)
    path = _PATHS[allocation](enc)
    curve = path.curve(view, flags, cp.targetBitsPerSample)
    sol = path.solve_bucket(curve, flags, cp.nChannels, limit, b, lo, hi, pinned)
    if not sol["met"] and sol["total_bytes"] > limit:
        raise ValueError(_unreachable(limit, sol["total_bytes"], hi, head))
    if not sol["met"]:
        over = sol["bucket"]["first_over"]
        level = path.solver.bucket_scan(sol["n_bytes"], cp.nChannels, b, want_level=True)["level"]
        raise ValueError(_buffer_overflows(b, over, int(level[over].item()), limit, sol["total_bytes"], hi))
    out = path.second_pass(view, flags, sol)
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    return head + body[:int(total.item())].cpu().numpy().tobytes(), sol, out, limit, b, enc


def encode_stream_abr_buffered(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel=None,
                               start_bytes=0, max_kbps_per_channel=320, block_switching=False, header_samples=None,
                               nmr_range_db=(-30, 30), allocation="budget", use_vq=False):
    """encode_stream_abr(kbps_per_channel) for a decoder with a buffer -> .pac bytes: one target NMR for the whole
    stream, found by the same bisection on the grid of 1/64 dB in nmr_range_db, at which the body stays within
    kbps_per_channel's size AND the stream plays through a leaky bucket (include/pacx_bucket.h, pacx_bucket_scan): every block's
    records, their length prefixes included, arrive in a buffer of buffer_bytes that starts at start_bytes, and
    drain_kbps_per_channel (default: kbps_per_channel) leaves it per block, bucket() says how much exactly; the level
    right after a block arrives never exceeds buffer_bytes.  The bytes are encode_stream_nmr's at the target found
    (allocation as there), with use_vq=True encode_stream_vq_nmr's (allocation "band" only).  Unlike segment_hops=, the
    constraint has no grid: a burst is refused exactly when the buffer cannot absorb it, wherever it lies.  One curve,
    one solve (Encoder.rate_solve_bucket / band_solve_bucket, on the scalar sibling for gain-shape streams), one
    second pass.  ValueError when even the highest target of the range does not give both: encode_stream_abr's message
    if the size does not fit there, else one that names the first block above the buffer, its level and the buffer.
    A target is one for the whole stream: the loudest stretch the buffer cannot absorb sets the quality of all of it."""
    return _encode_stream_buffered(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel, start_bytes,
                                   max_kbps_per_channel, block_switching, header_samples, nmr_range_db, allocation,
                                   use_vq)[0]


def encode_stream_abr_pinned(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel=None,
                             start_bytes=0, max_kbps_per_channel=320, block_switching=False, header_samples=None,
                             nmr_range_db=(-30, 30), allocation="budget", use_vq=False, pin_step_db=1.0, max_phases=8):
    """encode_stream_abr_buffered with a target per block -> .pac bytes: the size and the leaky bucket are that call's,
    word for word, but only the blocks the buffer binds pay for it.  The stream's target holds wherever the buffer
    allows; a stretch of blocks that would overflow it at that target is pinned at a higher one, phase by phase
    (include/pacx_bucket_pin.h: Encoder.rate_solve_bucket_pinned / band_solve_bucket_pinned, on the scalar sibling for
    gain-shape streams): a pinned block lies within pin_step_db (a multiple of 1/64 dB) of the lowest level at which
    its stretch fits, and at most max_phases (1 ... 16) levels are pinned -- with max_phases=1 the stream is
    encode_stream_abr_buffered's, with a buffer nothing reaches encode_stream_abr's.  No block ends above the one
    target of encode_stream_abr_buffered; the assignment written was measured to fit.  Every block is coded as
    encode_stream_nmr codes it at that block's target (allocation as there).  One curve, one solve, one second pass.
    ValueError as encode_stream_abr_buffered raises it, in the same words."""
    return _encode_stream_buffered(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel, start_bytes,
                                   max_kbps_per_channel, block_switching, header_samples, nmr_range_db, allocation,
                                   use_vq, (pin_step_db, max_phases))[0]


class _Blocks:
    """what _abr_limit reads of a PCM view: the blocks the driver writes"""

    def __init__(self, n_frames):
        self.n_frames = n_frames


def _abr_chunked_setup(pcm, sample_rate, chunk_hops, max_kbps_per_channel, block_switching, header_samples,
                       nmr_range_db, use_vq, allocation="band"):
    """everything encode_stream_abr_chunked refuses, before any GPU work -> (CodingParams, header bytes, make), make()
    -> the streaming.HostStreamRateEncoder of the call"""
    from .engine import Encoder
    if use_vq and not _check_allocation(allocation):
        raise NotImplementedError("gain-shape streams: allocation 'band' only")
    try:
        hops = int(chunk_hops)
    except (TypeError, ValueError):
        hops = 0
    if isinstance(chunk_hops, bool) or hops != chunk_hops or hops < 1:
        raise ValueError(f"chunk_hops = {chunk_hops!r}: a whole number of blocks, at least 1")
    lo, hi = _abr_range(nmr_range_db)
    Encoder._profile_len("nmr_range_db", lo, hi)
    cp = _rate_coding_params(pcm, sample_rate, max_kbps_per_channel, header_samples, use_vq)
    if len(pcm) == 0:
        raise ValueError("pcm: at least one block of 1024 samples")

    def make():
        from .streaming import HostStreamRateEncoder
        return HostStreamRateEncoder(context.encoder_for_params(cp), cp.nChannels, hops, cp.targetBitsPerSample,
                                     block_switching=block_switching, nmr_lo_db=lo, nmr_hi_db=hi, allocation=allocation)
    return cp, header_bytes(cp), make


def iter_encode_abr_chunked(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, chunk_hops=4096,
                            max_kbps_per_channel=320, block_switching=False, header_samples=None,
                            nmr_range_db=(-30, 30), use_vq=False, segment_hops=None, peak_kbps_per_channel=None,
                            allocation="band"):
    """encode_stream_abr_chunked piece by piece: an iterator that gives the file's header, then the bodies of the
    chunks in order (bytes; their concatenation is that call's result).  The arguments are checked, the stream is
    analysed and the target solved when this is called; the second pass runs as the iterator is consumed.
    With peak_kbps_per_channel one error can come from the ITERATOR instead: a segment that fits its peak at its own
    floor but whose bytes rise with the target (encode_stream_abr_chunked explains); the pieces before the chunk in
    which that segment ends have been handed out by then."""
    return _iter_encode_abr(pcm, sample_rate, kbps_per_channel, max_bytes, chunk_hops, max_kbps_per_channel,
                            block_switching, header_samples, nmr_range_db, use_vq, segment_hops, peak_kbps_per_channel,
                            allocation, None)


def _kept_bytes_per_cf(cp, allocation):
    """_BandPath / _BudgetPath.kept_bytes_per_cf from the CodingParams alone (header_bytes has set the band tables), so
    that a caller's store is refused before an encoder exists: the kind's bytes at the handle's band_stride, or at the
    row of pacx_rate_curve_layout (the budget rule of coder/codec.py:288-299 at the cap rate, in steps of 32 bits)"""
    nb_long, nb_short = cp.sfBands.nBands, cp.sfBandsShort.nBands
    if allocation == "band":
        return curves.BAND.kept_bytes_per_cf(max(nb_long, _lib.SUB * nb_short))

    def steps(half_n, short, last_or_next, nb):
        n_eff = int(1.45 * half_n) if short else half_n
        if last_or_next:
            n_eff = int(0.85 * n_eff)
        cap = cp.targetBitsPerSample * float(n_eff) - float(cp.nScaleBits * (nb + 1)) - float(cp.nMantSizeBits * nb)
        return min(max(int(np.floor(cap / 32.0)), 0), 2047)
    j_long = max(steps(1024, False, lon, nb_long) for lon in (False, True))
    j_short = max(steps(128, True, lon, nb_short) for lon in (False, True))
    return curves.RATE.kept_bytes_per_cf(max(j_long + 1, _lib.SUB * (j_short + 1)))


def _iter_encode_abr(pcm, sample_rate, kbps_per_channel, max_bytes, chunk_hops, max_kbps_per_channel, block_switching,
                     header_samples, nmr_range_db, use_vq, segment_hops, peak_kbps_per_channel, allocation, keep):
    """iter_encode_abr_chunked (keep None) and iter_encode_abr_kept (keep = (curve_store,)): one implementation"""
    _check_allocation(allocation)
    peak = _check_segment_keywords(segment_hops, peak_kbps_per_channel, [(kbps_per_channel, max_bytes)])
    cp, head, make = _abr_chunked_setup(pcm, sample_rate, chunk_hops, max_kbps_per_channel, block_switching,
                                        header_samples, nmr_range_db, use_vq, allocation)
    blocks = len(pcm) // 1024 + 2
    if segment_hops is None or peak:
        limit = _abr_limit(cp, _Blocks(blocks), head, kbps_per_channel, max_bytes)
    if segment_hops is not None:
        first, count, seg_limit = segment_limits(peak_kbps_per_channel if peak else kbps_per_channel, cp.nChannels,
                                                 cp.sampleRate, blocks, segment_hops)
    if keep is not None and keep[0] is not None:                       # refused here: no encoder yet
        from .streaming import HostStreamRateEncoder
        HostStreamRateEncoder.check_store(keep[0], blocks * cp.nChannels * _kept_bytes_per_cf(cp, allocation),
                                          "curve_store")
    hr = make()
    if keep is not None:
        hr.keep_curves(keep[0])
    check = None
    if segment_hops is None:
        hr.analyse(pcm)
        sol = hr.solve(limit)
        if not sol["met"]:
            raise ValueError(_unreachable(limit, sol["total_bytes"], hr.hi, head))
        targets = sol["target_nmr_db"]
    elif not peak:
        hr.analyse(pcm, segment_hops=segment_hops, segment_limits=seg_limit)
        sol = hr.solve_segments()
        if not sol["met"].all():
            s = int(np.argmin(sol["met"]))
            raise ValueError(_segment_unreachable(s, first, count, seg_limit, sol["total_bytes"][s], hr.hi))
        targets = sol["target_nmr_db"]
    else:
        hr.analyse(pcm, segment_hops=segment_hops, segment_limits=seg_limit, peak=True)
        sol = hr.solve_peak(limit)
        if not sol["stream_met"]:
            raise ValueError(_unreachable(limit, sol["stream_total_bytes"], hr.hi, head))
        targets = sol["target_nmr_db"]

        def over_peak(s, total):
            return _segment_over_peak(s, first, count, seg_limit, total, sol["floor_nmr_db"][s], hr.hi,
                                      sol["stream_target_nmr_db"])
        # a segment that cannot be reached is beyond its peak for certain; a reachable one whose size somewhere above
        # its floor exceeds the peak may be (its row is gone): the first of those, if it comes earlier, decides in
        # the second pass which segment is named
        doubtful = sol["floor_met"] & (sol["worst_above"] > seg_limit)
        if not sol["floor_met"].all():
            s = int(np.argmin(sol["floor_met"]))
            if not doubtful[:s].any():
                raise ValueError(over_peak(s, sol["floor_total_bytes"][s]))
        check = over_peak if doubtful.any() else None

    def parts():
        from .streaming import SegmentOverLimit
        yield head
        try:
            if segment_hops is None:
                bodies = hr.encode(pcm, targets)
            else:
                bodies = hr.encode(pcm, targets, segment_hops=segment_hops,
                                   segment_limits=seg_limit if check else None)
            for body in bodies:
                yield body.tobytes()
        except SegmentOverLimit as e:
            raise ValueError(check(e.segment, e.total_bytes)) from None
    return parts()


def encode_stream_abr_chunked(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, chunk_hops=4096,
                              max_kbps_per_channel=320, block_switching=False, header_samples=None,
                              nmr_range_db=(-30, 30), use_vq=False, segment_hops=None, peak_kbps_per_channel=None,
                              allocation="band"):
    """encode_stream_abr(allocation="band") for a stream too long for one batch -> the same .pac bytes, from host
    memory to host memory in chunks of chunk_hops blocks, with device memory bounded by the chunk.  pcm: anything that
    slices to int16 [n, nCh] pieces (an np.memmap included), n a multiple of 1024 and at least 1024.  Two passes
    (streaming.HostStreamRateEncoder): per chunk the band curve and its size at EVERY target of nmr_range_db, added
    into one profile (Encoder.band_profile; at most 128 dB of range); the solve of encode_stream_abr read from that
    profile (Encoder.profile_solve); then per chunk curve, pick at the target found and second pass.  The sizes
    (kbps_per_channel or max_bytes), max_kbps_per_channel and the ValueError when even the highest target does not fit
    are encode_stream_abr's.  use_vq: the gain-shape coder without SBR, the bytes of encode_stream_vq_abr.
    iter_encode_abr_chunked gives the same bytes piece by piece.
    allocation="budget": the bytes of encode_stream_abr(allocation="budget") -- that call's default -- instead, by the
    same two passes on the rate curve (Encoder.rate_curve, rate_profile[_segments], rate_pick[_segments],
    encode_pack_budget), with segment_hops and peak_kbps_per_channel as below; not with use_vq (NotImplementedError).
    segment_hops=S and peak_kbps_per_channel=P mean what they mean for encode_stream_abr, under its rules, with its
    bytes and its error messages: the first pass keeps a profile row per segment the chunk touches
    (Encoder.band_profile_segments), solves and drops the rows of the segments that end in it
    (profile_solve_segments) and, with a peak, adds them clamped at their floors into the stream's profile
    (profile_clamp_add), on which the stream's solve is the peak solve's; the second pass picks per segment
    (band_pick_segments).  A segment that cannot be reached and a stream size that cannot be reached are refused
    before any byte is produced.  One case is found only in the second pass: a segment that fits its peak at its floor
    but not at the stream's target, because its bytes rise with the target there -- its row is gone by the time the
    stream's target is known.  The second pass then sums the records of every segment and raises encode_stream_abr's
    message when the first offending segment ends; this call returns nothing in that case, the iterator form has
    handed out the pieces before."""
    return b"".join(iter_encode_abr_chunked(pcm, sample_rate, kbps_per_channel, max_bytes, chunk_hops,
                                            max_kbps_per_channel, block_switching, header_samples, nmr_range_db, use_vq,
                                            segment_hops, peak_kbps_per_channel, allocation))


def iter_encode_abr_kept(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, chunk_hops=4096,
                         max_kbps_per_channel=320, block_switching=False, header_samples=None, nmr_range_db=(-30, 30),
                         use_vq=False, segment_hops=None, peak_kbps_per_channel=None, allocation="band",
                         curve_store=None):
    """encode_stream_abr_kept piece by piece, as iter_encode_abr_chunked gives encode_stream_abr_chunked's."""
    return _iter_encode_abr(pcm, sample_rate, kbps_per_channel, max_bytes, chunk_hops, max_kbps_per_channel,
                            block_switching, header_samples, nmr_range_db, use_vq, segment_hops, peak_kbps_per_channel,
                            allocation, (curve_store,))


def encode_stream_abr_kept(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, chunk_hops=4096,
                           max_kbps_per_channel=320, block_switching=False, header_samples=None, nmr_range_db=(-30, 30),
                           use_vq=False, segment_hops=None, peak_kbps_per_channel=None, allocation="band",
                           curve_store=None):
    """encode_stream_abr_chunked with every chunk's curve taken ONCE -> the same .pac bytes, the same refusals and
    error messages.  The first pass writes each chunk's curve out as 16-bit thresholds (Encoder.band_thresholds /
    rate_thresholds, include/pacx.h: what a pick at a grid target of nmr_range_db reads of the curve -- a quarter of a
    band curve's bytes, half of a rate curve's, about as many per channel-frame as the PCM itself) and copies them down
    behind the kernels; the second pass sends them up behind the PCM and picks from them
    (Encoder.band_pick_thresholds[_segments] / rate_pick_thresholds[_segments]) instead of taking the curve again
    (streaming.HostStreamRateEncoder.keep_curves).  Device memory stays bounded by the chunk; host memory holds
    HostStreamRateEncoder.kept_bytes(len(pcm) // 1024) bytes between the passes.
    curve_store=None: that memory is made by the call; else a writable C-contiguous uint8 buffer of at least that many
    bytes, for instance an np.memmap over a scratch file (ValueError before any GPU work otherwise).  The other
    parameters are encode_stream_abr_chunked's, in its order.  The curve is the expensive part of a chunk for
    gain-shape streams and for allocation="budget" (README has the figures)."""
    return b"".join(iter_encode_abr_kept(pcm, sample_rate, kbps_per_channel, max_bytes, chunk_hops,
                                         max_kbps_per_channel, block_switching, header_samples, nmr_range_db, use_vq,
                                         segment_hops, peak_kbps_per_channel, allocation, curve_store))


def iter_encode_abr_buffered_kept(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel=None,
                                  start_bytes=0, max_kbps_per_channel=320, block_switching=False, header_samples=None,
                                  nmr_range_db=(-30, 30), allocation="budget", use_vq=False, chunk_hops=4096,
                                  curve_store=None, levels=4):
    """encode_stream_abr_buffered_kept piece by piece: the file's header, then the bodies of the chunks in order.  The
    arguments are checked, the stream is analysed and the target solved when this is called; the second pass runs as
    the iterator is consumed."""
    from .streaming import HostStreamRateEncoder
    # encode_stream_abr_buffered's refusals, in its order; then the chunked call's and the store's: no encoder yet
    band = _check_allocation(allocation)
    if use_vq and not band:
        raise NotImplementedError("gain-shape streams: allocation 'band' only")
    _abr_range(nmr_range_db)
    if not kbps_per_channel > 0:
        raise ValueError("kbps_per_channel must be positive")
    if pcm.ndim != 2:
        raise ValueError("pcm: int16 [samples, channels]")
    b = bucket(kbps_per_channel if drain_kbps_per_channel is None else drain_kbps_per_channel, pcm.shape[1],
               sample_rate, buffer_bytes, start_bytes)
    cp, head, make = _abr_chunked_setup(pcm, sample_rate, chunk_hops, max_kbps_per_channel, block_switching,
                                        header_samples, nmr_range_db, use_vq, allocation)
    levels = Encoder._tree_levels("levels", levels)
    blocks = len(pcm) // 1024 + 2
    limit = _abr_limit(cp, _Blocks(blocks), head, kbps_per_channel, None)
    if curve_store is not None:
        HostStreamRateEncoder.check_store(curve_store, blocks * cp.nChannels * _kept_bytes_per_cf(cp, allocation),
                                          "curve_store")
    hr = make()
    hr.keep_curves(curve_store).analyse(pcm)
    sol = hr.solve_bucket(limit, b, levels)
    if not sol["met"] and sol["total_bytes"] > limit:
        raise ValueError(_unreachable(limit, sol["total_bytes"], hr.hi, head))
    if not sol["met"]:
        # the one thing the message needs that the solve does not carry: the level at the first block above the buffer
        over = sol["bucket"]["first_over"]
        raise ValueError(_buffer_overflows(b, over, hr.level_at(hr.hi, b, over), limit, sol["total_bytes"], hr.hi))

    def parts():
        yield head
        for body in hr.encode(pcm, sol["target_nmr_db"], use_kept=True):
            yield body.tobytes()
    return parts()


def encode_stream_abr_buffered_kept(pcm, sample_rate, kbps_per_channel, buffer_bytes, drain_kbps_per_channel=None,
                                    start_bytes=0, max_kbps_per_channel=320, block_switching=False, header_samples=None,
                                    nmr_range_db=(-30, 30), allocation="budget", use_vq=False, chunk_hops=4096,
                                    curve_store=None, levels=4):
    """encode_stream_abr_buffered for a stream too long for one batch -> the same .pac bytes, the same two ValueErrors
    in the same words, from host memory to host memory in chunks of chunk_hops blocks with every chunk's curve taken
    once.  The parameters are encode_stream_abr_buffered's, in its order, then encode_stream_abr_kept's chunk_hops and
    curve_store, and levels.  pcm: anything that slices to int16 [n, nCh] pieces (an np.memmap included), n a multiple
    of 1024 and at least 1024.  The first pass keeps every chunk's curve as 16-bit thresholds
    (streaming.HostStreamRateEncoder.keep_curves, analyse); the solve walks the kept chunks once per `levels`
    decisions of encode_stream_abr_buffered's bisection (HostStreamRateEncoder.solve_bucket,
    include/pacx_bucket_kept.h: 13, 7, 5, 4, 3 passes over the store for levels 1 ... 5 on the default range, the PCM
    untouched); the second pass picks from the kept curves at the target found.  Device memory stays bounded by the
    chunk.  The chunked call's refusals (chunk_hops, a range above 128 dB, an empty stream) and a curve_store that is
    too small, read-only or not uint8 are raised before any GPU work.  iter_encode_abr_buffered_kept gives the same
    bytes piece by piece."""
    return b"".join(iter_encode_abr_buffered_kept(pcm, sample_rate, kbps_per_channel, buffer_bytes,
                                                  drain_kbps_per_channel, start_bytes, max_kbps_per_channel,
                                                  block_switching, header_samples, nmr_range_db, allocation, use_vq,
                                                  chunk_hops, curve_store, levels))


def encode_stream_vq_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel=320, block_switching=False,
                         header_samples=None):
    """encode_stream_nmr(allocation="band") for the gain-shape coder -> .pac bytes with useVQ set and useSBR clear:
    every band of every block gets the smallest size (0, 2, ..., 16 bits a line) at which the noise of the band AS THE
    DECODER RECONSTRUCTS IT stays at or below target_nmr_db of the masked threshold, no block above the budget of
    max_kbps_per_channel.  The curve is taken with the coder and the decoder themselves (Encoder.vq_band_curve,
    include/pacx.h: pacx_vq_band_curve_batch), the pick runs on the encoder's scalar sibling, the second pass is
    Encoder.encode_vq_alloc.  Every decoder of encode_stream(use_vq=True) output takes the stream.  Gain-shape without
    SBR, 1024 lines, one batch; the cap's limits are encode_stream_nmr's."""
    return _encode_stream_nmr(pcm, sample_rate, target_nmr_db, max_kbps_per_channel, block_switching, header_samples,
                              "band", use_vq=True)[0]


def encode_stream_vq_abr(pcm, sample_rate, kbps_per_channel=None, max_bytes=None, max_kbps_per_channel=320,
                         block_switching=False, header_samples=None, nmr_range_db=(-30, 30), segment_hops=None,
                         peak_kbps_per_channel=None):
    """encode_stream_abr(allocation="band") for the gain-shape coder: the stream of encode_stream_vq_nmr at the lowest
    target on the grid that fits the size.  kbps_per_channel / max_bytes, nmr_range_db, segment_hops and
    peak_kbps_per_channel mean what they mean there, with the same rules, limits and error messages (one
    implementation serves both); the solves are pacx_band_solve / _segments / _peak on the gain-shape curve."""
    done, _ = _encode_stream_abr(pcm, sample_rate, [(kbps_per_channel, max_bytes)], max_kbps_per_channel,
                                 block_switching, header_samples, nmr_range_db, "band", segment_hops,
                                 peak_kbps_per_channel, use_vq=True)
    return done[0][0]


def parse_header(data):
    """coder/pacfile.py:142-151 -> (CodingParams, header length)."""
    from struct import unpack, calcsize
    from .audiofile import CodingParams
    if data[:4] != b"PAC ":
        raise RuntimeError("Tried to read a non-PAC file into a PACFile object")
    fmt = "<LHLLHHHH"
    (sr, n_ch, n_samples, n_lines, n_scale, n_mant_size, use_sbr, use_vq) = unpack(fmt, data[4:4 + calcsize(fmt)])
    pos = 4 + calcsize(fmt)
    n_bands = unpack("<L", data[pos:pos + 4])[0]
    n_lines_band = unpack("<" + str(n_bands) + "H", data[pos + 4:pos + 4 + 2 * n_bands])
    cp = CodingParams()
    cp.sampleRate, cp.nChannels, cp.numSamples = sr, n_ch, n_samples
    cp.nMDCTLines = cp.nSamplesPerBlock = n_lines
    cp.nScaleBits, cp.nMantSizeBits = n_scale, n_mant_size
    cp.useSBR, cp.useVQ = bool(use_sbr), bool(use_vq)
    cp.sfBands = ScaleFactorBands(n_lines_band)
    cp.sfBandsShort = ScaleFactorBands(AssignMDCTLinesFromFreqLimits(128, sr))
    cp.targetBitsPerSample = 128 / (sr / 1000)            # not used by the decoder
    return cp, pos + 4 + 2 * n_bands


def record_chain(data, pos, max_record):
    """Walks the '<L nBytes' chain of a .pac body (sequential by nature) and returns the
    payload offsets and sizes.  Sizes come from the file, so they are checked before anything
    is handed to the GPU: the reference's reader raises when a block is cut short
    (coder/pacfile.py:200-205), and a record longer than any the coder writes is corrupt."""
    offs, sizes = [], []
    end = len(data)
    while pos < end:
        if pos + 4 > end:
            raise RuntimeError(_PARTIAL)
        n = int.from_bytes(data[pos:pos + 4], "little")
        if n < 1 or n > max_record or pos + 4 + n > end:
            raise RuntimeError(_PARTIAL + f" (record of {n} bytes at offset {pos})")
        offs.append(pos + 4)
        sizes.append(n)
        pos += 4 + n
    return offs, sizes


def _decode_blockwise(f):
    """the reference's decode loop (coder/pacfile.py:745-757) block by block through the PACFile mirror (function
    level: nMDCTLines other than 1024): yields int16 [nMDCTLines, nCh] per hop"""
    from .pcmfile import fraction_to_codes
    cp = f.ReadFileHeader()
    while True:
        block = f.ReadDataBlock(cp)
        if not block:
            break
        yield np.stack([fraction_to_codes(x) for x in block], axis=1).astype(np.int16)


def _reader(source):
    """read(n) over a bytes-like object (slices of it, no copy) or a binary file object"""
    if hasattr(source, "read"):
        return source.read
    view = memoryview(source).cast("B")
    at = [0]

    def read(n):
        piece = view[at[0]:at[0] + n]
        at[0] += len(piece)
        return piece
    return read


_stream_decoder = [None, None]      # (key, streaming.HostStreamDecoder) of the last iter_decode


def iter_decode(source, chunk_bytes=16 << 20, max_blocks=None, depth=2):
    """A .pac (bytes-like, or a binary file object positioned at its start) -> int16 [hops*1024, nCh] arrays,
    chunk by chunk: at most chunk_bytes of the body and max_blocks hops are on the device at a time
    (streaming.HostStreamDecoder; the records are found there, pacx_index_body) and a file object is read no
    more than one buffer ahead.  Their concatenation is decode_stream's array.  max_blocks None: what
    chunk_bytes holds at 128 bytes per record (a chunk of shorter records ends early; nothing is lost)."""
    for _, pcm, pinned in _iter_decode(source, chunk_bytes, max_blocks, depth):
        yield pcm.copy() if pinned else pcm                           # out of the pinned buffer, which a later chunk reuses


def _iter_decode(source, chunk_bytes, max_blocks, depth):
    """iter_decode's chunks as (CodingParams, array, array is a view of a pinned buffer)"""
    import io
    read = _reader(source)
    head = bytes(read(4 + 22 + 4))                                    # coder/pacfile.py:136-151
    if len(head) == 30:
        head += bytes(read(2 * int.from_bytes(head[-4:], "little")))
    cp, _ = parse_header(head)
    if cp.nMDCTLines != 1024 and not cp.useVQ and not cp.useSBR:
        f = PACFile("<memory>")
        f.fp = io.BytesIO(head + source.read() if hasattr(source, "read") else bytes(source))
        for pcm in _decode_blockwise(f):
            yield cp, pcm, False
        return
    from .streaming import HostStreamDecoder
    enc = context.encoder_for_params(cp)
    chunk_bytes = int(chunk_bytes)
    if max_blocks is None:
        max_blocks = max(1, chunk_bytes // (128 * cp.nChannels))
    key = (cp.nChannels, chunk_bytes, int(max_blocks), int(depth))
    hs = _stream_decoder[1]
    if _stream_decoder[0] != key or hs.enc is not enc or hs.in_use:
        # the last decoder's buffers are kept (pinning them costs as much as decoding a short file); a decoder that
        # another iter_decode is in the middle of is left alone
        if hs is None or not hs.in_use:
            _stream_decoder[:] = [None, None]
        hs = HostStreamDecoder(enc, cp.nChannels, chunk_bytes, max_blocks, depth=depth)
        if _stream_decoder[1] is None:
            _stream_decoder[:] = [key, hs]
    hs.in_use = True
    try:
        for pcm in hs.decode(read):
            yield cp, pcm, True
    finally:
        hs.in_use = False


def decode_stream(data, chunk_bytes=None, max_blocks=None, depth=2):
    """Whole .pac (bytes; scalar, gain-shape or gain-shape + SBR) -> int16 [n, nCh], batched on the GPU: what
    the reference's decode loop (coder/pacfile.py:745-757) writes as PCM.  chunk_bytes: in chunks of that many
    bytes through iter_decode (bounded memory, record index built on the device); None: the whole file in one
    batch, its length prefixes walked on the host."""
    import torch
    if chunk_bytes is not None:
        # np.concatenate(list(iter_decode(...))) with one copy per sample instead of two: every chunk goes from its
        # pinned buffer straight to its place in the result, sized from the header and grown if the body holds more
        out, n = None, 0
        for cp, pcm, _ in _iter_decode(data, chunk_bytes, max_blocks, depth):
            if out is None:
                most = (len(data) // (5 * cp.nChannels) + 2) * cp.nMDCTLines      # a record is five bytes at least
                guess = min(int(cp.numSamples) + 4 * cp.nMDCTLines, most)         # the header's word is only a hint
                out = np.empty((max(guess, len(pcm)), cp.nChannels), np.int16)
            if n + len(pcm) > len(out):
                out = np.concatenate((out[:n], np.empty((max(len(out), len(pcm)), out.shape[1]), np.int16)))
            out[n:n + len(pcm)] = pcm
            n += len(pcm)
        return out[:n] if out is not None else np.zeros((0, parse_header(data)[0].nChannels), np.int16)
    cp, pos = parse_header(data)
    if cp.nMDCTLines != 1024 and not cp.useVQ and not cp.useSBR:
        # function level: the reference's decode loop block by block through the PACFile mirror
        import io
        from .pcmfile import fraction_to_codes
        f = PACFile("<memory>")
        f.fp = io.BytesIO(bytes(data))
        cp = f.ReadFileHeader()
        out = []
        while True:
            block = f.ReadDataBlock(cp)
            if not block:
                break
            out.append(np.stack([fraction_to_codes(x) for x in block], axis=1))
        return np.concatenate(out).astype(np.int16) if out else np.zeros((0, cp.nChannels), np.int16)
    enc = context.encoder_for_params(cp)
    offs, sizes = record_chain(data, pos, enc.payload_stride)
    if len(offs) % cp.nChannels:
        raise RuntimeError(_PARTIAL)
    body = torch.frombuffer(bytearray(data) + bytearray(8), dtype=torch.uint8).to(enc.device)
    sizes_t = torch.tensor(sizes, dtype=torch.int32, device=enc.device)
    offs_t = torch.tensor(offs, dtype=torch.int64, device=enc.device)
    if cp.useVQ:
        out = enc.decode_vq(body, sizes_t, cp.nChannels, offsets=offs_t)
        st = int(out["status"].max().item()) if len(sizes) else 0
        if st & _ST_MALFORMED:
            raise RuntimeError(_PARTIAL)
        if st & _ST_VQ_UNDEFINED:
            raise RuntimeError(_VQ_UNDEFINED)
        return out["pcm"].cpu().numpy()
    codes = enc.unpack(body, sizes_t, offs_t)
    if len(sizes) and int(codes["status"].max().item()) & _ST_MALFORMED:
        raise RuntimeError(_PARTIAL)
    return _decode_scalar(enc, cp, codes).cpu().numpy()
