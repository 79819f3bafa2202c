"""Host memory to host memory: the encode path as a pipeline of fixed-size chunks.

The C ABI takes device pointers (include/pacx.h); a caller whose PCM sits in host memory -- the
reference's driver reads a WAV file hop by hop (coder/pacfile.py:716-757) -- pays two PCIe crossings
around every batch.  Serial on one stream that is 12.5 M channel-frames/s at 8192 channel-frames per
step; here the copies of chunk i+1 (PCM in) and of chunk i-1 (packed body out) overlap the kernels of
chunk i: three HIP streams, `depth` buffers of everything (pinned on the host side), stream-to-stream
events and NO host synchronisation inside the loop -- the host only waits when it takes a finished
body (round 2 measured this pipeline in tools/pcie_probe.py: 24.8 M cf/s at 131 072 cf per chunk, the
268 MB of PCM then cross at ~50 GB/s, which is the bound).

    hs = HostStreamEncoder(enc, n_channels=2, hops_per_chunk=65536)
    buf = hs.input(k)                # pinned int16 [nCh, hops_per_chunk * 1024]: fill it in place (zero copy) ...
    hs.submit(k, n_hops)             # ... H2D, encode + pack + body, D2H are queued; returns at once
    body = hs.result(k)              # uint8 view of the pinned body of that chunk (waits for its D2H only)

or, for a stream already in memory, `for body in hs.encode(pcm): ...` / `pacfile.encode_stream(...,
chunk_hops=N)`, whose bytes equal the one-batch path's (tests/test_gpu_round3.py).  HostStreamDecoder (below) is
the same arrangement for the way back: .pac bytes in, PCM out, `pacfile.decode_stream(..., chunk_bytes=N)`.
HostStreamRateEncoder is the average-bit-rate encode on the same chunk front end (_chunk_front), in two passes:
`pacfile.encode_stream_abr_chunked(..., chunk_hops=N)`.

Chunks are consecutive pieces of ONE stream: the one-hop halo (frame f spans hops f-1, f) and, with
block switching, the transient decisions of the two hops before a chunk are carried from chunk to chunk
on the device.  finish() writes what the reference's driver writes after the last hop: that hop a second
time and the zero block of Close (coder/pacfile.py:743-757, 612-625).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .engine import PcmView, _ptr

HOP = 1024


def _chunk_front(enc, n_ch, dev_in, n_hops, halo, carry, tr, block_switching, tail):
    """The front end of one chunk of a stream, queued on the current stream: dev_in [nCh, (F + 1) * 1024] holds the
    chunk's n_hops hops from column 1024 on.  The hop before them comes from `halo` (frame f spans hops f - 1, f), which
    then takes the chunk's last hop; with block switching the detector runs on the chunk's hops and `carry`, the
    decisions of the two hops before the chunk, turns them into the packed flags (last, cur, next) of its frames and
    takes the chunk's last two.  tail: the driver's last two blocks (the last hop again, Close): no detection, Close
    writes (0, 0, 0).  -> (PcmView of the chunk's frames, flags or None)"""
    dev_in[:, :HOP].copy_(halo)                                      # frame 0 of the chunk starts in the previous chunk
    halo.copy_(dev_in[:, n_hops * HOP:(n_hops + 1) * HOP])
    view = PcmView(dev_in, n_ch, n_hops, HOP, dev_in.shape[1], 1)
    flags = None
    if block_switching:
        tr = tr[:n_hops]
        if tail:
            tr.zero_()                                               # the pass after EOF and Close: no detection
        else:
            hops = _lib.PacxPcm(dev_in.data_ptr() + 2 * HOP, _lib.PCM_I16, n_ch, n_hops, HOP, dev_in.shape[1], 1)
            enc._call("pacx_transient_flags", ctypes.byref(hops), _ptr(tr), None, enc._stream())
        ext = torch.cat((carry, tr))                                 # decisions of hops g-2, g-1, g, ...
        flags = ext[:n_hops] | (ext[1:n_hops + 1] << 1) | (ext[2:n_hops + 2] << 2)
        if tail:
            flags[-1] = 0                                            # Close writes (0, 0, 0)
        carry.copy_(ext[n_hops:n_hops + 2])
        flags = flags.contiguous()
    return view, flags


class HostStreamEncoder:
    def __init__(self, enc, n_channels, hops_per_chunk, depth=2, block_switching=False):
        self.enc, self.n_ch, self.F, self.depth = enc, int(n_channels), int(hops_per_chunk), int(depth)
        self.block_switching = bool(block_switching)
        dev = enc.device
        F, n_ch = self.F, self.n_ch
        self.n_cf = F * n_ch
        enc.reserve(self.n_cf)
        # body capacity: the bit budget bounds a channel-block (dist.slot_bytes has the argument)
        from .dist import slot_bytes
        self.cap = slot_bytes(self.n_cf, enc.target_bits_per_sample)
        self.s_in, self.s_k, self.s_out = (torch.cuda.Stream(device=dev) for _ in range(3))
        self.host_in = [torch.zeros((n_ch, F * HOP), dtype=torch.int16).pin_memory() for _ in range(depth)]
        self.dev_in = [torch.zeros((n_ch, (F + 1) * HOP), dtype=torch.int16, device=dev) for _ in range(depth)]
        self.outs = [self._alloc_out() for _ in range(depth)]
        self.bodies = [torch.empty(self.cap, dtype=torch.uint8, device=dev) for _ in range(depth)]
        self.totals = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(depth)]
        self.host_body = [torch.empty(self.cap, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.host_total = [torch.zeros(1, dtype=torch.int64).pin_memory() for _ in range(depth)]
        self.ev_in = [torch.cuda.Event() for _ in range(depth)]
        self.ev_k = [torch.cuda.Event() for _ in range(depth)]
        self.ev_out = [torch.cuda.Event() for _ in range(depth)]
        self.halo = torch.zeros((n_ch, HOP), dtype=torch.int16, device=dev)        # the hop before the next chunk
        self.carry = torch.zeros(2, dtype=torch.uint8, device=dev)                 # transient decisions of the two hops before it
        self.tr = torch.zeros(F, dtype=torch.uint8, device=dev)
        self.fetch = self.cap                       # bytes the next submit fetches: the whole slot until a length is known
        self.fetched = [0] * depth                  # bytes the D2H of each slot's submit actually copied
        self.pending = [False] * depth
        self.n_hops_of = [0] * depth
        self.next_slot = 0
        self.raises = torch.zeros(1, dtype=torch.int32, device=dev)              # PACX_ST_REF_RAISES seen in any chunk

    def _alloc_out(self):
        if self.enc.use_vq:
            e = self.enc
            return {"overall": e._empty((self.n_cf, _lib.SUB), torch.int32),
                    "bit_alloc": torch.zeros((self.n_cf, e.band_stride), dtype=torch.int32, device=e.device),
                    "status": e._empty((self.n_cf,), torch.int32),
                    "payload": e._empty((self.n_cf, e.payload_stride), torch.uint8),
                    "n_bytes": e._empty((self.n_cf,), torch.int32)}
        out = self.enc.alloc_outputs(self.n_cf, with_payload=True)
        out["mantissa"] = None                      # 4 KB per channel-frame nobody reads (short frames pack from the handle's own)
        return out

    # ------------------------------------------------------------------ the three queues
    def input(self, k):
        """pinned staging buffer of slot k: int16 [nCh, hops_per_chunk*1024] as a NumPy view, planar"""
        if self.pending[k]:
            raise RuntimeError(f"slot {k} is still in flight: take result({k}) first")
        return self.host_in[k].numpy()

    def submit(self, k, n_hops=None, _tail=False):
        """queue chunk k (its first n_hops hops): H2D on the copy-in stream, encode + pack + body on the kernel
        stream, D2H on the copy-out stream.  Returns without waiting for any of it."""
        enc, F = self.enc, self.F
        n_hops = F if n_hops is None else int(n_hops)
        if not 0 < n_hops <= F:
            raise ValueError("n_hops must be in 1..hops_per_chunk")
        if self.pending[k]:
            raise RuntimeError(f"slot {k} is still in flight")
        n_cf = n_hops * self.n_ch
        dev_in, out = self.dev_in[k], self.outs[k]
        with torch.cuda.stream(self.s_in):
            self.s_in.wait_event(self.ev_k[k])                       # the kernels that last read dev_in[k] are done
            dev_in[:, HOP:(n_hops + 1) * HOP].copy_(self.host_in[k][:, :n_hops * HOP], non_blocking=True)
            self.ev_in[k].record(self.s_in)
        with torch.cuda.stream(self.s_k):
            self.s_k.wait_event(self.ev_in[k])
            self.s_k.wait_event(self.ev_out[k])                      # the body that last sat in bodies[k] has left
            view, flags = _chunk_front(enc, self.n_ch, dev_in, n_hops, self.halo, self.carry, self.tr,
                                       self.block_switching, _tail)
            sub = {name: (t[:n_cf] if t is not None else None) for name, t in out.items()}
            if enc.use_vq:
                enc.encode_vq(view, flags, sub)
            else:
                enc.encode_pack(view, flags, sub)
                if enc.use_sbr:                                      # scalar mantissas in an SBR file: where the reference raises
                    self.raises |= (sub["status"] & _lib.ST_REF_RAISES).max()
            enc._call("pacx_gather_body", ctypes.c_int64(n_cf), _ptr(sub["payload"]), _ptr(sub["n_bytes"]),
                      _ptr(self.bodies[k]), ctypes.c_int64(self.cap), _ptr(self.totals[k]), enc._stream())
            self.ev_k[k].record(self.s_k)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(self.ev_k[k])
            n = min(self.fetch, self.cap)
            self.host_body[k][:n].copy_(self.bodies[k][:n], non_blocking=True)
            self.fetched[k] = n
            self.host_total[k].copy_(self.totals[k], non_blocking=True)
            self.ev_out[k].record(self.s_out)
        self.pending[k] = True
        self.n_hops_of[k] = n_hops

    def result(self, k):
        """the packed body of chunk k ('<L nBytes' + payload per channel-block, in stream order): a uint8 NumPy
        view of pinned memory, valid until slot k is submitted again.  Waits for that chunk's D2H copy only."""
        if not self.pending[k]:
            raise RuntimeError(f"nothing was submitted in slot {k}")
        self.ev_out[k].synchronize()
        n = int(self.host_total[k].item())
        if n > self.cap:
            raise RuntimeError(f"body of {n} bytes does not fit its {self.cap}-byte buffer")
        got = self.fetched[k]
        if n > got:                                # the fetch was sized from an earlier chunk: get the rest
            with torch.cuda.stream(self.s_out):
                self.host_body[k][got:n].copy_(self.bodies[k][got:n], non_blocking=True)
            self.s_out.synchronize()
        # later submits fetch what this chunk needed plus a margin instead of the whole slot; a slot already in
        # flight keeps the count it was submitted with (fetched[k]), which is what its own result() tops up from
        per_hop = -(-n // max(self.n_hops_of[k], 1))
        self.fetch = min(self.cap, per_hop * self.F + (1 << 16))
        self.pending[k] = False
        return self.host_body[k][:n].numpy()

    # ------------------------------------------------------------------ a whole stream
    def encode(self, pcm, finish=True):
        """pcm: int16 [n_hops*1024, nCh] in host memory (any NumPy array).  Yields the chunks' bodies in order;
        with finish, the last two blocks of the file (the last hop again, Close) close the stream."""
        pcm = np.asarray(pcm)
        n_hops = len(pcm) // HOP
        order = []
        for h0 in range(0, n_hops, self.F):
            k = self.next_slot
            self.next_slot = (k + 1) % self.depth
            if self.pending[k]:
                yield self.result(order.pop(0))
            n = min(self.F, n_hops - h0)
            self.input(k)[:, :n * HOP] = pcm[h0 * HOP:(h0 + n) * HOP].T
            self.submit(k, n)
            order.append(k)
        if finish and n_hops:
            k = self.next_slot
            self.next_slot = (k + 1) % self.depth
            if self.pending[k]:
                yield self.result(order.pop(0))
            tail = self.input(k)
            tail[:, :HOP] = pcm[(n_hops - 1) * HOP:n_hops * HOP].T
            tail[:, HOP:2 * HOP] = 0
            self.submit(k, 2, _tail=True)
            order.append(k)
        for k in order:
            yield self.result(k)

    def reference_raises(self):
        """True if a block of the stream so far is one the reference cannot write (PACX_ST_REF_RAISES: scalar
        mantissas in an SBR file, an omitted band got bits -- coder/quantize.py:73-74 raises TypeError there)"""
        return bool(int(self.raises.item()))

    def reset(self):
        """start a new stream (halo and transient carry back to the start of a file)"""
        torch.cuda.synchronize(self.enc.device)
        self.halo.zero_()
        self.carry.zero_()
        self.raises.zero_()
        self.pending = [False] * self.depth


class SegmentOverLimit(ValueError):
    """HostStreamRateEncoder.encode(..., segment_limits=...): a segment's records took more than its limit.  Raised when
    the chunk in which the first such segment ends is taken; .segment, .total_bytes, .limit_bytes"""

    def __init__(self, segment, total_bytes, limit_bytes):
        super().__init__(f"segment {segment} takes {total_bytes} bytes, its limit is {limit_bytes}")
        self.segment, self.total_bytes, self.limit_bytes = int(segment), int(total_bytes), int(limit_bytes)


class HostStreamRateEncoder:
    """The average-bit-rate encode with band-by-band allocation (pacfile.encode_stream_abr(allocation="band")) in
    chunks of bounded size, host memory to host memory, in two passes over the PCM:

        hr = HostStreamRateEncoder(enc, n_channels=2, hops_per_chunk=4096, max_bits_per_sample=cap, block_switching=True)
        hr.analyse(pcm)                       # per chunk: band curve -> its size at every target, added to the profile
        sol = hr.solve(limit_bytes)           # band_solve's decision on the profile: target_nmr_db, met, total_bytes
        for body in hr.encode(pcm, sol["target_nmr_db"]): ...     # per chunk: curve -> pick -> second pass -> body

    The profile (Encoder.band_profile: G int64 words) is all that the first pass keeps, so device memory is bounded by
    the chunk and the bodies are those of the one-batch call: the curve of a frame, the pick at the target and the
    second pass do not depend on how the stream is cut.  The curve is taken twice -- once per pass -- unless keep_curves()
    was called: then analyse() also writes every chunk's curve out as 16-bit thresholds (Encoder.band_thresholds /
    rate_thresholds), copies them down behind the kernels into host memory or the caller's buffer, and encode() sends them
    up behind the PCM and picks from them without taking the curve again (pacfile.encode_stream_abr_kept).
    Chunks run on HostStreamEncoder's front end (_chunk_front): the PCM of chunk i + 1 goes up while chunk i computes,
    halo and transient carry stay on the device, the driver's last two blocks are a chunk of their own.  pcm is
    anything that slices to int16 [n, nCh] pieces (an np.memmap included); only a chunk of it is touched at a time.
    enc: a scalar encoder, or a gain-shape one without SBR (its curve and second pass, the pick and the solve on its
    scalar sibling), with the cap rate as its rate.

    With segments (pacfile.segment_limits: the n + 2 blocks the driver writes, cut every S blocks, the tail chunk
    included) the first pass keeps a profile ROW per segment the current chunk touches instead
    (Encoder.band_profile_segments), solves the rows of the segments that end in the chunk
    (Encoder.profile_solve_segments) and forgets them:

        hr.analyse(pcm, segment_hops=S, segment_limits=limits)             # one limit per segment
        seg = hr.solve_segments()                                          # target_nmr_db, met, total_bytes, worst_above [n_seg]
        for body in hr.encode(pcm, seg["target_nmr_db"], segment_hops=S): ...

        hr.analyse(pcm, segment_hops=S, segment_limits=peaks, peak=True)   # the limits are peaks: the solved rows are also
        sol = hr.solve_peak(limit_bytes)                                   # clamp-added into the stream's profile
        for body in hr.encode(pcm, sol["target_nmr_db"], segment_hops=S, segment_limits=peaks): ...

    The row buffer holds ceil(max(hops_per_chunk, 2) * nCh / (S * nCh)) + 1 rows of G int64 words -- bounded by the
    chunk; the row of a segment still open at a chunk's end is carried to the next chunk.  Per segment the object
    keeps the solve's result and worst_above on the device, 24 bytes: the only thing that grows with the stream, read
    back once.  The limits and targets of the segments a chunk touches go up with the chunk's PCM.

    allocation="budget" (scalar encoders): pacfile.encode_stream_abr(allocation="budget") instead -- BitAlloc with one
    budget per block.  The same two passes on the other curve (pacfile._BudgetPath): Encoder.rate_curve,
    rate_profile[_segments], rate_pick[_segments] and encode_pack_budget in place of band_curve, band_profile[_segments],
    band_pick[_segments] and encode_pack_alloc; the rows, their solves, the clamped sum, the staging and the check of the
    segments' sums are shared."""

    def __init__(self, enc, n_channels, hops_per_chunk, max_bits_per_sample, block_switching=False, nmr_lo_db=-30,
                 nmr_hi_db=30, depth=2, allocation="band"):
        from .pacfile import _PATHS, _check_allocation
        self.enc, self.n_ch, self.F, self.depth = enc, int(n_channels), int(hops_per_chunk), int(depth)
        if self.F < 1 or self.depth < 2:
            raise ValueError("hops_per_chunk must be at least 1 and depth at least 2")
        self.block_switching, self.max_bps = bool(block_switching), float(max_bits_per_sample)
        self.lo, self.hi = nmr_lo_db, nmr_hi_db
        if not _check_allocation(allocation) and enc.use_vq:
            raise NotImplementedError("gain-shape streams: allocation 'band' only")
        self.path = _PATHS[allocation](enc)
        dev, F, n_ch = enc.device, self.F, self.n_ch
        self.n_cf = max(F, 2) * n_ch                                   # the tail chunk holds two blocks
        enc.reserve(self.n_cf)
        self.cap = self.n_cf * (enc.payload_stride + 4)
        rng = range(self.depth)
        self.s_in, self.s_k, self.s_out = (torch.cuda.Stream(device=dev) for _ in range(3))
        self.host_in = [torch.zeros((n_ch, max(F, 2) * HOP), dtype=torch.int16).pin_memory() for _ in rng]
        self.dev_in = [torch.zeros((n_ch, (max(F, 2) + 1) * HOP), dtype=torch.int16, device=dev) for _ in rng]
        self.bodies = [torch.empty(self.cap, dtype=torch.uint8, device=dev) for _ in rng]
        self.totals = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in rng]
        self.host_body = [torch.empty(self.cap, dtype=torch.uint8).pin_memory() for _ in rng]
        self.host_total = [torch.zeros(1, dtype=torch.int64).pin_memory() for _ in rng]
        self.ev_in = [torch.cuda.Event() for _ in rng]
        self.ev_k = [torch.cuda.Event() for _ in rng]
        self.ev_out = [torch.cuda.Event() for _ in rng]
        self.halo = torch.zeros((n_ch, HOP), dtype=torch.int16, device=dev)
        self.carry = torch.zeros(2, dtype=torch.uint8, device=dev)
        self.tr = torch.zeros(max(F, 2), dtype=torch.uint8, device=dev)
        self.profile = self.path.profile(self.path.no_frames(self.max_bps), self.lo, self.hi)  # zeros [G]; checks the range
        self.n_frames = 0                                              # blocks the last analyse() saw
        self.seg = None                                                # the segments of the last analyse(), if any
        self.rows = None
        self.stage = {}                                                # per-segment words that go up with a chunk
        self.seg_check = [None] * self.depth                           # encode(): (first segment, count) of a slot's sums
        self.keep = None                                               # keep_curves(): (the caller's store or None,)
        self.kept = None                                               # the last analyse()'s kept curves, if it kept them

    # ------------------------------------------------------------------ the curves kept between the passes
    def keep_curves(self, store=None):
        """From the next analyse() on, keep every chunk's curve as 16-bit thresholds (Encoder.band_thresholds /
        rate_thresholds: what a pick at a grid target of the object's range reads of it) in host memory, so that
        encode() picks from them and takes no curve a second time.  store=None: host memory the object allocates when
        the stream is analysed; else a writable C-contiguous uint8 buffer (an np.memmap included) of at least
        kept_bytes(n_hops) bytes, checked by analyse() -- ValueError before any GPU work.  -> self."""
        self.keep, self.kept = (store,), None
        return self

    def kept_bytes(self, n_hops):
        """bytes of the store for a stream of n_hops hops: the n_hops + 2 blocks the driver writes, every channel"""
        return (int(n_hops) + 2) * self.n_ch * self.path.kept_bytes_per_cf(self.max_bps)

    @staticmethod
    def check_store(store, need, what="store"):
        """a caller's store as a flat uint8 NumPy view of it, or ValueError"""
        msg = f"{what}: a writable C-contiguous uint8 buffer of at least {need} bytes"
        try:
            mv = memoryview(store)
        except TypeError:
            raise ValueError(msg) from None
        if mv.format != "B" or mv.itemsize != 1:
            raise ValueError(f"{msg} (its items are not uint8)")
        if mv.readonly:
            raise ValueError(f"{msg} (it is read-only)")
        if not mv.c_contiguous:
            raise ValueError(f"{msg} (it is not C-contiguous)")
        if mv.nbytes < need:
            raise ValueError(f"{msg} (it holds {mv.nbytes})")
        return np.frombuffer(mv, dtype=np.uint8)

    def _kept_buffers(self):
        """per slot: the chunk's kept bytes on the device and their pinned staging buffer, for both ways"""
        if not hasattr(self, "dev_kept"):
            n = self.n_cf * self.path.kept_bytes_per_cf(self.max_bps)
            self.dev_kept = [torch.zeros(n, dtype=torch.uint8, device=self.enc.device) for _ in range(self.depth)]
            self.host_kept = [torch.zeros(n, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
            self.ev_keep = [torch.cuda.Event() for _ in range(self.depth)]

    def _kept_views(self, k, n):
        kept = self.path.kept_views(self.dev_kept[k], n * self.n_ch, self.max_bps)
        kept.update(nmr_lo_db=self.lo, nmr_hi_db=self.hi)
        return kept

    def _chunks(self, pcm):
        """the chunks of a stream and the driver's last two blocks, one after the other: fills the pinned buffer of
        the next slot, queues its way up and yields (slot, hops, tail).  The caller then queues the chunk's work on
        the kernel stream, _front() first and ev_k[slot] last."""
        if len(pcm) % HOP or len(pcm) == 0:
            raise ValueError("pcm: int16 [n, nCh], n a multiple of 1024 and at least 1024")
        torch.cuda.synchronize(self.enc.device)                        # a new pass over the stream
        with torch.cuda.stream(self.s_k):
            self.halo.zero_()
            self.carry.zero_()
        n_hops = len(pcm) // HOP
        pieces = [(h0, min(self.F, n_hops - h0), False) for h0 in range(0, n_hops, self.F)] + [(n_hops - 1, 2, True)]
        for i, (h0, n, tail) in enumerate(pieces):
            k = i % self.depth
            self.ev_in[k].synchronize()                                # the copy that last read host_in[k] is done
            buf = self.host_in[k].numpy()
            piece = np.asarray(pcm[h0 * HOP:(h0 + (1 if tail else n)) * HOP])
            if piece.dtype != np.int16 or piece.ndim != 2 or piece.shape[1] != self.n_ch:
                raise ValueError(f"pcm: int16 [n, {self.n_ch}]")
            buf[:, :len(piece)] = piece.T
            if tail:
                buf[:, HOP:2 * HOP] = 0                                # Close
            with torch.cuda.stream(self.s_in):
                self.s_in.wait_event(self.ev_k[k])                     # the kernels that last read dev_in[k] are done
                self.dev_in[k][:, HOP:(n + 1) * HOP].copy_(self.host_in[k][:, :n * HOP], non_blocking=True)
                self.ev_in[k].record(self.s_in)
            yield k, n, tail

    def _front(self, k, n, tail):
        """on the kernel stream: wait for the chunk's PCM, then the front end -> (view, flags)"""
        self.s_k.wait_event(self.ev_in[k])
        return _chunk_front(self.enc, self.n_ch, self.dev_in[k], n, self.halo, self.carry, self.tr,
                            self.block_switching, tail)

    # ------------------------------------------------------------------ segments: uniform stretches of S blocks
    def _segments(self, pcm, segment_hops, per_segment, what):
        """(S * nCh, number of segments, per_segment as an array of that length) for the n + 2 blocks of pcm"""
        hops = int(segment_hops)
        if isinstance(segment_hops, bool) or hops != segment_hops or hops < 1:
            raise ValueError(f"segment_hops = {segment_hops!r}: a whole number of blocks, at least 1")
        n_seg = -(-(len(pcm) // HOP + 2) // hops)
        per_segment = np.asarray(per_segment)
        if per_segment.shape != (n_seg,):
            raise ValueError(f"{what}: one per segment, [{n_seg}] for this stream")
        return hops * self.n_ch, n_seg, per_segment

    def _piece(self, blocks_before, n, tail, seg_cf):
        """where a chunk of n blocks lies among the segments -> (first_off, index of its first segment, segments it
        touches, how many of them end in it: the stream's last segment ends with the tail chunk)"""
        cf0, n_cf = blocks_before * self.n_ch, n * self.n_ch
        first_off, s0 = cf0 % seg_cf, cf0 // seg_cf
        touched, closed = -(-(first_off + n_cf) // seg_cf), (first_off + n_cf) // seg_cf
        return first_off, s0, touched, touched if tail else closed

    def _stage_up(self, name, k, values, dtype):
        """per-segment words of a chunk on their way up behind the chunk's PCM (copy-in stream, the slot's pinned
        buffer; ev_in[k] then stands for both) -> the device tensor, valid for the kernels of this chunk"""
        R = self.rows_max
        if (name, R) not in self.stage:                                # kept for good: see _rows_max
            self.stage[name, R] = ([torch.zeros(R, dtype=dtype).pin_memory() for _ in range(self.depth)],
                                   [torch.zeros(R, dtype=dtype, device=self.enc.device) for _ in range(self.depth)])
        host, dev = self.stage[name, R]
        m = len(values)
        host[k].numpy()[:m] = values
        with torch.cuda.stream(self.s_in):
            dev[k][:m].copy_(host[k][:m], non_blocking=True)
            self.ev_in[k].record(self.s_in)
        return dev[k][:m]

    def _rows_max(self, seg_cf):
        """the segments a chunk can touch.  What is staged per segment (self.stage) is keyed by this number and never
        dropped: work queued on it may outlive an encode() that is given up half-way"""
        self.rows_max = -(-max(self.F, 2) * self.n_ch // seg_cf) + 1

    def _row_buffer(self, seg_cf):
        """the first pass's rows"""
        self._rows_max(seg_cf)
        G = self.profile.numel()
        if self.rows is None or tuple(self.rows.shape) != (self.rows_max, G):
            torch.cuda.synchronize(self.enc.device)                    # nothing queued still works on the old rows
            self.rows = torch.zeros((self.rows_max, G), dtype=torch.int64, device=self.enc.device)

    def analyse(self, pcm, segment_hops=None, segment_limits=None, peak=False):
        """the first pass: the stream's size at every target of the range, into self.profile (zeroed first).
        -> the profile, int64 device tensor [G]; the host does not wait for it.
        segment_hops=S, segment_limits=[n_seg]: a profile row per segment instead; per chunk the rows of the segments
        the chunk touches are added to, those of the segments that end in it are solved against their limits (result and
        worst_above stay on the device, for solve_segments()) and cleared, the row of a segment still open is carried.
        peak: the limits are peaks, and the solved rows are clamp-added into self.profile, which is then the stream's
        size at every stream target with every segment held at its floor (solve_peak()).  The row buffer has
        ceil(max(hops_per_chunk, 2) nCh / (S nCh)) + 1 rows.  No host wait per chunk either way.
        After keep_curves(): one more step per chunk behind the profile step, the chunk's thresholds on the kernel
        stream and their copy down on the copy-out stream into the slot's pinned staging buffer; the host moves a
        slot's buffer into the store when the slot comes round again and after the last chunk, its only new wait."""
        solver = self.path.solver
        segmented = segment_hops is not None
        self.kept = None
        keep, store = self.keep is not None, None
        if keep:                                                       # refused before any GPU work
            need = self.kept_bytes(len(pcm) // HOP)
            store = np.empty(need, np.uint8) if self.keep[0] is None else self.check_store(self.keep[0], need)
        if segmented:
            seg_cf, n_seg, limits = self._segments(pcm, segment_hops, segment_limits, "segment_limits")
            try:
                limits = limits.astype(np.int64, casting="same_kind")
            except TypeError:
                raise ValueError("segment_limits: whole numbers of bytes") from None
            if (limits < 0).any():
                raise ValueError(f"segment_limits: negative limit for segment {int(np.argmax(limits < 0))}")
            self._row_buffer(seg_cf)
            dev = self.enc.device
            self.seg = {"seg_cf": seg_cf, "n_seg": n_seg, "peak": bool(peak), "limits": limits,
                        "result": torch.zeros((n_seg, 4), dtype=torch.int32, device=dev),
                        "worst": torch.zeros((n_seg,), dtype=torch.int64, device=dev)}
        elif segment_limits is not None or peak:
            raise ValueError("segment_limits and peak go with segment_hops")
        else:
            self.seg = None
        with torch.cuda.stream(self.s_k):
            self.profile.zero_()
            if segmented:
                self.rows.zero_()
        if keep:
            self._kept_buffers()
            per_block = self.n_ch * self.path.kept_bytes_per_cf(self.max_bps)
            waiting = [None] * self.depth                              # (offset in the store, bytes) of a slot's staging buffer

            def land(k):
                """a slot's kept bytes from its staging buffer into the store: the one host wait keeping adds"""
                if waiting[k] is not None:
                    (at, nb), waiting[k] = waiting[k], None
                    self.ev_keep[k].synchronize()
                    store[at:at + nb] = self.host_kept[k].numpy()[:nb]
        frames = 0
        for k, n, tail in self._chunks(pcm):
            if keep:
                land(k)                                                # the slot comes round again
            if segmented:
                first_off, s0, touched, closed = self._piece(frames, n, tail, seg_cf)
                limit_dev = self._stage_up("limit", k, limits[s0:s0 + closed], torch.int64)
            with torch.cuda.stream(self.s_k):
                view, flags = self._front(k, n, tail)
                curve = self.path.curve(view, flags, self.max_bps)
                if not segmented:
                    self.path.profile(curve, self.lo, self.hi, out=self.profile)
                else:
                    self.path.profile_segments(curve, seg_cf, first_off, self.lo, self.hi, out=self.rows)
                    if closed:
                        done, res = self.rows[:closed], self.seg["result"][s0:s0 + closed]
                        solver.profile_solve_segments(done, limit_dev, self.lo, self.hi,
                                                      out=(res, self.seg["worst"][s0:s0 + closed]))
                        if peak:
                            solver.profile_clamp_add(done, res, self.lo, self.hi, out=self.profile)
                        if touched > closed:                           # the open segment's row moves to the front
                            self.rows[0].copy_(self.rows[closed])
                            self.rows[1:touched].zero_()
                        else:
                            self.rows[:touched].zero_()
                if keep:                                               # after the profile step: the curve as thresholds
                    self.s_k.wait_event(self.ev_keep[k])               # the bytes that last sat in dev_kept[k] have left
                    self.path.thresholds(curve, self.lo, self.hi,
                                         out=self.path.kept_views(self.dev_kept[k], n * self.n_ch, self.max_bps))
                self.ev_k[k].record(self.s_k)
            if keep:
                nb = n * per_block
                with torch.cuda.stream(self.s_out):
                    self.s_out.wait_event(self.ev_k[k])
                    self.host_kept[k][:nb].copy_(self.dev_kept[k][:nb], non_blocking=True)
                    self.ev_keep[k].record(self.s_out)
                waiting[k] = (frames * per_block, nb)
            frames += n
        self.n_frames = frames
        if keep:
            for k in range(self.depth):
                land(k)                                                # after the last chunk
            self.kept = {"store": store, "hops": len(pcm) // HOP, "per_block": per_block}
        return self.profile

    def solve(self, limit_bytes):
        """Encoder.profile_solve on the profile of the last analyse(): dict target_nmr_db, met, total_bytes"""
        with torch.cuda.stream(self.s_k):
            return self.path.solver.profile_solve(self.profile, limit_bytes, self.lo, self.hi)

    def solve_segments(self):
        """what the last analyse(segment_hops=...) found per segment, read back once: dict of NumPy arrays
        target_nmr_db (the lowest target of the range at which the segment fits its limit; the highest where it cannot),
        met, total_bytes at that target, worst_above (the most it takes at that target or any higher one)"""
        if self.seg is None:
            raise RuntimeError("solve_segments: the last analyse() had no segments")
        with torch.cuda.stream(self.s_k):
            out = self.path.solver.decode_results(self.seg["result"])
            out["worst_above"] = self.seg["worst"].cpu().numpy()
        return out

    def solve_peak(self, limit_bytes):
        """the two-level solve after analyse(..., peak=True): Encoder.profile_solve on the clamped stream profile is
        the stream's result, and every segment takes T_s = max(stream target, its floor).  -> dict
        stream_target_nmr_db, stream_met, stream_total_bytes; NumPy arrays per segment target_nmr_db (T_s),
        floor_nmr_db, pinned, floor_met (False: the segment cannot be reached), floor_total_bytes, worst_above (a
        segment whose worst_above is within its peak is within it at T_s, whatever T_s)"""
        if self.seg is None or not self.seg["peak"]:
            raise RuntimeError("solve_peak: the last analyse() was not one with peak=True")
        stream, seg = self.solve(limit_bytes), self.solve_segments()
        floor = seg["target_nmr_db"]
        return {"stream_target_nmr_db": stream["target_nmr_db"], "stream_met": stream["met"],
                "stream_total_bytes": stream["total_bytes"], "floor_nmr_db": floor,
                "target_nmr_db": np.maximum(floor, stream["target_nmr_db"]), "pinned": floor > stream["target_nmr_db"],
                "floor_met": seg["met"], "floor_total_bytes": seg["total_bytes"], "worst_above": seg["worst_above"]}

    # ------------------------------------------------------------------ the buffered solve on the kept curves
    def _kept_pieces(self):
        """(blocks before, blocks) of every chunk the last analyse() wrote into the store, the tail chunk last"""
        hops = self.kept["hops"]
        return [(h0, min(self.F, hops - h0)) for h0 in range(0, hops, self.F)] + [(hops, 2)]

    def _kept_up(self, k, blocks_before, n):
        """a chunk's kept bytes from the store into dev_kept[k], on the copy-in stream behind the kernels that last read
        it; ev_in[k] stands for the copy"""
        per_block = self.kept["per_block"]
        at, kb = blocks_before * per_block, n * per_block
        self.ev_in[k].synchronize()                                    # the copy that last read host_kept[k] is done
        self.host_kept[k].numpy()[:kb] = self.kept["store"][at:at + kb]
        with torch.cuda.stream(self.s_in):
            self.s_in.wait_event(self.ev_k[k])
            self.dev_kept[k][:kb].copy_(self.host_kept[k][:kb], non_blocking=True)
            self.ev_in[k].record(self.s_in)

    def _need_kept(self, what):
        if self.keep is None or self.kept is None:
            raise RuntimeError(f"{what}: after keep_curves() and analyse()")

    def solve_bucket(self, limit_bytes, bucket, levels=4):
        """Encoder.band_solve_bucket's / rate_solve_bucket's decision for the stream of the last analyse(), from the
        curves it kept (keep_curves(); RuntimeError otherwise): one target for the stream under limit_bytes and the
        leaky bucket `bucket` (pacfile.bucket).  The bisection's path is walked `levels` decisions (1 ... 5) a pass
        (include/pacx_bucket_kept.h): per pass every chunk's kept bytes go up on the copy-in stream, the kernel stream
        takes the chunk's bytes at the pass's 2^levels - 1 targets (Encoder.band_bytes_thresholds /
        rate_bytes_thresholds) and carries every target's scan over the chunk (bucket_scan_targets), and behind the last
        chunk the tree step decides (bucket_tree_step).  Encoder.bucket_tree_passes(lo, hi, levels) passes, 4 at the
        defaults; the host waits for no result until the one read-back at the end.  -> dict target_nmr_db, met,
        total_bytes and bucket (Encoder.bucket_scan's dict at that target)."""
        from .engine import Encoder
        what = "solve_bucket"
        self._need_kept(what)
        levels = Encoder._tree_levels(what, levels)                    # refused before any GPU work
        Encoder._whole_bytes(what, limit_bytes)
        Encoder._bucket_struct(what, bucket)
        solver = self.path.solver
        drain, size = int(bucket[0]), int(bucket[1])
        n_t = (1 << levels) - 1
        dev = self.enc.device
        if not hasattr(self, "bytes_t"):
            self.bytes_t = torch.empty(_lib.BUCKET_TREE_TARGETS * self.n_cf, dtype=torch.int32, device=dev)
            self.tree = None
        torch.cuda.synchronize(dev)                                    # a new pass over the stream
        with torch.cuda.stream(self.s_k):
            self.tree = tree = solver.bucket_tree_begin(bucket, self.lo, self.hi, levels, tree=self.tree)
        pieces, i = self._kept_pieces(), 0
        for _ in range(solver.bucket_tree_passes(self.lo, self.hi, levels)):
            for before, n in pieces:
                k, i = i % self.depth, i + 1
                self._kept_up(k, before, n)
                n_cf = n * self.n_ch
                with torch.cuda.stream(self.s_k):
                    self.s_k.wait_event(self.ev_in[k])
                    rows = self.path.bytes_kept(self._kept_views(k, n), tree["target_t"][:n_t],
                                                out=self.bytes_t[:n_t * n_cf].view(n_t, n_cf))
                    solver.bucket_scan_targets(rows, self.n_ch, drain, size, before, tree["acc"][:n_t])
                    self.ev_k[k].record(self.s_k)
            with torch.cuda.stream(self.s_k):
                solver.bucket_tree_step(limit_bytes, bucket, levels, tree)
        with torch.cuda.stream(self.s_k):
            return solver.bucket_tree_result(tree)

    def level_at(self, target_nmr_db, bucket, hop):
        """the bucket's level right after block `hop` arrives with the stream of the last analyse() picked at
        target_nmr_db, in 1 / 65536 byte: the kept chunks up to that block, one after the other, through the pick at
        one target and Encoder.bucket_scan(want_level=True), the start level of a chunk carried by the host -- a wait per
        chunk, for the path that ends in an error message.  The blocks before `hop` must not overflow the bucket."""
        self._need_kept("level_at")
        solver, start = self.path.solver, int(bucket[2])
        torch.cuda.synchronize(self.enc.device)
        for i, (before, n) in enumerate(self._kept_pieces()):
            k = i % self.depth
            self._kept_up(k, before, n)
            with torch.cuda.stream(self.s_k):
                self.s_k.wait_event(self.ev_in[k])
                pick = self.path.pick(self._kept_views(k, n), float(target_nmr_db))
                scan = solver.bucket_scan(pick["n_bytes"], self.n_ch, (int(bucket[0]), int(bucket[1]), start),
                                          want_level=True)
                self.ev_k[k].record(self.s_k)
                if before <= hop < before + n:
                    return int(scan["level"][hop - before].item())
            start = scan["end_q16"]
        raise ValueError(f"level_at: block {hop} is not one of the stream's {self.kept['hops'] + 2}")

    def _result(self, k):
        """the body of the chunk in slot k: a uint8 NumPy view of pinned memory, valid until the slot is used again"""
        self.ev_out[k].synchronize()
        n = int(self.host_total[k].item())
        if n > self.cap:
            raise RuntimeError(f"body of {n} bytes does not fit its {self.cap}-byte buffer")
        if self.seg_check[k] is not None:                              # the segments that ended in this chunk
            (s0, m, limits), self.seg_check[k] = self.seg_check[k], None
            took = self.host_sum[k][:m].numpy()
            over = took > limits[s0:s0 + m]
            if over.any():
                i = int(np.argmax(over))
                raise SegmentOverLimit(s0 + i, took[i], limits[s0 + i])
        with torch.cuda.stream(self.s_out):
            self.host_body[k][:n].copy_(self.bodies[k][:n], non_blocking=True)
        self.s_out.synchronize()
        return self.host_body[k][:n].numpy()

    def encode(self, pcm, target_nmr_db, segment_hops=None, segment_limits=None, use_kept=True):
        """the second pass: yields the chunks' bodies in order ('<L nBytes' + payload per channel-block), every band at
        the smallest size that keeps it at or below target_nmr_db (Encoder.band_pick), the driver's last two blocks
        last.  A body is a view of pinned memory, valid until the next one is taken.
        segment_hops=S with target_nmr_db [n_seg] (multiples of 1/64 dB): one target per segment
        (Encoder.band_pick_segments).  segment_limits=[n_seg] besides: every segment's records are summed as they are
        picked (n_bytes + 4 each), and SegmentOverLimit is raised in place of the body of the chunk in which the first
        segment beyond its limit ends -- the bodies before it have been handed out by then.
        After keep_curves() and an analyse() of a stream of this length the curves are not taken again: every chunk's
        kept bytes go up behind its PCM and the pick runs on them (Encoder.band_pick_thresholds[_segments]); the front
        end still runs, the second pass needs its flags.  The targets must then be multiples of 1/64 dB inside the
        object's range (ValueError).  The store belongs to the last analyse(): the length of pcm is checked, that it
        is the same stream cannot be.  use_kept=False: the curves are taken again whatever is kept."""
        enc, order = self.enc, []
        segmented = segment_hops is not None
        kept = self.kept if use_kept and self.kept is not None and self.kept["hops"] == len(pcm) // HOP else None
        if kept is not None:
            g = np.atleast_1d(np.asarray(target_nmr_db, np.float64)) * _lib.RATE_TARGET_GRID
            if not np.isfinite(g).all() or (g != np.round(g)).any() or (g < self.lo * _lib.RATE_TARGET_GRID).any() or \
                    (g > self.hi * _lib.RATE_TARGET_GRID).any():
                raise ValueError(f"target_nmr_db: with kept curves, multiples of 1/{_lib.RATE_TARGET_GRID} dB in "
                                 f"[{self.lo}, {self.hi}]")
        if segmented:
            seg_cf, n_seg, targets = self._segments(pcm, segment_hops, target_nmr_db, "target_nmr_db")
            grid = targets.astype(np.float64) * _lib.RATE_TARGET_GRID
            if not np.isfinite(grid).all() or (grid != np.round(grid)).any() or (np.abs(grid) > 2 ** 26).any():
                raise ValueError(f"target_nmr_db: finite multiples of 1/{_lib.RATE_TARGET_GRID} dB")
            grid = grid.astype(np.int32)
            self._rows_max(seg_cf)
            limits = None
            if segment_limits is not None:
                limits = self._segments(pcm, segment_hops, segment_limits, "segment_limits")[2].astype(np.int64)
                R = self.rows_max
                if ("sums", R) not in self.stage:
                    self.stage["sums", R] = (
                        [torch.zeros(R, dtype=torch.int64).pin_memory() for _ in range(self.depth)],
                        [torch.zeros(R, dtype=torch.int64, device=enc.device) for _ in range(self.depth)],
                        torch.zeros(R, dtype=torch.int64, device=enc.device))
                # sums: per local segment, [0] starts with the carry; sums_done[k]: the chunk's, on their way down
                self.host_sum, sums_done, sums = self.stage["sums", R]
        elif segment_limits is not None:
            raise ValueError("segment_limits goes with segment_hops")
        self.seg_check = [None] * self.depth
        frames = 0
        for k, n, tail in self._chunks(pcm):
            if len(order) == self.depth:                               # slot k still holds a body nobody took
                yield self._result(order.pop(0))
            if segmented:
                first_off, s0, touched, closed = self._piece(frames, n, tail, seg_cf)
                target_dev = self._stage_up("target", k, grid[s0:s0 + touched], torch.int32)
            if kept is not None:                                       # the chunk's kept bytes go up behind its PCM
                at, kb = frames * kept["per_block"], n * kept["per_block"]
                self.host_kept[k].numpy()[:kb] = kept["store"][at:at + kb]
                with torch.cuda.stream(self.s_in):
                    self.dev_kept[k][:kb].copy_(self.host_kept[k][:kb], non_blocking=True)
                    self.ev_in[k].record(self.s_in)
            with torch.cuda.stream(self.s_k):
                view, flags = self._front(k, n, tail)
                curve = self.path.curve(view, flags, self.max_bps) if kept is None else self._kept_views(k, n)
                if segmented:
                    pick = self.path.pick_segments(curve, seg_cf, first_off, target_dev)
                    if limits is not None:
                        if frames == 0:                                # cleared on this stream, behind whatever an encode()
                            sums.zero_()                               # given up half-way still had queued on it
                        # what the segments take; the open one's bytes so far sit in sums[0], from the chunk before
                        nb = pick["n_bytes"].to(torch.int64)
                        ids = (torch.arange(n * self.n_ch, device=enc.device) + first_off) // seg_cf
                        sums.index_add_(0, ids, torch.where(nb > 0, nb + 4, torch.zeros_like(nb)))
                else:
                    pick = self.path.pick(curve, float(target_nmr_db))
                out = self.path.second_pass(view, flags, pick)
                self.s_k.wait_event(self.ev_out[k])                    # the total that last sat in totals[k] has left
                enc._call("pacx_gather_body", ctypes.c_int64(n * self.n_ch), _ptr(out["payload"]), _ptr(out["n_bytes"]),
                          _ptr(self.bodies[k]), ctypes.c_int64(self.cap), _ptr(self.totals[k]), enc._stream())
                if segmented and limits is not None:                   # after the wait above: sums_done[k] has left too
                    sums_done[k].copy_(sums)
                    carry = sums[closed].clone() if touched > closed else None
                    sums.zero_()
                    if carry is not None:
                        sums[0] = carry
                self.ev_k[k].record(self.s_k)
            with torch.cuda.stream(self.s_out):
                self.s_out.wait_event(self.ev_k[k])
                self.host_total[k].copy_(self.totals[k], non_blocking=True)
                if segmented and limits is not None and closed:
                    self.host_sum[k][:closed].copy_(sums_done[k][:closed], non_blocking=True)
                    self.seg_check[k] = (s0, closed, limits)
                self.ev_out[k].record(self.s_out)
            order.append(k)
            frames += n
        for k in order:
            yield self._result(k)


class HostStreamDecoder:
    """The decode side of the same pipeline: a .pac body in host memory (or coming out of a file) to int16
    PCM in host memory, in chunks of at most `chunk_bytes` bytes and `max_blocks` hops, so the memory in use is
    bounded by the chunk and not by the stream.

        hs = HostStreamDecoder(enc, n_channels=2, chunk_bytes=16 << 20, max_blocks=32768)
        for pcm in hs.decode(read):      # read(n) -> up to n more bytes of the body, b"" at its end
            ...                          # int16 [hops*1024, nCh]: a view of pinned memory, valid until the next one

    Per chunk: the bytes go up on the copy-in stream and pacx_index_body finds the records there (no walk of the
    length prefixes on the host); the host takes the 24-byte result, which tells it how many records to decode and
    how many bytes they took, queues unpack + decode + pacx_overlap_add_pcm on the kernel stream and the PCM's way
    back on the copy-out stream, moves the bytes the chunk did not consume to the front of the next pinned buffer,
    tops that up from the source and submits it -- while the chunk before is still decoding.  The host waits for an
    index result and for PCM it is about to hand out, never for a decode it has just queued.  The half-block
    across a chunk boundary is the decoder's one `tail` (on the device); the last chunk flushes it as the
    reference does at EOF (coder/pacfile.py:245-249).

    A malformed stream raises what pacfile.decode_stream raises, when the chunk that holds the fault is reached:
    the PCM of the chunks before it has been handed out by then, as in the reference's hop-by-hop loop."""

    def __init__(self, enc, n_channels, chunk_bytes, max_blocks, depth=2, timing=False):
        self.enc, self.n_ch = enc, int(n_channels)
        self.chunk_bytes, self.max_blocks, self.depth = int(chunk_bytes), int(max_blocks), int(depth)
        need = self.n_ch * (enc.payload_stride + 4)
        if self.chunk_bytes < need:
            raise ValueError(f"chunk_bytes below {need} (one hop of {self.n_ch} longest records) cannot guarantee progress")
        if self.max_blocks < 1 or self.depth < 2:
            raise ValueError("max_blocks must be at least 1 and depth at least 2")
        dev, C, n_ch = enc.device, self.chunk_bytes, self.n_ch
        self.max_cf = n_cf = self.max_blocks * n_ch
        i32, i64, u8, f64 = torch.int32, torch.int64, torch.uint8, torch.float64
        self.s_in, self.s_k, self.s_out = (torch.cuda.Stream(device=dev) for _ in range(3))
        rng = range(self.depth)
        self.host_in = [torch.empty(C, dtype=u8).pin_memory() for _ in rng]
        self.dev_in = [torch.zeros(C + 8, dtype=u8, device=dev) for _ in rng]        # 8 bytes of slack for the parsers
        self.offsets = [torch.empty(n_cf, dtype=i64, device=dev) for _ in rng]
        self.sizes = [torch.empty(n_cf, dtype=i32, device=dev) for _ in rng]
        self.index = [torch.zeros(3, dtype=i64, device=dev) for _ in rng]
        self.host_index = [torch.zeros(3, dtype=i64).pin_memory() for _ in rng]
        self.pcm = [torch.empty(((self.max_blocks + 1) * HOP, n_ch), dtype=torch.int16, device=dev) for _ in rng]
        self.host_pcm = [torch.empty(((self.max_blocks + 1) * HOP, n_ch), dtype=torch.int16).pin_memory() for _ in rng]
        self.status = [torch.zeros(1, dtype=i32, device=dev) for _ in rng]
        self.host_status = [torch.zeros(1, dtype=i32).pin_memory() for _ in rng]
        self.ev_in = [torch.cuda.Event() for _ in rng]
        self.ev_k = [torch.cuda.Event() for _ in rng]
        self.ev_out = [torch.cuda.Event() for _ in rng]
        # what only the kernel stream touches exists once: the chunks' decodes run one after the other
        self.blocks = torch.empty((n_cf, 2 * HOP), dtype=f64, device=dev)
        self.codes = {"flags": torch.empty(n_cf, dtype=u8, device=dev),
                      "overall": torch.empty((n_cf, _lib.SUB), dtype=i32, device=dev),
                      "bit_alloc": torch.zeros((n_cf, enc.band_stride), dtype=i32, device=dev),
                      "status": torch.zeros(n_cf, dtype=i32, device=dev)}
        if not enc.use_vq:
            self.codes["scale_factor"] = torch.zeros((n_cf, enc.band_stride), dtype=i32, device=dev)
            self.codes["mantissa"] = torch.empty((n_cf, HOP), dtype=i32, device=dev)
            if enc.use_sbr:
                self.codes["status_sbr"] = torch.zeros(n_cf, dtype=i32, device=dev)
        self.status_bits = torch.zeros(n_cf, dtype=i32, device=dev)
        self.tail = torch.zeros((n_ch, HOP), dtype=f64, device=dev)               # the half-block before the next chunk
        self.n_bytes_of, self.final_of, self.hops_of = [0] * self.depth, [False] * self.depth, [0] * self.depth
        self.pending = [False] * self.depth
        self.timing = [] if timing else None       # per chunk: (records, index events, decode events)
        self.in_use = False                        # a decode() of this object is under way (pacfile.iter_decode keeps one)

    # ------------------------------------------------------------------ the three queues
    def input(self, k):
        """pinned staging buffer of slot k: uint8 [chunk_bytes] as a NumPy view"""
        return self.host_in[k].numpy()

    def submit_index(self, k, n_bytes, final):
        """queue the first n_bytes of slot k: H2D, pacx_index_body and its result's way back, all on the copy-in
        stream (beside the decode of the chunk before).  final: the source has nothing more."""
        enc, n = self.enc, int(n_bytes)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if self.timing is not None else None
        with torch.cuda.stream(self.s_in):
            self.s_in.wait_event(self.ev_k[k])                       # the decode that last read dev_in[k] and its index is done
            self.dev_in[k][:n].copy_(self.host_in[k][:n], non_blocking=True)
            self.dev_in[k][n:n + 8].zero_()
            if ev:
                ev[0].record(self.s_in)
            enc._call("pacx_index_body", _ptr(self.dev_in[k]), ctypes.c_int64(n), self.n_ch, int(bool(final)),
                      ctypes.c_int64(self.max_cf), _ptr(self.offsets[k]), _ptr(self.sizes[k]), _ptr(self.index[k]),
                      enc._stream())
            if ev:
                ev[1].record(self.s_in)
            self.host_index[k].copy_(self.index[k], non_blocking=True)
            self.ev_in[k].record(self.s_in)
        self.n_bytes_of[k], self.final_of[k] = n, bool(final)
        self._index_events = ev

    def index_result(self, k):
        """(records found, bytes they took, position of the prefix at which the chain broke or -1) of slot k: waits
        for that chunk's copy-in and index only"""
        self.ev_in[k].synchronize()
        n_rec, consumed, error_at = (int(v) for v in self.host_index[k].tolist())
        if not (0 <= n_rec <= self.max_cf and n_rec % self.n_ch == 0 and 0 <= consumed <= self.n_bytes_of[k]):
            raise RuntimeError(f"pacx_index_body returned {n_rec} records, {consumed} bytes")
        return n_rec, consumed, error_at

    def submit_decode(self, k, n_records, flush):
        """queue unpack + decode + overlap-and-add of the records index_result(k) reported on the kernel stream and
        the PCM's copy to pinned memory on the copy-out stream.  Returns without waiting for any of it."""
        enc, c, n = self.enc, self.codes, int(n_records)
        n_blocks = n // self.n_ch
        hops = n_blocks + int(bool(flush))
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if self.timing is not None else None
        with torch.cuda.stream(self.s_k):
            st = enc._stream()
            self.s_k.wait_event(self.ev_in[k])
            self.s_k.wait_event(self.ev_out[k])                      # the PCM that last sat in pcm[k] has left
            if ev:
                ev[0].record(self.s_k)
            if n:
                body, offs, sizes = _ptr(self.dev_in[k]), _ptr(self.offsets[k]), _ptr(self.sizes[k])
                c["bit_alloc"][:n].zero_()                           # the one-batch path hands the kernels zeroed band arrays
                if enc.use_vq:
                    enc._call("pacx_decode_vq_batch", ctypes.c_int64(n_blocks), self.n_ch, body, 0, offs, sizes,
                              _ptr(c["flags"]), _ptr(c["overall"]), _ptr(c["bit_alloc"]), None, _ptr(self.blocks), None,
                              _ptr(c["status"]), st)
                else:
                    c["scale_factor"][:n].zero_()
                    enc._call("pacx_unpack_batch", ctypes.c_int64(n), body, 0, offs, sizes, _ptr(c["flags"]),
                              _ptr(c["overall"]), _ptr(c["scale_factor"]), _ptr(c["bit_alloc"]), _ptr(c["mantissa"]),
                              _ptr(c["status"]), st)
                    if enc.use_sbr:                                  # PACFile.Decode's routing (pacfile._decode_scalar)
                        enc._call("pacx_decode_sbr_batch", ctypes.c_int64(n_blocks), self.n_ch, _ptr(c["flags"]),
                                  _ptr(c["overall"]), _ptr(c["scale_factor"]), _ptr(c["bit_alloc"]), _ptr(c["mantissa"]),
                                  0, None, _ptr(self.blocks), None, _ptr(c["status_sbr"]), st)
                        torch.bitwise_or(c["status"][:n], c["status_sbr"][:n], out=c["status"][:n])
                    else:
                        enc._call("pacx_decode_batch", ctypes.c_int64(n_blocks), self.n_ch, _ptr(c["flags"]),
                                  _ptr(c["overall"]), _ptr(c["scale_factor"]), _ptr(c["bit_alloc"]), _ptr(c["mantissa"]),
                                  _ptr(self.blocks), None, st)
                torch.bitwise_and(c["status"][:n], _lib.ST_MALFORMED | _lib.ST_VQ_UNDEFINED, out=self.status_bits[:n])
                torch.amax(self.status_bits[:n], dim=0, keepdim=True, out=self.status[k])
            else:
                self.status[k].zero_()
            if ev:
                ev[1].record(self.s_k)
            enc._call("pacx_overlap_add_pcm", ctypes.c_int64(n_blocks), self.n_ch, _ptr(self.blocks), _ptr(self.tail),
                      int(bool(flush)), _ptr(self.pcm[k]), st)
            self.ev_k[k].record(self.s_k)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(self.ev_k[k])
            self.host_pcm[k][:hops * HOP].copy_(self.pcm[k][:hops * HOP], non_blocking=True)
            self.host_status[k].copy_(self.status[k], non_blocking=True)
            self.ev_out[k].record(self.s_out)
        self.hops_of[k] = hops
        self.pending[k] = True
        if self.timing is not None:
            self.timing.append((n, self._index_events, ev))

    def result(self, k):
        """int16 [hops*1024, nCh] of chunk k: a NumPy view of pinned memory, valid until slot k decodes again.  Waits
        for that chunk's D2H copy only.  Raises what pacfile.decode_stream raises for a record the parsers reject."""
        if not self.pending[k]:
            raise RuntimeError(f"nothing was submitted in slot {k}")
        self.ev_out[k].synchronize()
        self.pending[k] = False
        st = int(self.host_status[k].item())
        if st:
            from . import pacfile
            if st & _lib.ST_MALFORMED:
                raise RuntimeError(pacfile._PARTIAL)
            if self.enc.use_vq:
                raise RuntimeError(pacfile._VQ_UNDEFINED)
            raise IndexError(pacfile._SBR_INDEX)
        return self.host_pcm[k][:self.hops_of[k] * HOP].numpy()

    # ------------------------------------------------------------------ a whole stream
    def _fill(self, k, have, read):
        """top slot k's pinned buffer up from the source -> (bytes in it, source exhausted)"""
        buf = self.input(k)
        while have < self.chunk_bytes:
            piece = read(self.chunk_bytes - have)
            if not len(piece):
                return have, True
            buf[have:have + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
            have += len(piece)
        return have, False

    def decode(self, read):
        """read(n) -> up to n further bytes of the body (bytes-like), empty at its end.  Yields the chunks' PCM in
        order; the source is read no more than one buffer ahead of the chunk being decoded."""
        from . import pacfile
        self.reset()
        k, order = 0, []
        have, exhausted = self._fill(k, 0, read)
        self.submit_index(k, have, exhausted)
        while True:
            n_rec, consumed, error_at = self.index_result(k)
            n_buf = self.n_bytes_of[k]
            if error_at >= 0 or (n_rec == 0 and consumed < n_buf):
                # a broken chain, or less than one whole hop where one must be (a full buffer, or the stream's end)
                for j in order:
                    yield self.result(j)
                raise RuntimeError(pacfile._PARTIAL)
            if self.pending[k]:
                yield self.result(order.pop(0))                      # the chunk that last used this slot's PCM buffers
            last = self.final_of[k] and consumed == n_buf
            self.submit_decode(k, n_rec, last)
            order.append(k)
            if last:
                break
            k2 = (k + 1) % self.depth
            rem = n_buf - consumed
            self.input(k2)[:rem] = self.input(k)[consumed:n_buf]     # what this chunk did not take opens the next one
            if not exhausted:
                rem, exhausted = self._fill(k2, rem, read)
            self.submit_index(k2, rem, exhausted)
            k = k2
        for j in order:
            yield self.result(j)

    def timings(self):
        """[(records, index ms, decode-kernel ms)] per chunk since the decoder was made (timing=True): device-event times"""
        torch.cuda.synchronize(self.enc.device)
        return [(n, a[0].elapsed_time(a[1]), b[0].elapsed_time(b[1])) for n, a, b in self.timing]

    def reset(self):
        """start a new stream"""
        torch.cuda.synchronize(self.enc.device)
        self.tail.zero_()
        self.pending = [False] * self.depth
