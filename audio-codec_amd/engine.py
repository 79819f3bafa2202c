"""Batched encode engine: owns one pacx handle (HIP library, include/pacx.h) and
runs the per-frame hot path of codec.Encode for thousands of channel-frames per
launch.  PyTorch is used for device memory and streams only.

Reference path replaced: coder/codec.py:225-380 (Encode/EncodeSingleChannel)
and the window/mdct/psychoac/bitalloc/quantize functions it calls.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, tables
from .curves import BAND, RATE
from .psychoac import ScaleFactorBands, AssignMDCTLinesFromFreqLimits

N_LONG, N_SHORT = 1024, 128          # MDCT lines of long / short blocks


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class PcmView:
    """Strided view of PCM on the device (see pacx_pcm in include/pacx.h)."""

    def __init__(self, tensor, n_channels, n_frames, frame_stride, channel_stride,
                 sample_stride=1):
        if tensor.dtype == torch.int16:
            dt = _lib.PCM_I16
        elif tensor.dtype == torch.float64:
            dt = _lib.PCM_F64
        else:
            raise TypeError("PCM must be int16 codes or float64 signed fractions")
        if not tensor.is_cuda:
            raise ValueError("PCM tensor must live on the GPU")
        self.tensor = tensor                      # keeps the memory alive
        self.n_channels, self.n_frames = int(n_channels), int(n_frames)
        # the C side cannot see the allocation: the last element the view addresses, counted from the tensor's place
        # in its storage, has to lie inside that storage (negative strides are left to the library, which refuses them)
        if self.n_frames > 0 and self.n_channels > 0:
            last = (self.n_frames - 1) * max(int(frame_stride), 0) + (self.n_channels - 1) * max(int(channel_stride), 0) \
                + (2 * N_LONG - 1) * max(int(sample_stride), 0)
            have = tensor.untyped_storage().nbytes() // tensor.element_size() - tensor.storage_offset()
            if last >= have:
                raise ValueError(f"PCM view leaves its storage: its last element is {last} past the tensor's first, "
                                 f"the storage holds {have} from there")
        self.c = _lib.PacxPcm(tensor.data_ptr(), dt, self.n_channels, self.n_frames,
                              int(frame_stride), int(channel_stride), int(sample_stride))

    @property
    def n_cf(self):
        return self.n_channels * self.n_frames

    @staticmethod
    def stream(planar, hop=N_LONG):
        """planar: [n_ch, (n_hops+1)*hop] -- hop 0 is the prior block (zeros at
        the start of a file); frame f spans hops f, f+1 (coder/pacfile.py:460-464)."""
        n_ch, n = planar.shape
        assert planar.is_contiguous() and n % hop == 0 and n >= 2 * hop
        return PcmView(planar, n_ch, n // hop - 1, hop, n, 1)

    @staticmethod
    def frames(blocks):
        """blocks: [n_frames, n_ch, 2*hop] independent full blocks."""
        n_f, n_ch, n = blocks.shape
        assert blocks.is_contiguous()
        return PcmView(blocks, n_ch, n_f, n_ch * n, n, 1)


class Encoder:
    """One handle = one (sampleRate, bit rate, band layout) on one GPU."""

    def __init__(self, sample_rate, target_bits_per_sample, n_scale_bits=4, n_mant_size_bits=12,
                 sf_bands=None, sf_bands_short=None, device=None, n_mdct_lines=N_LONG,
                 use_vq=False, use_sbr=False, guard=False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.PacxError("no GPU visible: the encode path has no CPU implementation")
        if n_mdct_lines != N_LONG:
            raise _lib.PacxError("kernels are built for nMDCTLines = 1024")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.sample_rate = int(sample_rate)
        self.target_bits_per_sample = float(target_bits_per_sample)
        self.n_scale_bits, self.n_mant_size_bits = int(n_scale_bits), int(n_mant_size_bits)
        self.sfBands = sf_bands or ScaleFactorBands(
            AssignMDCTLinesFromFreqLimits(N_LONG, self.sample_rate))
        self.sfBandsShort = sf_bands_short or ScaleFactorBands(
            AssignMDCTLinesFromFreqLimits(N_SHORT, self.sample_rate))
        for bands in (self.sfBands, self.sfBandsShort):
            if np.any(np.asarray(bands.nLines) <= 0):
                # a band without lines (the default 25-band table below 31 kHz: bands above Nyquist are empty): the
                # reference gets as far as CalcSMRs' np.amax over the empty band (coder/psychoac.py:289) and raises
                raise ValueError("zero-size array to reduction operation maximum which has no identity")

        keep = self._host = {}
        def f64(name, arr):
            keep[name] = np.ascontiguousarray(arr, dtype=np.float64)
            return keep[name].ctypes.data_as(_lib.c_double_p)
        def i32(name, arr):
            keep[name] = np.ascontiguousarray(arr, dtype=np.int32)
            return keep[name].ctypes.data_as(_lib.c_int32_p)
        sr = self.sample_rate
        cfg = _lib.PacxConfig()
        cfg.abi_version = _lib.PACX_ABI_VERSION
        cfg.device = self.device.index
        cfg.sample_rate = sr
        cfg.n_lines_long, cfg.n_lines_short = N_LONG, N_SHORT
        cfg.n_scale_bits, cfg.n_mant_size_bits = self.n_scale_bits, self.n_mant_size_bits
        cfg.n_bands_long, cfg.n_bands_short = self.sfBands.nBands, self.sfBandsShort.nBands
        cfg.target_bits_per_sample = self.target_bits_per_sample
        cfg.band_lines_long = i32("bl", self.sfBands.nLines)
        cfg.band_lines_short = i32("bs", self.sfBandsShort.nLines)
        cfg.win_long = f64("wl", tables.long_windows(2 * N_LONG))
        cfg.win_short = f64("ws", tables.sine(2 * N_SHORT))
        cfg.hann_long = f64("hl", tables.hann(2 * N_LONG))
        cfg.hann_short = f64("hs", tables.hann(2 * N_SHORT))
        cfg.bark_long = f64("zl", tables.bark(tables.line_freqs(N_LONG, sr)))
        cfg.thresh_long = f64("tl", tables.thresh(tables.line_freqs(N_LONG, sr)))
        cfg.bark_short = f64("zs", tables.bark(tables.line_freqs(N_SHORT, sr)))
        cfg.thresh_short = f64("ts", tables.thresh(tables.line_freqs(N_SHORT, sr)))
        cfg.fft_norm_long = tables.fft_norm(2 * N_LONG)
        cfg.fft_norm_short = tables.fft_norm(2 * N_SHORT)
        cfg.fft_freq_step_long = tables.fft_freq_step(2 * N_LONG, sr)
        cfg.fft_freq_step_short = tables.fft_freq_step(2 * N_SHORT, sr)
        self.use_vq, self.use_sbr = bool(use_vq), bool(use_sbr)
        cfg.use_vq, cfg.use_sbr = int(self.use_vq), int(self.use_sbr)
        l_max = int(max(np.max(self.sfBands.nLines), np.max(self.sfBandsShort.nLines)))
        cfg.half_log2 = f64("hl2", tables.half_log2(l_max))
        cfg.vq_log2_tan = f64("lt", tables.vq_log2_tan())
        cfg.log_mu1 = tables.log_mu1()
        gw, gr = tables.sbr_gauss()
        cfg.sbr_gauss, cfg.sbr_gauss_radius = f64("gw", gw), gr
        cfg.line_freq_long = f64("lf", (np.arange(N_LONG) + 1 / 2) * (sr / (2 * N_LONG)))
        cfg.kbd_long = f64("kl", tables.kbd(2 * N_LONG))
        cfg.kbd_short = f64("ks", tables.kbd(2 * N_SHORT))
        cfg.guard = int(bool(guard))             # PACX_ST_GUARD in the status words (about 3 % of throughput)
        h = ctypes.c_void_p()
        rc = self.lib.pacx_create(ctypes.byref(cfg), ctypes.byref(h))
        _lib.check(self.lib, None, rc, "pacx_create")
        self.h = h
        self.band_stride = self.lib.pacx_band_stride(h)
        self.payload_stride = self.lib.pacx_payload_stride(h)

    def set_side_fork(self, enable):
        """all-long scalar batches: the side chain on the handle's second stream beside the transform (pays with several
        handles in the process, costs with one: include/pacx.h)"""
        self._call("pacx_set_side_fork", int(bool(enable)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.pacx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ----------------------------------------------------------------- helpers
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(self.h, *args)
        _lib.check(self.lib, self.h, rc, name)

    def reserve(self, n_cf):
        self._call("pacx_reserve", ctypes.c_int64(int(n_cf)))

    def flags_tensor(self, flags, n_frames):
        """flags: None, or per-frame iterable of (last, cur, next) / packed uint8."""
        if flags is None:
            return None
        if isinstance(flags, torch.Tensor):
            t = flags.to(device=self.device, dtype=torch.uint8)
        else:
            a = np.asarray(flags)
            if a.ndim == 2:
                a = (a[:, 0] != 0) * 1 + (a[:, 1] != 0) * 2 + (a[:, 2] != 0) * 4
            t = torch.as_tensor(a.astype(np.uint8), device=self.device)
        assert t.numel() == n_frames
        return t.contiguous()

    # ------------------------------------------------------------------ stages
    def mdct(self, pcm, flags=None, short=False, want_scale=False, prewindowed=False, kbd=False):
        """window + MDCT (+ overall scale factor).  lines: [n_cf, 1024] float64
        (short: [n_cf, 8, 128]).  kbd: KBDWindow instead of the sine window."""
        fl = self.flags_tensor(flags, pcm.n_frames)
        lines = self._empty((pcm.n_cf, N_LONG), torch.float64)
        scale = self._empty((pcm.n_cf, _lib.SUB) if short else (pcm.n_cf,), torch.int32) \
            if want_scale else None
        mode = (_lib.MDCT_SHORT if short else 0) | (_lib.MDCT_PREWINDOWED if prewindowed else 0) | \
            (_lib.MDCT_KBD if kbd else 0)
        self._call("pacx_mdct_batch", ctypes.byref(pcm.c), _ptr(fl), mode, _ptr(lines),
                   _ptr(scale), self._stream())
        if short:
            lines = lines.view(pcm.n_cf, _lib.SUB, N_SHORT)
        return (lines, scale) if want_scale else lines

    def smr(self, pcm, lines, short=False, want_threshold=False, want_peaks=False):
        """CalcSMRs.  lines are the unscaled MDCT lines.  smr: [n_cf, band_stride]."""
        lines = lines.contiguous().view(pcm.n_cf, N_LONG)
        smr = torch.zeros((pcm.n_cf, self.band_stride), dtype=torch.float64, device=self.device)
        thr = self._empty((pcm.n_cf, N_LONG), torch.float64) if want_threshold else None
        npk = self._empty((pcm.n_cf, _lib.SUB) if short else (pcm.n_cf,), torch.int32) \
            if want_peaks else None
        self._call("pacx_smr_batch", ctypes.byref(pcm.c), _ptr(lines), int(bool(short)), _ptr(smr),
                   _ptr(thr), _ptr(npk), self._stream())
        out = [smr]
        if want_threshold:
            out.append(thr)
        if want_peaks:
            out.append(npk)
        return out[0] if len(out) == 1 else tuple(out)

    def smr_generic(self, data, lines, t, want_threshold=False, want_peaks=False):
        """CalcSMRs / getMaskedThreshold for ANY block length (pacx_smr_generic_batch): data [n, N] float64 time
        blocks, lines [n, N/2] = MDCTdata / 2^MDCTscale; t: dict of device tensors hann, tw_cos, tw_sin [N], bark,
        quiet [N/2], band_lower, band_lines (int32) and the floats fft_norm, fft_freq_step (psychoac._generic_tables)."""
        data, lines = data.contiguous(), lines.contiguous()
        n_blocks, n = data.shape
        nb = int(t["band_lines"].numel())
        c = _lib.PacxSmrTables(t["hann"].data_ptr(), t["tw_cos"].data_ptr(), t["tw_sin"].data_ptr(), float(t["fft_norm"]),
                               float(t["fft_freq_step"]), t["bark"].data_ptr(), t["quiet"].data_ptr(),
                               t["band_lower"].data_ptr(), t["band_lines"].data_ptr(), nb)
        smr = self._empty((n_blocks, nb), torch.float64)
        thr = self._empty((n_blocks, n // 2), torch.float64) if want_threshold else None
        npk = self._empty((n_blocks,), torch.int32) if want_peaks else None
        self._call("pacx_smr_generic_batch", ctypes.c_int64(n_blocks), int(n), _ptr(data), _ptr(lines), ctypes.byref(c),
                   _ptr(smr), _ptr(thr), _ptr(npk), self._stream())
        out = [smr] + ([thr] if want_threshold else []) + ([npk] if want_peaks else [])
        return out[0] if len(out) == 1 else tuple(out)

    def bit_alloc(self, smr, n_channels=1, flags=None, short=False):
        smr = smr.contiguous()
        n_cf = smr.shape[0]
        fl = self.flags_tensor(flags, n_cf // n_channels)
        ba = torch.zeros((n_cf, self.band_stride), dtype=torch.int32, device=self.device)
        status = torch.zeros((n_cf,), dtype=torch.int32, device=self.device)
        self._call("pacx_bitalloc_batch", ctypes.c_int64(n_cf), int(n_channels), _ptr(fl),
                   int(bool(short)), _ptr(smr), _ptr(ba), _ptr(status), self._stream())
        return ba, status

    def quantize(self, lines, overall_scale, bit_alloc, short=False):
        n_cf = bit_alloc.shape[0]
        lines = lines.contiguous().view(n_cf, N_LONG)
        sf = torch.zeros((n_cf, self.band_stride), dtype=torch.int32, device=self.device)
        mant = self._empty((n_cf, N_LONG), torch.int32)
        self._call("pacx_quantize_batch", ctypes.c_int64(n_cf), _ptr(lines),
                   _ptr(overall_scale.contiguous()), _ptr(bit_alloc.contiguous()), int(bool(short)),
                   _ptr(sf), _ptr(mant), self._stream())
        return sf, mant

    # -------------------------------------------------------------- whole path
    def _encode(self, pcm, flags, out, default, call):
        """The frame the encode* methods and the curves share: the flags tensor, `out` or default(n_cf),
        call(view, flags pointer, out), and the flags in the dict."""
        fl = self.flags_tensor(flags, pcm.n_frames)
        if out is None:
            out = default(pcm.n_cf)
        call(ctypes.byref(pcm.c), _ptr(fl), out)
        out["flags"] = fl
        return out

    def _pack_outputs(self, n_cf):
        return self.alloc_outputs(n_cf, with_payload=True)

    @staticmethod
    def _pack_ptrs(out, want_mantissa):
        """the outputs of the packing scalar encodes, in the order their entry points take them"""
        return [_ptr(out["overall"]), _ptr(out["scale_factor"]), _ptr(out["bit_alloc"]),
                _ptr(out["mantissa"]) if want_mantissa else None, _ptr(out["status"]), _ptr(out["payload"]),
                _ptr(out["n_bytes"])]

    def encode(self, pcm, flags=None, out=None):
        """codec.Encode for every channel of every frame of `pcm`.
        Returns dict of device tensors: overall [n_cf,8], scale_factor / bit_alloc
        [n_cf, band_stride], mantissa [n_cf,1024] (line-indexed), status [n_cf]."""
        return self._encode(pcm, flags, out, self.alloc_outputs, lambda view, fl, o: self._call(
            "pacx_encode_batch", view, fl, _ptr(o["overall"]), _ptr(o["scale_factor"]), _ptr(o["bit_alloc"]),
            _ptr(o["mantissa"]), _ptr(o["status"]), self._stream()))

    def encode_pack(self, pcm, flags=None, out=None, want_mantissa=False):
        """encode() + pack() in one call (long frames: one fused kernel after the
        masking stage).  `out` as alloc_outputs(n_cf, with_payload=True)."""
        return self._encode(pcm, flags, out, self._pack_outputs, lambda view, fl, o: self._call(
            "pacx_encode_pack_batch", view, fl, *self._pack_ptrs(o, want_mantissa), self._stream()))

    def _call_rate(self, name, *args):
        """the constant-quality entry points: PACX_E_UNSUPPORTED (a gain-shape or SBR handle) is NotImplementedError"""
        rc = getattr(self.lib, name)(self.h, *args)
        if rc == _lib.E_UNSUPPORTED:
            msg = self.lib.pacx_last_error(self.h)
            raise NotImplementedError(f"{name}: {msg.decode() if msg else 'unsupported'}")
        _lib.check(self.lib, self.h, rc, name)

    def encode_pack_nmr(self, pcm, flags, target_nmr_db, max_bits_per_sample, out=None, want_mantissa=False):
        """Constant quality (pacx_encode_pack_nmr_batch, include/pacx.h): every long block and short sub-block gets the
        BitAlloc budget a bisection finds for it -- predicted noise at most target_nmr_db of the mask in every band,
        at most the budget of the cap rate max_bits_per_sample.  Returns encode_pack()'s dict plus budget
        [n_cf, 8] int32 (bits; long frames use [:, 0]); status carries ST_RATE_CAP where the cap was reached."""
        def call(view, fl, o):
            if "budget" not in o:
                o["budget"] = torch.zeros((pcm.n_cf, _lib.SUB), dtype=torch.int32, device=self.device)
            self._call_rate("pacx_encode_pack_nmr_batch", view, fl, ctypes.c_double(target_nmr_db),
                            ctypes.c_double(max_bits_per_sample), *self._pack_ptrs(o, want_mantissa), _ptr(o["budget"]),
                            self._stream())
        return self._encode(pcm, flags, out, self._pack_outputs, call)

    def encode_pack_budget(self, pcm, flags, budget, out=None, want_mantissa=False):
        """encode_pack() with the BitAlloc budget of every long block / short sub-block given by the caller
        (pacx_encode_pack_budget_batch): budget int32 [n_cf, 8] in bits, long frames use [:, 0]."""
        def call(view, fl, o):
            given = self._given(budget, "budget", (pcm.n_cf, _lib.SUB))
            self._call_rate("pacx_encode_pack_budget_batch", view, fl, _ptr(given), *self._pack_ptrs(o, want_mantissa),
                            self._stream())
            o["budget"] = given
        return self._encode(pcm, flags, out, self._pack_outputs, call)

    def _given(self, values, name, shape):
        """the caller's budgets or allocation as an int32 device tensor of this shape"""
        t = torch.as_tensor(values, device=self.device).to(torch.int32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: int32 [{shape[0]}, {shape[1]}]")
        return t

    def rate_curve_layout(self, max_bits_per_sample):
        """(row, sub_stride) of a rate curve with this cap rate (pacx_rate_curve_layout)"""
        row, sub = ctypes.c_int32(0), ctypes.c_int32(0)
        self._call_rate("pacx_rate_curve_layout", ctypes.c_double(max_bits_per_sample), ctypes.byref(row),
                        ctypes.byref(sub))
        return row.value, sub.value

    def rate_curve(self, pcm, flags, max_bits_per_sample, out=None):
        """The rate-distortion curve of every long block / short sub-block (pacx_rate_curve_batch, include/pacx.h):
        for every BitAlloc budget 32 j up to the cap rate's, worst [n_cf, row] float64 (max_b NMR_b, dB) and bits
        [n_cf, row] int32 (what the packer writes); sub-block sb of a short-coded frame at [sb * sub_stride ...].
        steps [n_cf, 8] int32: J of every unit, -1 where there is none.  Entries no unit uses are not written (they
        keep what `out` held; NaN / 0 in a dict made here).  -> dict worst, bits, steps, row, sub_stride."""
        n_cf = pcm.n_cf
        fl = self.flags_tensor(flags, pcm.n_frames)
        row, sub = self.rate_curve_layout(max_bits_per_sample)
        if out is None:
            out = {"worst": torch.full((n_cf, row), float("nan"), dtype=torch.float64, device=self.device),
                   "bits": torch.zeros((n_cf, row), dtype=torch.int32, device=self.device),
                   "steps": torch.full((n_cf, _lib.SUB), -1, dtype=torch.int32, device=self.device)}
        if tuple(out["worst"].shape) != (n_cf, row) or tuple(out["bits"].shape) != (n_cf, row) or \
                tuple(out["steps"].shape) != (n_cf, _lib.SUB):
            raise ValueError(f"rate curve: worst, bits [{n_cf}, {row}], steps [{n_cf}, {_lib.SUB}]")
        self._call_rate("pacx_rate_curve_batch", ctypes.byref(pcm.c), _ptr(fl), ctypes.c_double(max_bits_per_sample),
                        row, _ptr(out["worst"]), _ptr(out["bits"]), _ptr(out["steps"]), self._stream())
        out["row"], out["sub_stride"], out["flags"] = row, sub, fl
        return out

    # ---- the operations on a curve, each written once for both kinds (curves.RATE, curves.BAND): the public methods
    # below are their names, signatures and documentation
    def _checked(self, kind, curve, what, kept=False):
        """The one checker of a curve's arrays, or of a kept curve's: -> (the arrays, n_cf, width, the head arguments
        behind n_cf).  A rate curve's width is its own row, a band curve's the handle's band_stride."""
        arrays = [curve[a.key].contiguous() for a in (kind.kept if kept else kind.curve)]
        if kind.head:
            n_cf, width = arrays[0].shape
        else:
            n_cf, width = arrays[0].shape[0], self.band_stride
        if any(t.dtype != a.dtype or tuple(t.shape) != a.shape(n_cf, width)
               for t, a in zip(arrays, kind.kept if kept else kind.curve)):
            raise ValueError(f"{what}: {kind.as_kept if kept else kind.as_curve}")
        head = [int(width)] + [int(curve[k]) for k in kind.head[1:]] if kind.head else []
        return arrays, n_cf, width, head

    def _curve_call(self, what, checked, *tail):
        """pacx_<what>(handle, n_cf, head, the three arrays, tail, stream)"""
        arrays, n_cf, _, head = checked
        self._call_rate("pacx_" + what, ctypes.c_int64(n_cf), *head, *(_ptr(t) for t in arrays), *tail, self._stream())

    def _picked(self, kind, checked):
        """what a pick or a solve writes per channel-frame"""
        _, n_cf, width, _ = checked
        return {kind.per_cf.key: torch.zeros(kind.per_cf.shape(n_cf, width), dtype=torch.int32, device=self.device),
                "n_bytes": torch.zeros((n_cf,), dtype=torch.int32, device=self.device),
                "capped": torch.zeros((n_cf,), dtype=torch.uint8, device=self.device)}

    def _pick_call(self, kind, what, checked, *middle):
        """the frame of every pick: middle, then the three outputs -> dict budget / bit_alloc, n_bytes, capped (bool)"""
        out = self._picked(kind, checked)
        self._curve_call(what, checked, *middle, _ptr(out[kind.per_cf.key]), _ptr(out["n_bytes"]), _ptr(out["capped"]))
        out["capped"] = out["capped"].bool()
        return out

    @staticmethod
    def _whole_bytes(what, limit_bytes):
        """a limit the C side takes by value"""
        if int(limit_bytes) != limit_bytes or limit_bytes < 0:
            raise ValueError(f"{what}: limit_bytes = {limit_bytes!r}: a whole number of bytes, not negative")
        return ctypes.c_int64(int(limit_bytes))

    @staticmethod
    def _rate_results(res, one=False):
        """pacx_rate_result words (int32 NumPy array [n, 4]: t, met, total as int64 in two of them) -> dict of NumPy
        arrays target_nmr_db, met, total_bytes; one: of the first result's numbers"""
        out = {"target_nmr_db": res[:, 0].astype(np.float64) / float(_lib.RATE_TARGET_GRID), "met": res[:, 1] != 0,
               "total_bytes": res[:, 2:].copy().view(np.int64)[:, 0]}
        if one:
            out = {"target_nmr_db": float(out["target_nmr_db"][0]), "met": bool(out["met"][0]),
                   "total_bytes": int(out["total_bytes"][0])}
        return out

    def _solve(self, kind, op, curve, seg_first, limit_bytes, nmr_lo_db, nmr_hi_db, stream_limit=None):
        """The six solves: op "solve_segments" with seg_first and one limit per segment, "solve_peak" with those (the
        limits are then the peaks) and stream_limit for the whole batch, else "solve", the whole stream with its one
        limit (the plain C entry point).  Checks the curve, makes the outputs, calls pacx_<kind>_<op> and decodes the
        pacx_rate_result of every segment."""
        what, peak = f"{kind.prefix}_{op}", op == "solve_peak"
        segmented = peak or op == "solve_segments"
        checked = self._checked(kind, curve, what)
        n_cf, out = checked[1], self._picked(kind, checked)
        if segmented:
            first, limit = self._segments(what, seg_first, limit_bytes, n_cf)
            limits = [ctypes.c_int64(len(limit)), first.ctypes.data, limit.ctypes.data]
        else:
            limits = [ctypes.c_int64(int(limit_bytes))]
        n_seg = len(limit) if segmented else 1
        # a peak solve's floors and the stream's result ride behind the segments' results: one tensor, one copy back
        result = torch.zeros((n_seg + ((n_seg + 3) // 4 + 1 if peak else 0), 4), dtype=torch.int32, device=self.device)
        if peak:
            limits.append(self._whole_bytes(what, stream_limit))
            more = [_ptr(result[n_seg + 1:]), _ptr(result), _ptr(result[n_seg:])]       # floor, result, result_stream
        else:
            more = [_ptr(result)]
        self._curve_call(what, checked, *limits, ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db),
                         _ptr(out[kind.per_cf.key]), _ptr(out["n_bytes"]), _ptr(out["capped"]), *more)
        res = result.cpu().numpy()
        out["capped"] = out["capped"].bool()
        out.update(self._rate_results(res[:n_seg], one=not segmented))
        if peak:
            out["floor_nmr_db"] = res[n_seg + 1:].reshape(-1)[:n_seg].astype(np.float64) / float(_lib.RATE_TARGET_GRID)
            out.update({"stream_" + k: v for k, v in self._rate_results(res[n_seg:n_seg + 1], one=True).items()})
            out["pinned"] = out["target_nmr_db"] > out["stream_target_nmr_db"]
        return out

    def rate_solve(self, curve, flags, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """One target NMR for the whole stream (pacx_rate_solve, include/pacx.h): the bisection over the grid of
        1/64 dB in [nmr_lo_db, nmr_hi_db] for the smallest target whose body -- every unit at the budget
        encode_pack_nmr's bisection would give it, read from the curve -- stays within limit_bytes.  flags: as
        given to rate_curve (the curve's steps already carry what the solve needs of them).  -> dict
        target_nmr_db, met (False: not even nmr_hi_db fits; the outputs are then that target's), total_bytes,
        budget [n_cf, 8] int32 for encode_pack_budget, n_bytes [n_cf] int32 (predicted), capped [n_cf] bool."""
        return self._solve(RATE, "solve", curve, None, limit_bytes, nmr_lo_db, nmr_hi_db)

    def _profile(self, kind, curve, nmr_lo_db, nmr_hi_db, out):
        what = kind.prefix + "_profile"
        checked = self._checked(kind, curve, what)
        n = self._profile_len(what, nmr_lo_db, nmr_hi_db)
        profile = torch.zeros((n,), dtype=torch.int64, device=self.device) if out is None else \
            self._profile_tensor(what, out, n)
        self._curve_call(what, checked, ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db), _ptr(profile))
        return profile

    def _profile_segments(self, kind, curve, seg_cf, first_off, nmr_lo_db, nmr_hi_db, out):
        what = kind.prefix + "_profile_segments"
        checked = self._checked(kind, curve, what)
        n = self._profile_len(what, nmr_lo_db, nmr_hi_db)
        n_seg = self._uniform_segments(what, checked[1], seg_cf, first_off)
        rows = torch.zeros((n_seg, n), dtype=torch.int64, device=self.device) if out is None else \
            self._profile_rows(what, out, n, n_seg)
        if n_seg == 0:                                                  # no frame and no segment begun: nothing to add to
            return rows
        self._curve_call(what, checked, ctypes.c_int64(int(seg_cf)), ctypes.c_int64(int(first_off)),
                         ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db), _ptr(rows))
        return rows

    def _pick(self, kind, curve, target_nmr_db, kept=False):
        """the pick at one target, on a curve or (kept) on its thresholds, whose range then goes before the target"""
        what = kind.prefix + ("_pick_thresholds" if kept else "_pick")
        checked = self._checked(kind, curve, what, kept)
        return self._pick_call(kind, what, checked, *(self._kept_range(what, curve) if kept else ()),
                               ctypes.c_double(target_nmr_db))

    def _pick_segments(self, kind, curve, seg_cf, first_off, target_t, kept=False):
        """the pick at one target per uniform segment, on a curve or (kept) on its thresholds"""
        what = kind.prefix + ("_pick_thresholds_segments" if kept else "_pick_segments")
        checked = self._checked(kind, curve, what, kept)
        t = self._segment_targets(what, target_t, self._uniform_segments(what, checked[1], seg_cf, first_off))
        return self._pick_call(kind, what, checked, ctypes.c_int64(int(seg_cf)), ctypes.c_int64(int(first_off)),
                               *(self._kept_range(what, curve) if kept else ()), _ptr(t))

    def _thresholds(self, kind, curve, nmr_lo_db, nmr_hi_db, out):
        what = kind.prefix + "_thresholds"
        checked = self._checked(kind, curve, what)
        _, n_cf, width, head = checked
        self._profile_len(what, nmr_lo_db, nmr_hi_db)
        kept = self._kept_out(what, out, {a.key: (a.shape(n_cf, width), a.dtype) for a in kind.kept})
        self._curve_call(what, checked, ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db),
                         *(_ptr(kept[a.key]) for a in kind.kept))
        kept.update(zip(kind.head, head), nmr_lo_db=nmr_lo_db, nmr_hi_db=nmr_hi_db)
        return kept

    @staticmethod
    def _segments(what, seg_first, limit_bytes, n_cf):
        """the host arrays of a segmented solve as int64, checked as the C side checks them"""
        try:
            first = np.ascontiguousarray(np.asarray(seg_first).astype(np.int64, casting="same_kind"))
            limit = np.ascontiguousarray(np.asarray(limit_bytes).astype(np.int64, casting="same_kind"))
        except TypeError:
            raise ValueError(f"{what}: seg_first and limit_bytes are sequences of integers") from None
        if first.ndim != 1 or limit.ndim != 1 or len(limit) < 1 or len(first) != len(limit) + 1:
            raise ValueError(f"{what}: seg_first [n_seg + 1] and limit_bytes [n_seg], n_seg >= 1")
        if first[0] != 0 or first[-1] != n_cf or (np.diff(first) < 0).any():
            raise ValueError(f"{what}: seg_first starts at 0, never decreases and ends at n_cf = {n_cf}")
        if (limit < 0).any():
            raise ValueError(f"{what}: negative limit for segment {int(np.argmax(limit < 0))}")
        return first, limit

    def rate_solve_segments(self, curve, seg_first, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """rate_solve with one limit and one target per stretch of consecutive channel-frames
        (pacx_rate_solve_segments, include/pacx.h): segment s holds the channel-frames seg_first[s] ... seg_first[s + 1]
        - 1 (it may be empty) and gets what rate_solve gives on that slice of the curve with limit_bytes[s]: rate_solve
        is the same solve with the one segment [0, n_cf].  seg_first [n_seg + 1] and limit_bytes [n_seg]: any integer
        sequences.  -> dict budget, n_bytes, capped as rate_solve, and NumPy arrays target_nmr_db [n_seg] float64, met
        [n_seg] bool, total_bytes [n_seg] int64."""
        return self._solve(RATE, "solve_segments", curve, seg_first, limit_bytes, nmr_lo_db, nmr_hi_db)

    def rate_solve_peak(self, curve, seg_first, peak_bytes, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """An average for the stream and a peak for every segment (pacx_rate_solve_peak, include/pacx.h): one target for
        the whole curve within limit_bytes, and for a segment that would exceed its peak_bytes[s] there the lowest
        target at which it fits, its floor.  Segments as rate_solve_segments.  -> dict budget, n_bytes, capped as
        rate_solve; NumPy arrays per segment target_nmr_db (max of the stream's target and the floor), met (the bytes at
        that target against the peak), total_bytes, floor_nmr_db, pinned (target above the stream's); and
        stream_target_nmr_db, stream_met, stream_total_bytes for the whole."""
        return self._solve(RATE, "solve_peak", curve, seg_first, peak_bytes, nmr_lo_db, nmr_hi_db, limit_bytes)

    # ---- a leaky bucket (pacx_bucket_scan and the two buffered solves, include/pacx_bucket.h): bucket is the triple
    # (drain_q16, size_bytes, start_q16) as pacfile.bucket gives it, levels in 1 / 65536 byte
    @staticmethod
    def _hop_channels(what, n_channels, n_cf):
        """the channels of a hop, checked as the C side checks them against the channel-frames"""
        n_ch = int(n_channels)
        if n_ch != n_channels or n_ch < 1 or n_cf % n_ch:
            raise ValueError(f"{what}: n_channels = {n_channels!r}: at least 1, and the {n_cf} channel-frames a whole "
                             f"number of hops")
        return n_ch

    @staticmethod
    def _bucket_struct(what, bucket):
        """the triple as a pacx_bucket; what the numbers may be is the C side's to say"""
        try:
            drain, size, start = (int(v) for v in bucket)
            if (drain, size, start) != tuple(bucket) or max(abs(drain), abs(size), abs(start)) >= 1 << 63:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"{what}: a bucket is three integers (drain_q16, size_bytes, start_q16)") from None
        return _lib.PacxBucket(drain, size, start)

    @staticmethod
    def _bucket_result(words):
        """pacx_bucket_result as int64 words -> dict of its fields, the levels in bytes as float as well"""
        out = {k: int(v) for k, v in zip(_lib.BUCKET_RESULT, words)}
        out.update({"peak_bytes": out["peak_q16"] / 2.0 ** _lib.BUCKET_Q, "end_bytes": out["end_q16"] / 2.0 ** _lib.BUCKET_Q})
        return out

    def _bucket_levels(self, what, n_bytes, n_channels, bucket, want_level, want_through):
        """the two scans: pacx_<what>, which with want_through has one more array to write"""
        nb = torch.as_tensor(n_bytes, device=self.device).to(torch.int32).contiguous().reshape(-1)
        n_ch = self._hop_channels(what, n_channels, nb.numel())
        n_hops = nb.numel() // n_ch
        b = self._bucket_struct(what, bucket)
        per_hop = {k: self._empty((n_hops,), torch.int64) for k, want in (("through", want_through), ("level", want_level))
                   if want}
        result = torch.zeros((len(_lib.BUCKET_RESULT),), dtype=torch.int64, device=self.device)
        self._call("pacx_" + what, ctypes.c_int64(n_hops), n_ch, _ptr(nb), ctypes.byref(b), _ptr(per_hop.get("level")),
                   *([_ptr(per_hop["through"])] if want_through else []), _ptr(result), self._stream())
        out = self._bucket_result(result.cpu().numpy())
        out.update(per_hop)
        return out

    def bucket_scan(self, n_bytes, n_channels, bucket, want_level=False):
        """The level of a leaky bucket over the hops of a stream (pacx_bucket_scan, include/pacx_bucket.h): n_bytes [n_cf]
        int32 as a pick, a solve or a second pass writes it, n_channels consecutive entries a hop.  Every hop adds
        its records with their 4-byte prefixes, then drain_q16 leaves, never below empty.  -> dict total (bytes),
        peak_q16 and peak_hop (the highest level right after a hop's records arrive and the first hop that reaches it;
        -1: the start level is the peak), first_over (the first hop above size_bytes, -1: none), end_q16 (the level
        handed to the next piece of the stream: scans in pieces are exact), peak_bytes and end_bytes as float;
        want_level: also level, int64 device tensor [n_hops] in 1 / 65536 byte."""
        return self._bucket_levels("bucket_scan", n_bytes, n_channels, bucket, want_level, False)

    def rate_solve_bucket(self, curve, flags, n_channels, limit_bytes, bucket, nmr_lo_db=-30, nmr_hi_db=30):
        """rate_solve under a leaky bucket (pacx_rate_solve_bucket, include/pacx_bucket.h): the same bisection for the
        smallest target whose body stays within limit_bytes AND whose level in the bucket, n_channels channel-frames
        a hop, never exceeds size_bytes.  flags: as rate_solve takes them.  -> rate_solve's dict (met False: not even
        nmr_hi_db gives both) plus bucket, bucket_scan's dict of the n_bytes returned."""
        return self._solve_bucket(RATE, curve, n_channels, limit_bytes, bucket, nmr_lo_db, nmr_hi_db)

    # ---- per-block targets under a bucket (pacx_bucket_through and the two pinned solves, include/pacx_bucket_pin.h)
    def bucket_through(self, n_bytes, n_channels, bucket, want_level=False):
        """The level THROUGH every hop of a leaky bucket (pacx_bucket_through, include/pacx_bucket_pin.h): bucket_scan's
        arguments and dict, plus through, int64 device tensor [n_hops] in 1 / 65536 byte: the highest level that any
        stretch of consecutive hops containing the hop brings the buffer to (the start level counts as a stretch that
        begins before the first hop).  A hop lies in a stretch that overflows exactly when its entry is above
        size_bytes << 16.  want_level: also level, as bucket_scan gives it."""
        return self._bucket_levels("bucket_through", n_bytes, n_channels, bucket, want_level, True)

    @staticmethod
    def _pin_args(what, pin_step_db, max_phases):
        """the step of a pinned solve in grid units and its phase count, checked as the C side checks them"""
        try:
            step = float(pin_step_db) * _lib.RATE_TARGET_GRID
            ok = step == int(step) and 1 <= step < 1 << 31
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"{what}: pin_step_db = {pin_step_db!r}: a multiple of 1/{_lib.RATE_TARGET_GRID} dB, at "
                             f"least one of them")
        if isinstance(max_phases, bool) or not isinstance(max_phases, (int, np.integer)) or \
                not 1 <= max_phases <= _lib.PIN_PHASES_MAX:
            raise ValueError(f"{what}: max_phases = {max_phases!r}: a whole number in [1, {_lib.PIN_PHASES_MAX}]")
        return int(step), int(max_phases)

    def _solve_bucket(self, kind, curve, n_channels, limit_bytes, bucket, nmr_lo_db, nmr_hi_db, pinned=None):
        """The four solves under a bucket, pinned = (pin_step_db, max_phases) for the two with a target per hop: checks
        the curve, makes the outputs, calls pacx_<kind>_solve_bucket[_pinned] and decodes the results, which ride in
        one tensor: pacx_rate_result, pacx_bucket_result (five int64 in three rows) and, pinned, pacx_pin_result."""
        what = f"{kind.prefix}_solve_bucket" + ("" if pinned is None else "_pinned")
        pin = () if pinned is None else self._pin_args(what, *pinned)
        checked = self._checked(kind, curve, what)
        n_cf, out = checked[1], self._picked(kind, checked)
        limit = self._whole_bytes(what, limit_bytes)
        n_ch = self._hop_channels(what, n_channels, n_cf)
        checked = checked[:3] + ([ctypes.c_int32(n_ch)] + checked[3],)              # n_ch goes behind n_cf
        b = self._bucket_struct(what, bucket)
        result = torch.zeros((5 if pin else 4, 4), dtype=torch.int32, device=self.device)
        per_hop = torch.zeros((2, n_cf // n_ch), dtype=torch.int32, device=self.device) if pin else ()   # target_t, phase_of
        self._curve_call(what, checked, limit, ctypes.byref(b), ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db),
                         *(ctypes.c_int32(v) for v in pin), _ptr(out[kind.per_cf.key]), _ptr(out["n_bytes"]),
                         _ptr(out["capped"]), *(_ptr(t) for t in per_hop), _ptr(result), _ptr(result[1:]),
                         *([_ptr(result[4:])] if pin else []))
        res = result.cpu().numpy()
        out["capped"] = out["capped"].bool()
        out.update(self._rate_results(res, one=True), bucket=self._bucket_result(res[1:].reshape(-1).view(np.int64)))
        if pin:
            out.update({"target_t": per_hop[0], "phase_of": per_hop[1], "phases": int(res[4, 0]), "open": bool(res[4, 1])})
        return out

    def rate_solve_bucket_pinned(self, curve, flags, n_channels, limit_bytes, bucket, nmr_lo_db=-30, nmr_hi_db=30,
                                 pin_step_db=1.0, max_phases=8):
        """rate_solve_bucket with a target per hop (pacx_rate_solve_bucket_pinned, include/pacx_bucket_pin.h): the
        stream's target wherever the buffer allows, and where a stretch would overflow it a higher one, pinned phase by
        phase (at most max_phases; a pinned hop lies within pin_step_db of the lowest level its stretch allows).
        -> rate_solve_bucket's dict (target_nmr_db: the stream's level, the target of every free hop) plus target_t and
        phase_of, int32 device tensors [n_hops] (grid units; the phase that pinned the hop, -1: free), phases (the
        bisections run) and open (True: the last phase allowed still pinned a hop)."""
        return self._solve_bucket(RATE, curve, n_channels, limit_bytes, bucket, nmr_lo_db, nmr_hi_db,
                                  (pin_step_db, max_phases))

    # ---- the whole-grid profile of a rate curve and the pick at known targets (pacx_rate_profile and its three
    # companions, include/pacx.h): the band siblings below on the other curve, with their checks
    def rate_profile(self, curve, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """band_profile on a rate curve (pacx_rate_profile): int64 device tensor [G], entry g = what rate_pick at
        nmr_lo_db + g / 64 dB gives as sum(n_bytes + 4 where n_bytes > 0) -- rate_solve's total at that target.  With
        `out` the sizes are ADDED to it.  profile_solve on the profile of a whole curve is rate_solve's decision.
        -> the tensor."""
        return self._profile(RATE, curve, nmr_lo_db, nmr_hi_db, out)

    def rate_profile_segments(self, curve, seg_cf, first_off=0, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """band_profile_segments on a rate curve (pacx_rate_profile_segments): int64 device tensor [n_seg, G], row s
        what rate_profile gives for the frames of local segment s; with `out` ADDED to its first n_seg rows, the others
        left alone.  profile_solve_segments and profile_clamp_add take the rows as they take a band curve's.
        -> the tensor."""
        return self._profile_segments(RATE, curve, seg_cf, first_off, nmr_lo_db, nmr_hi_db, out)

    def rate_pick(self, curve, target_nmr_db):
        """Every unit at the budget the curve gives at target_nmr_db, a multiple of 1/64 dB (pacx_rate_pick): what
        rate_solve returns at the target it finds.  -> dict budget [n_cf, 8] int32 for encode_pack_budget, n_bytes
        [n_cf] int32 (predicted), capped [n_cf] bool."""
        return self._pick(RATE, curve, target_nmr_db)

    def rate_pick_segments(self, curve, seg_cf, first_off, target_t):
        """rate_pick with one target per segment (pacx_rate_pick_segments); target_t as band_pick_segments takes it.
        -> rate_pick's dict."""
        return self._pick_segments(RATE, curve, seg_cf, first_off, target_t)

    def band_curve(self, pcm, flags, max_bits_per_sample, out=None):
        """The noise-to-mask ratio of every band at every mantissa size (pacx_band_curve_batch, include/pacx.h): nmr
        [n_cf, band_stride, 16] float64, candidate i = 0 bits for i = 0, else i + 1 (+inf beyond maxMantBits), band
        slots as bit_alloc; cap [n_cf, 8] int32, the cap budget 32 J of every long block / short sub-block, -1 where
        there is none; cap_alloc [n_cf, band_stride] int32, BitAlloc's allocation at that budget.  Slots no band uses
        are not written (they keep what `out` held; NaN in a dict made here).  -> dict nmr, cap, cap_alloc."""
        return self._band_curve("pacx_band_curve_batch", pcm, flags, max_bits_per_sample, out)

    def _band_curve(self, name, pcm, flags, max_bits_per_sample, out):
        """band_curve and vq_band_curve: the same dict from either entry point"""
        n_cf = pcm.n_cf
        shapes = {a.key: a.shape(n_cf, self.band_stride) for a in BAND.curve}

        def default(n_cf):
            return {"nmr": torch.full(shapes["nmr"], float("nan"), dtype=torch.float64, device=self.device),
                    "cap": torch.full(shapes["cap"], -1, dtype=torch.int32, device=self.device),
                    "cap_alloc": torch.zeros(shapes["cap_alloc"], dtype=torch.int32, device=self.device)}

        def call(view, fl, o):
            if any(tuple(o[k].shape) != shape for k, shape in shapes.items()):
                raise ValueError(f"band curve: nmr [{n_cf}, {self.band_stride}, {_lib.BAND_CAND}], cap [{n_cf}, {_lib.SUB}], "
                                 f"cap_alloc [{n_cf}, {self.band_stride}]")
            self._call_rate(name, view, fl, ctypes.c_double(max_bits_per_sample), _ptr(o["nmr"]), _ptr(o["cap"]),
                            _ptr(o["cap_alloc"]), self._stream())
        return self._encode(pcm, flags, out, default, call)

    def band_pick(self, curve, target_nmr_db):
        """Per band the smallest mantissa size whose NMR on the curve is at or below target_nmr_db (pacx_band_pick,
        include/pacx.h); a unit whose bands ask for more than its cap gets cap_alloc.  -> dict bit_alloc
        [n_cf, band_stride] int32 for encode_pack_alloc, n_bytes [n_cf] int32 (predicted), capped [n_cf] bool."""
        return self._pick(BAND, curve, target_nmr_db)

    def band_solve(self, curve, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """rate_solve on a band curve (pacx_band_solve, include/pacx.h): the lowest target on the grid of 1/64 dB in
        [nmr_lo_db, nmr_hi_db] whose body, every band at band_pick's size, stays within limit_bytes.  -> dict
        target_nmr_db, met, total_bytes and band_pick's bit_alloc, n_bytes, capped at that target."""
        return self._solve(BAND, "solve", curve, None, limit_bytes, nmr_lo_db, nmr_hi_db)

    @staticmethod
    def _profile_len(what, nmr_lo_db, nmr_hi_db):
        """G of a profile over this range, checked as the C side checks it"""
        grid = _lib.RATE_TARGET_GRID
        lo, hi = float(nmr_lo_db) * grid, float(nmr_hi_db) * grid
        if not (np.isfinite(lo) and np.isfinite(hi)) or max(abs(lo), abs(hi)) > 2.0 ** 20 * grid or \
                lo != np.floor(lo) or hi != np.floor(hi) or lo > hi:
            raise ValueError(f"{what}: nmr_lo_db <= nmr_hi_db, finite multiples of 1/{grid} dB")
        if hi - lo + 1 > _lib.PROFILE_MAX:
            raise ValueError(f"{what}: a profile holds at most {_lib.PROFILE_MAX} targets "
                             f"(a range of {(_lib.PROFILE_MAX - 1) // grid} dB)")
        return int(hi - lo) + 1

    def _profile_tensor(self, what, profile, n):
        if not isinstance(profile, torch.Tensor) or profile.dtype != torch.int64 or tuple(profile.shape) != (n,) or \
                profile.device != torch.device(self.device) or not profile.is_contiguous():
            raise ValueError(f"{what}: a profile is a contiguous int64 device tensor [{n}] for this range")
        return profile

    def band_profile(self, curve, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """The body size of a band curve at every target of the grid in one pass (pacx_band_profile, include/pacx.h):
        int64 device tensor [G], G = 64 (nmr_hi_db - nmr_lo_db) + 1, entry g = what band_pick at nmr_lo_db + g / 64 dB
        gives as sum(n_bytes + 4 where n_bytes > 0).  With `out` (such a tensor) the sizes are ADDED to it: the profile
        of a stream is the sum of its pieces' in any order, which is what lets a stream too long for one batch be
        solved (profile_solve).  -> the tensor."""
        return self._profile(BAND, curve, nmr_lo_db, nmr_hi_db, out)

    def profile_solve(self, profile, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """band_solve's decision read from a profile (pacx_profile_solve): the lowest target of the range whose size on
        the profile stays within limit_bytes, by the same bisection.  On the profile of a whole curve:
        band_solve(curve, ...)'s target_nmr_db, met, total_bytes.  -> dict of those three."""
        n = self._profile_len("profile_solve", nmr_lo_db, nmr_hi_db)
        profile = self._profile_tensor("profile_solve", profile, n)
        limit = self._whole_bytes("profile_solve", limit_bytes)
        result = torch.zeros((1, 4), dtype=torch.int32, device=self.device)
        self._call_rate("pacx_profile_solve", _ptr(profile), limit, ctypes.c_double(nmr_lo_db),
                        ctypes.c_double(nmr_hi_db), _ptr(result), self._stream())
        return self._rate_results(result.cpu().numpy(), one=True)

    # ---- a profile per uniform segment of a piece (pacx_band_profile_segments and its three companions, include/pacx.h):
    # frame cf of the piece lies in local segment (first_off + cf) // seg_cf
    @staticmethod
    def _uniform_segments(what, n_cf, seg_cf, first_off):
        """n_seg of a piece, the two numbers checked as the C side checks them"""
        if isinstance(seg_cf, bool) or int(seg_cf) != seg_cf or not 1 <= seg_cf <= _lib.SEG_CF_MAX:
            raise ValueError(f"{what}: seg_cf = {seg_cf!r}: a whole number of channel-frames in [1, 2^40]")
        if isinstance(first_off, bool) or int(first_off) != first_off or not 0 <= first_off < seg_cf:
            raise ValueError(f"{what}: first_off = {first_off!r}: a whole number in [0, seg_cf)")
        return -(-(int(first_off) + n_cf) // int(seg_cf))

    def _profile_rows(self, what, rows, n, at_least=1):
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.ndim != 2 or rows.shape[1] != n or \
                rows.shape[0] < at_least or rows.device != torch.device(self.device) or not rows.is_contiguous():
            raise ValueError(f"{what}: profile rows are a contiguous int64 device tensor [n_seg >= {at_least}, {n}] for "
                             f"this range")
        return rows

    def _seg_results(self, what, result, n_seg):
        if not isinstance(result, torch.Tensor) or result.dtype != torch.int32 or tuple(result.shape) != (n_seg, 4) or \
                result.device != torch.device(self.device) or not result.is_contiguous():
            raise ValueError(f"{what}: results are a contiguous int32 device tensor [{n_seg}, 4] (pacx_rate_result)")
        return result

    def band_profile_segments(self, curve, seg_cf, first_off=0, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """band_profile with a row per segment (pacx_band_profile_segments): int64 device tensor [n_seg, G], row s what
        band_profile gives for the frames of local segment s, n_seg = ceil((first_off + n_cf) / seg_cf).  With `out`
        (such a tensor of at least n_seg rows) the sizes are ADDED to its first n_seg rows and the others are left
        alone: a segment cut by the piece gets the rest of its row from the next piece's call.  -> the tensor."""
        return self._profile_segments(BAND, curve, seg_cf, first_off, nmr_lo_db, nmr_hi_db, out)

    def profile_solve_segments(self, rows, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """profile_solve on every row against its own limit (pacx_profile_solve_segments), and per row the largest
        size from the target found on.  limit_bytes: a sequence of whole numbers, one per row, checked here (none
        negative) and sent up; or an int64 device tensor [n_seg] the caller has checked.  -> dict of NumPy arrays
        target_nmr_db, met, total_bytes, worst_above [n_seg] and "result", the pacx_rate_result words as an int32
        device tensor [n_seg, 4] (profile_clamp_add takes it).  out = (result, worst_above), device tensors int32
        [n_seg, 4] and int64 [n_seg]: written instead, nothing is read back and the host does not wait -> out."""
        what = "profile_solve_segments"
        n = self._profile_len(what, nmr_lo_db, nmr_hi_db)
        rows = self._profile_rows(what, rows, n)
        n_seg = rows.shape[0]
        if isinstance(limit_bytes, torch.Tensor):
            limit = limit_bytes
            if limit.dtype != torch.int64 or tuple(limit.shape) != (n_seg,) or limit.device != rows.device or \
                    not limit.is_contiguous():
                raise ValueError(f"{what}: limits on the device are a contiguous int64 tensor [{n_seg}]")
        else:
            try:
                host = np.ascontiguousarray(np.asarray(limit_bytes).astype(np.int64, casting="same_kind"))
            except TypeError:
                raise ValueError(f"{what}: limit_bytes is a sequence of integers") from None
            if host.shape != (n_seg,):
                raise ValueError(f"{what}: one limit per row, limit_bytes [{n_seg}]")
            if (host < 0).any():
                raise ValueError(f"{what}: negative limit for segment {int(np.argmax(host < 0))}")
            limit = torch.as_tensor(host).to(self.device)
        if out is None:
            result = torch.zeros((n_seg, 4), dtype=torch.int32, device=self.device)
            worst = torch.zeros((n_seg,), dtype=torch.int64, device=self.device)
        else:
            result, worst = out
            self._seg_results(what, result, n_seg)
            if not isinstance(worst, torch.Tensor) or worst.dtype != torch.int64 or tuple(worst.shape) != (n_seg,) or \
                    worst.device != rows.device or not worst.is_contiguous():
                raise ValueError(f"{what}: worst_above is a contiguous int64 device tensor [{n_seg}]")
        self._call_rate("pacx_profile_solve_segments", ctypes.c_int64(n_seg), _ptr(rows), _ptr(limit),
                        ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db), _ptr(result), _ptr(worst), self._stream())
        if out is not None:
            return out
        res = self.decode_results(result)
        res.update(worst_above=worst.cpu().numpy(), result=result)
        return res

    @staticmethod
    def decode_results(result):
        """pacx_rate_result words (int32 device tensor [n, 4]) -> dict of NumPy arrays target_nmr_db, met, total_bytes"""
        return Encoder._rate_results(result.cpu().numpy())

    def profile_clamp_add(self, rows, result, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """Every row held at its own target's size below that target, summed into one profile (pacx_profile_clamp_add):
        out[g] += sum over s of rows[s][max(g, t_s - t_lo)], t_s from `result` (profile_solve_segments' "result").  With
        the targets the floors of a peak solve, the sum over a stream's segments is the size of the stream at every
        stream target, and profile_solve on it is the peak solve's decision.  out: a profile [G], added to (zeros when
        not given).  -> the tensor."""
        what = "profile_clamp_add"
        n = self._profile_len(what, nmr_lo_db, nmr_hi_db)
        rows = self._profile_rows(what, rows, n)
        result = self._seg_results(what, result, rows.shape[0])
        profile = torch.zeros((n,), dtype=torch.int64, device=self.device) if out is None else \
            self._profile_tensor(what, out, n)
        self._call_rate("pacx_profile_clamp_add", ctypes.c_int64(rows.shape[0]), _ptr(rows), _ptr(result),
                        ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db), _ptr(profile), self._stream())
        return profile

    def _segment_targets(self, what, target_t, n_seg):
        """one target per local segment in whole grid units -> a contiguous int32 device tensor [n_seg]"""
        if isinstance(target_t, torch.Tensor):
            t = target_t
            if t.dtype != torch.int32 or tuple(t.shape) != (n_seg,) or t.device != torch.device(self.device) or \
                    not t.is_contiguous():
                raise ValueError(f"{what}: targets on the device are a contiguous int32 tensor [{n_seg}]")
            return t
        host = np.asarray(target_t)
        if host.shape != (n_seg,) or not np.array_equal(host, np.round(host)) or (np.abs(host) > 2 ** 26).any():
            raise ValueError(f"{what}: target_t [{n_seg}], whole grid units")
        return torch.as_tensor(np.ascontiguousarray(host.astype(np.int32))).to(self.device)

    def band_pick_segments(self, curve, seg_cf, first_off, target_t):
        """band_pick with one target per segment (pacx_band_pick_segments): target_t, whole grid units (64 per dB), one
        per local segment -- a sequence, or an int32 device tensor [n_seg].  -> band_pick's dict."""
        return self._pick_segments(BAND, curve, seg_cf, first_off, target_t)

    # ---- a curve kept as 16-bit thresholds and the picks on it (pacx_band_thresholds and its five companions,
    # include/pacx.h): what a chunked encode keeps between its passes instead of taking every curve twice
    def _kept_out(self, what, out, shapes):
        """the arrays of a kept curve: made here, or the caller's (contiguous device tensors of these shapes and types)"""
        if out is None:
            return {k: torch.empty(shape, dtype=dtype, device=self.device) for k, (shape, dtype) in shapes.items()}
        for k, (shape, dtype) in shapes.items():
            t = out.get(k)
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or \
                    t.device != torch.device(self.device) or not t.is_contiguous():
                raise ValueError(f"{what}: out[{k!r}] is a contiguous {dtype} device tensor {list(shape)}")
        return {k: out[k] for k in shapes}

    def _kept_range(self, what, kept):
        lo, hi = kept["nmr_lo_db"], kept["nmr_hi_db"]
        self._profile_len(what, lo, hi)
        return ctypes.c_double(lo), ctypes.c_double(hi)

    def band_thresholds(self, curve, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """A band curve in the form that decides a pick on the grid of 1/64 dB in [nmr_lo_db, nmr_hi_db]
        (pacx_band_thresholds, include/pacx.h): e [n_cf, band_stride, 16] uint16, the grid index from which each size
        passes (G = the number of grid targets where it never does, and in every entry no band uses), cap copied,
        cap_alloc as uint8: a quarter of the curve's bytes.  band_pick_thresholds[_segments] on it give band_pick's
        outputs at every grid target of the range.  out: a dict with e, cap, cap_alloc to write into.  -> dict e, cap,
        cap_alloc, nmr_lo_db, nmr_hi_db."""
        return self._thresholds(BAND, curve, nmr_lo_db, nmr_hi_db, out)

    def band_pick_thresholds(self, kept, target_nmr_db):
        """band_pick on a kept curve (pacx_band_pick_thresholds): target_nmr_db a multiple of 1/64 dB inside the range
        the thresholds were made for.  -> band_pick's dict, equal to band_pick's on the curve itself."""
        return self._pick(BAND, kept, target_nmr_db, kept=True)

    def band_pick_thresholds_segments(self, kept, seg_cf, first_off, target_t):
        """band_pick_segments on a kept curve (pacx_band_pick_thresholds_segments); target_t as band_pick_segments takes
        it, every target inside the range.  -> band_pick's dict."""
        return self._pick_segments(BAND, kept, seg_cf, first_off, target_t, kept=True)

    def rate_thresholds(self, curve, nmr_lo_db=-30, nmr_hi_db=30, out=None):
        """band_thresholds for a rate curve (pacx_rate_thresholds): e [n_cf, row] uint16, bits copied (0 where no unit
        uses the entry), steps with a J that would leave its row cut to the row: half of the curve's bytes.  out: a dict
        with e, bits, steps to write into.  -> dict e, bits, steps, row, sub_stride, nmr_lo_db, nmr_hi_db."""
        return self._thresholds(RATE, curve, nmr_lo_db, nmr_hi_db, out)

    def rate_pick_thresholds(self, kept, target_nmr_db):
        """rate_pick on a kept curve (pacx_rate_pick_thresholds): target_nmr_db a multiple of 1/64 dB inside the range
        the thresholds were made for.  -> rate_pick's dict, equal to rate_pick's on the curve itself."""
        return self._pick(RATE, kept, target_nmr_db, kept=True)

    def rate_pick_thresholds_segments(self, kept, seg_cf, first_off, target_t):
        """rate_pick_segments on a kept curve (pacx_rate_pick_thresholds_segments).  -> rate_pick's dict."""
        return self._pick_segments(RATE, kept, seg_cf, first_off, target_t, kept=True)

    # ---- the buffered solve for a stream in chunks, on kept curves (include/pacx_bucket_kept.h): a chunk's bytes at
    # every target of a pass, the scans of those targets carried from chunk to chunk, the tree of the next decisions
    def _tree_targets(self, what, target_t):
        """1 ... 31 grid targets -> a contiguous int32 device tensor [n]"""
        if isinstance(target_t, torch.Tensor):
            t = target_t
            if t.dtype != torch.int32 or t.ndim != 1 or t.device != torch.device(self.device) or not t.is_contiguous():
                raise ValueError(f"{what}: targets on the device are a contiguous int32 tensor [n_targets]")
        else:
            host = np.asarray(target_t)
            if host.ndim != 1 or not np.array_equal(host, np.round(host)) or (np.abs(host) > 2 ** 26).any():
                raise ValueError(f"{what}: target_t [n_targets], whole grid units")
            t = torch.as_tensor(np.ascontiguousarray(host.astype(np.int32))).to(self.device)
        if not 1 <= t.numel() <= _lib.BUCKET_TREE_TARGETS:
            raise ValueError(f"{what}: between 1 and {_lib.BUCKET_TREE_TARGETS} targets")
        return t

    def _bytes_thresholds(self, kind, kept, target_t, out):
        what = kind.prefix + "_bytes_thresholds"
        checked = self._checked(kind, kept, what, True)
        n_cf, t = checked[1], self._tree_targets(what, target_t)
        shape = (t.numel(), n_cf)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != shape or \
                out.device != torch.device(self.device) or not out.is_contiguous():
            raise ValueError(f"{what}: out is a contiguous int32 device tensor {list(shape)}")
        self._curve_call(what, checked, *self._kept_range(what, kept), ctypes.c_int32(t.numel()), _ptr(t), _ptr(out))
        return out

    def band_bytes_thresholds(self, kept, target_t, out=None):
        """The n_bytes of band_pick_thresholds at several targets in one pass over the kept curve
        (pacx_band_bytes_thresholds, include/pacx_bucket_kept.h): target_t, 1 ... 31 whole grid units (64 per dB, clamped
        into the curve's range) -- a sequence, or an int32 device tensor [n_targets].  -> int32 device tensor
        [n_targets, n_cf] (`out`, if given), row m what band_pick_thresholds gives as n_bytes at target_t[m] / 64 dB."""
        return self._bytes_thresholds(BAND, kept, target_t, out)

    def rate_bytes_thresholds(self, kept, target_t, out=None):
        """band_bytes_thresholds on a kept rate curve (pacx_rate_bytes_thresholds): row m is rate_pick_thresholds'
        n_bytes at target_t[m] / 64 dB."""
        return self._bytes_thresholds(RATE, kept, target_t, out)

    @staticmethod
    def bucket_no_hop(bucket, n=1):
        """the scan of no hop from the bucket's start level, n times: int64 NumPy array [n, 5] in the order of
        _lib.BUCKET_RESULT -- what bucket_scan_targets starts from"""
        start = int(bucket[2])
        return np.tile(np.array([0, start, -1, -1, start], np.int64), (int(n), 1))

    def bucket_scan_targets(self, n_bytes_t, n_channels, drain_q16, size_bytes, hop_off, acc):
        """bucket_scan of one piece of a stream at several targets, folded into the scans of the pieces before it
        (pacx_bucket_scan_targets): n_bytes_t int32 device tensor [n_targets, n_cf] (rows may lie further apart), row m
        the piece's n_bytes at target m; acc int64 device tensor [n_targets, 5] in the order of _lib.BUCKET_RESULT,
        in and out; hop_off: the hops of the stream before the piece.  Row m's scan starts at acc[m]'s end_q16.  From
        bucket_no_hop() on, acc[m] after the pieces of a stream in order is bucket_scan of the whole row.  -> acc."""
        what = "bucket_scan_targets"
        nb = n_bytes_t
        if not isinstance(nb, torch.Tensor) or nb.dtype != torch.int32 or nb.ndim != 2 or \
                nb.device != torch.device(self.device) or (nb.shape[1] > 1 and nb.stride(1) != 1) or \
                (nb.shape[0] > 1 and nb.stride(0) < nb.shape[1]):
            raise ValueError(f"{what}: n_bytes_t is an int32 device tensor [n_targets, n_cf] with contiguous rows")
        n, n_cf = nb.shape
        n_ch = self._hop_channels(what, n_channels, n_cf)
        if not isinstance(acc, torch.Tensor) or acc.dtype != torch.int64 or tuple(acc.shape) != (n, len(_lib.BUCKET_RESULT)) \
                or acc.device != torch.device(self.device) or not acc.is_contiguous():
            raise ValueError(f"{what}: acc is a contiguous int64 device tensor [{n}, {len(_lib.BUCKET_RESULT)}]")
        if int(hop_off) != hop_off:
            raise ValueError(f"{what}: hop_off = {hop_off!r}: a whole number of hops")
        self._call("pacx_" + what, ctypes.c_int64(n_cf // n_ch), n_ch, n, _ptr(nb),
                   ctypes.c_int64(nb.stride(0) if n > 1 else max(n_cf, 1)), ctypes.c_int64(int(drain_q16)),
                   ctypes.c_int64(int(size_bytes)), ctypes.c_int64(int(hop_off)), _ptr(acc), self._stream())
        return acc

    @staticmethod
    def _tree_levels(what, levels):
        if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or \
                not 1 <= levels <= _lib.BUCKET_TREE_LEVELS_MAX:
            raise ValueError(f"{what}: levels = {levels!r}: a whole number in [1, {_lib.BUCKET_TREE_LEVELS_MAX}]")
        return int(levels)

    @staticmethod
    def bucket_tree_passes(nmr_lo_db, nmr_hi_db, levels):
        """the passes of a solve on this range with this many decisions a pass: ceil((P - 1) / levels), P the pairs of
        rate_solve_bucket, 2 + ceil(log2(G + 1))"""
        g = int(round((float(nmr_hi_db) - float(nmr_lo_db)) * _lib.RATE_TARGET_GRID)) + 1
        return -(-(1 + (g).bit_length()) // int(levels))

    def bucket_tree_begin(self, bucket, nmr_lo_db=-30, nmr_hi_db=30, levels=4, tree=None):
        """Start a buffered solve whose probes are evaluated a tree at a time (pacx_bucket_tree_begin,
        include/pacx_bucket_kept.h).  -> tree, a dict of device tensors the caller hands to every call of the solve
        (made here, or the one given, used again): state (uint8 [128]), target_t (int32 [31], the first 2^levels - 1 the
        targets of the next pass in heap order), acc (int64 [31, 5], every row the scan of no hop), result (the two
        results, read by bucket_tree_result)."""
        what = "bucket_tree_begin"
        levels = self._tree_levels(what, levels)
        b = self._bucket_struct(what, bucket)
        if tree is None:
            tree = {"state": torch.zeros((_lib.BUCKET_TREE_STATE_BYTES,), dtype=torch.uint8, device=self.device),
                    "target_t": torch.zeros((_lib.BUCKET_TREE_TARGETS,), dtype=torch.int32, device=self.device),
                    "acc": torch.zeros((_lib.BUCKET_TREE_TARGETS, len(_lib.BUCKET_RESULT)), dtype=torch.int64,
                                       device=self.device),
                    "result": torch.zeros((4, 4), dtype=torch.int32, device=self.device)}
        self._call("pacx_" + what, ctypes.byref(b), ctypes.c_double(nmr_lo_db), ctypes.c_double(nmr_hi_db), levels,
                   _ptr(tree["state"]), _ptr(tree["target_t"]), _ptr(tree["acc"]), self._stream())
        return tree

    def bucket_tree_step(self, limit_bytes, bucket, levels, tree):
        """The decisions a pass allows (pacx_bucket_tree_step): walks tree["acc"] -- row k the scan of the whole stream at
        tree["target_t"][k], as bucket_scan_targets leaves it -- from slot 0 by rate_solve_bucket's decision, at most
        `levels` times, then writes the next pass's targets, resets acc and writes the results.  Nothing is read
        back.  -> tree."""
        what = "bucket_tree_step"
        levels = self._tree_levels(what, levels)
        b = self._bucket_struct(what, bucket)
        self._call("pacx_" + what, self._whole_bytes(what, limit_bytes), ctypes.byref(b), levels, _ptr(tree["state"]),
                   _ptr(tree["target_t"]), _ptr(tree["acc"]), _ptr(tree["result"]), _ptr(tree["result"][1:]),
                   self._stream())
        return tree

    def bucket_tree_result(self, tree):
        """the results of the last bucket_tree_step, read back: dict target_nmr_db, met, total_bytes and bucket
        (bucket_scan's dict): rate_solve_bucket's once bucket_tree_passes() steps have run"""
        res = tree["result"].cpu().numpy()
        return dict(self._rate_results(res, one=True), bucket=self._bucket_result(res[1:].reshape(-1).view(np.int64)))

    def band_solve_segments(self, curve, seg_first, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """band_solve with one limit and one target per stretch of consecutive channel-frames
        (pacx_band_solve_segments, include/pacx.h); segments and results as rate_solve_segments.  -> dict bit_alloc,
        n_bytes, capped as band_solve, and NumPy arrays target_nmr_db, met, total_bytes [n_seg]."""
        return self._solve(BAND, "solve_segments", curve, seg_first, limit_bytes, nmr_lo_db, nmr_hi_db)

    def band_solve_peak(self, curve, seg_first, peak_bytes, limit_bytes, nmr_lo_db=-30, nmr_hi_db=30):
        """rate_solve_peak on a band curve (pacx_band_solve_peak, include/pacx.h).  -> dict bit_alloc, n_bytes, capped as
        band_solve and rate_solve_peak's results per segment and for the stream."""
        return self._solve(BAND, "solve_peak", curve, seg_first, peak_bytes, nmr_lo_db, nmr_hi_db, limit_bytes)

    def band_solve_bucket(self, curve, n_channels, limit_bytes, bucket, nmr_lo_db=-30, nmr_hi_db=30):
        """rate_solve_bucket on a band curve (pacx_band_solve_bucket, include/pacx_bucket.h).  -> band_solve's dict plus
        bucket, bucket_scan's dict of the n_bytes returned."""
        return self._solve_bucket(BAND, curve, n_channels, limit_bytes, bucket, nmr_lo_db, nmr_hi_db)

    def band_solve_bucket_pinned(self, curve, n_channels, limit_bytes, bucket, nmr_lo_db=-30, nmr_hi_db=30,
                                 pin_step_db=1.0, max_phases=8):
        """rate_solve_bucket_pinned on a band curve (pacx_band_solve_bucket_pinned, include/pacx_bucket_pin.h).
        -> band_solve_bucket's dict plus target_t, phase_of, phases and open."""
        return self._solve_bucket(BAND, curve, n_channels, limit_bytes, bucket, nmr_lo_db, nmr_hi_db,
                                  (pin_step_db, max_phases))

    def encode_pack_alloc(self, pcm, flags, bit_alloc, out=None, want_mantissa=False):
        """encode_pack() with the mantissa size of every band given by the caller (pacx_encode_pack_alloc_batch):
        bit_alloc int32 [n_cf, band_stride]; values below 2 count as 0, values above maxMantBits as maxMantBits, and
        out["bit_alloc"] holds what was coded."""
        def call(view, fl, o):
            given = self._given(bit_alloc, "bit_alloc", (pcm.n_cf, self.band_stride))
            self._call_rate("pacx_encode_pack_alloc_batch", view, fl, _ptr(given), *self._pack_ptrs(o, want_mantissa),
                            self._stream())
        return self._encode(pcm, flags, out, self._pack_outputs, call)

    def encode_vq(self, pcm, flags=None, out=None, want_entries=False, entries_per_band=160):
        """The shipped configuration (gain-shape PVQ, SBR if the handle has it) from
        PCM to finished payloads.  Returns dict: overall [n_cf,8], bit_alloc
        [n_cf, band_stride] (final), payload [n_cf, payload_stride], n_bytes, status;
        with want_entries also entries [n_cf,8,32,cap] (structured: value, width,
        band) and entry_count [n_cf,8,32]."""
        def call(view, fl, o):
            ent = cnt = None
            if want_entries:
                ent = torch.zeros((pcm.n_cf, _lib.SUB, _lib.MAX_BANDS, entries_per_band, 2), dtype=torch.int64,
                                  device=self.device)
                cnt = torch.zeros((pcm.n_cf, _lib.SUB, _lib.MAX_BANDS), dtype=torch.int32, device=self.device)
            self._call("pacx_encode_vq_batch", view, fl, *self._vq_ptrs(o), _ptr(ent), _ptr(cnt),
                       ctypes.c_int32(entries_per_band if want_entries else 0), self._stream())
            if want_entries:
                o["entries"], o["entry_count"] = ent, cnt
        return self._encode(pcm, flags, out, self.alloc_vq_outputs, call)

    def vq_band_curve(self, pcm, flags, max_bits_per_sample, out=None):
        """band_curve for a gain-shape handle without SBR (pacx_vq_band_curve_batch, include/pacx.h): the same dict in
        the same layout, every column taken with the gain-shape coder and its decoder themselves -- candidate i is every
        band coded with (i + 1) x lines bits.  A band whose lines are all zero holds -inf (it codes nothing at any
        size).  The pick and the solves run on the scalar sibling of this handle (context.scalar_sibling), the second
        pass is encode_vq_alloc."""
        return self._band_curve("pacx_vq_band_curve_batch", pcm, flags, max_bits_per_sample, out)

    def encode_vq_alloc(self, pcm, flags, bit_alloc, out=None):
        """encode_vq() with the allocation of every band given by the caller (pacx_encode_vq_alloc_batch): bit_alloc
        int32 [n_cf, band_stride]; values below 2 count as 0, values above maxMantBits as maxMantBits, and
        out["bit_alloc"] holds what was coded (a band whose lines are all zero drops to 0).  -> encode_vq's dict."""
        def call(view, fl, o):
            given = self._given(bit_alloc, "bit_alloc", (pcm.n_cf, self.band_stride))
            self._call_rate("pacx_encode_vq_alloc_batch", view, fl, _ptr(given), *self._vq_ptrs(o), self._stream())
        return self._encode(pcm, flags, out, self.alloc_vq_outputs, call)

    @staticmethod
    def _vq_ptrs(out):
        """the outputs of the gain-shape encodes, in the order their entry points take them"""
        return [_ptr(out["overall"]), _ptr(out["bit_alloc"]), _ptr(out["payload"]), _ptr(out["n_bytes"]), _ptr(out["status"])]

    def alloc_vq_outputs(self, n_cf, with_payload=True):
        """what the gain-shape coder writes per channel-frame (the decoder reads the first three back)"""
        o = {
            "overall": self._empty((n_cf, _lib.SUB), torch.int32),
            "bit_alloc": torch.zeros((n_cf, self.band_stride), dtype=torch.int32, device=self.device),
            "status": self._empty((n_cf,), torch.int32),
        }
        if with_payload:
            o["payload"] = self._empty((n_cf, self.payload_stride), torch.uint8)
            o["n_bytes"] = self._empty((n_cf,), torch.int32)
        return o

    def alloc_outputs(self, n_cf, with_payload=False):
        o = {
            "overall": self._empty((n_cf, _lib.SUB), torch.int32),
            "scale_factor": torch.zeros((n_cf, self.band_stride), dtype=torch.int32, device=self.device),
            "bit_alloc": torch.zeros((n_cf, self.band_stride), dtype=torch.int32, device=self.device),
            "mantissa": self._empty((n_cf, N_LONG), torch.int32),
            "status": self._empty((n_cf,), torch.int32),
        }
        if with_payload:
            o["payload"] = self._empty((n_cf, self.payload_stride), torch.uint8)
            o["n_bytes"] = self._empty((n_cf,), torch.int32)
        return o

    def pack(self, enc, n_channels, out=None):
        """.pac payload of every cf: payload [n_cf, payload_stride] uint8, n_bytes [n_cf]."""
        n_cf = enc["bit_alloc"].shape[0]
        payload = out["payload"] if out else self._empty((n_cf, self.payload_stride), torch.uint8)
        n_bytes = out["n_bytes"] if out else self._empty((n_cf,), torch.int32)
        self._call("pacx_pack_batch", ctypes.c_int64(n_cf), int(n_channels), _ptr(enc.get("flags")),
                   _ptr(enc["overall"]), _ptr(enc["scale_factor"]), _ptr(enc["bit_alloc"]),
                   _ptr(enc["mantissa"]), _ptr(enc["status"]), _ptr(payload), _ptr(n_bytes),
                   self._stream())
        return payload, n_bytes

    def gather_body(self, payload, n_bytes, capacity=None, out=None):
        """'<L nBytes' + payload of every cf, back to back (the .pac body).  `out`: a uint8 device
        tensor to write into (e.g. a gather slot of dist.BitstreamGather); its length is the capacity."""
        n_cf = n_bytes.shape[0]
        if out is not None:
            capacity = out.numel()
        elif capacity is None:
            capacity = n_cf * (self.payload_stride + 4)
        body = out if out is not None else self._empty((capacity,), torch.uint8)
        total = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._call("pacx_gather_body", ctypes.c_int64(n_cf), _ptr(payload), _ptr(n_bytes), _ptr(body),
                   ctypes.c_int64(capacity), _ptr(total), self._stream())
        return body, total

    def transient_flags(self, planar, n_hops, hop=N_LONG):
        """Block-switching flags on the GPU for a device stream laid out as
        pacfile.device_stream builds it ([nCh, (n_hops+3)*hop]: zeros, the hops, the
        last hop again, zeros).  Returns (transient uint8[n_hops], flags uint8[n_hops+2])."""
        n_ch, n = planar.shape
        view = _lib.PacxPcm(planar.data_ptr() + 2 * hop, _lib.PCM_I16, n_ch, int(n_hops), hop, n, 1)
        tr = self._empty((max(n_hops, 1),), torch.uint8)
        fl = self._empty((n_hops + 2,), torch.uint8)
        self._call("pacx_transient_flags", ctypes.byref(view), _ptr(tr), _ptr(fl), self._stream())
        return tr[:n_hops], fl

    # ------------------------------------------------------------ decode side
    def unpack(self, payload, n_bytes, offsets=None):
        """Parse packed channel-blocks (slot layout, or a byte stream + int64 offsets).
        out["status"] carries PACX_ST_MALFORMED for a record that is truncated or corrupt."""
        n_cf = n_bytes.shape[0]
        out = self.alloc_outputs(n_cf)
        out["flags"] = self._empty((n_cf,), torch.uint8)
        stride = 0 if offsets is not None else int(payload.shape[1])
        self._call("pacx_unpack_batch", ctypes.c_int64(n_cf), _ptr(payload), stride, _ptr(offsets),
                   _ptr(n_bytes), _ptr(out["flags"]), _ptr(out["overall"]), _ptr(out["scale_factor"]),
                   _ptr(out["bit_alloc"]), _ptr(out["mantissa"]), _ptr(out["status"]), self._stream())
        return out

    def decode(self, codes, n_channels, want_blocks=False, want_pcm=True, extra=None, every_long_block=False):
        """codec.Decode + overlap-and-add + PCM for blocks in stream order.
        codes: dict with flags (per cf), overall, scale_factor, bit_alloc, mantissa.
        extra (a dict): route the blocks of an SBR file with scalar mantissas as PACFile.Decode does
        (coder/pacfile.py:645-668: long blocks with a coded omitted band through Decode_SBR's scalar
        branch; every_long_block: Decode_SBR on all of them); it receives "status"
        (PACX_ST_VQ_UNDEFINED where Decode_SBR raises IndexError) and "lines" (dequantised,
        reconstructed, before / 2^overall)."""
        n_cf = codes["bit_alloc"].shape[0]
        n_blocks = n_cf // n_channels
        blocks = self._empty((n_cf, 2 * N_LONG), torch.float64) if want_blocks else None
        pcm = self._empty(((n_blocks + 1) * N_LONG, n_channels), torch.int16) if want_pcm else None
        if extra is not None:
            extra["status"] = self._empty((n_cf,), torch.int32)
            extra["lines"] = self._empty((n_cf, N_LONG), torch.float64)
            self._call("pacx_decode_sbr_batch", ctypes.c_int64(n_blocks), int(n_channels), _ptr(codes["flags"]),
                       _ptr(codes["overall"]), _ptr(codes["scale_factor"]), _ptr(codes["bit_alloc"]),
                       _ptr(codes["mantissa"]), int(bool(every_long_block)), _ptr(extra["lines"]), _ptr(blocks), _ptr(pcm),
                       _ptr(extra["status"]), self._stream())
        else:
            self._call("pacx_decode_batch", ctypes.c_int64(n_blocks), int(n_channels), _ptr(codes["flags"]),
                       _ptr(codes["overall"]), _ptr(codes["scale_factor"]), _ptr(codes["bit_alloc"]),
                       _ptr(codes["mantissa"]), _ptr(blocks), _ptr(pcm), self._stream())
        return (blocks, pcm) if want_blocks and want_pcm else (blocks if want_blocks else pcm)

    def decode_vq(self, payload, n_bytes, n_channels, offsets=None, want_lines=False, want_blocks=False,
                  want_pcm=True):
        """Gain-shape coded channel-blocks (slot layout, or byte stream + int64
        offsets) -> dict: flags, overall, bit_alloc, status and, as requested,
        lines [n_cf,1024], blocks [n_cf,2048], pcm int16 [(n_blocks+1)*1024, nCh]."""
        n_cf = n_bytes.shape[0]
        n_blocks = n_cf // n_channels
        out = {
            "flags": self._empty((n_cf,), torch.uint8),
            **self.alloc_vq_outputs(n_cf, with_payload=False),
            "lines": self._empty((n_cf, N_LONG), torch.float64) if want_lines else None,
            "blocks": self._empty((n_cf, 2 * N_LONG), torch.float64) if want_blocks else None,
            "pcm": self._empty(((n_blocks + 1) * N_LONG, n_channels), torch.int16) if want_pcm else None,
        }
        stride = 0 if offsets is not None else int(payload.shape[1])
        self._call("pacx_decode_vq_batch", ctypes.c_int64(n_blocks), int(n_channels), _ptr(payload), stride,
                   _ptr(offsets), _ptr(n_bytes), _ptr(out["flags"]), _ptr(out["overall"]),
                   _ptr(out["bit_alloc"]), _ptr(out["lines"]), _ptr(out["blocks"]), _ptr(out["pcm"]),
                   _ptr(out["status"]), self._stream())
        return out

    def index_body(self, body, n_channels, final=True, max_records=None):
        """Record index of a .pac body that sits on the device (uint8 tensor starting at a length prefix), built
        there (pacx_index_body): offsets int64 / n_bytes int32 [max_records] as unpack / decode_vq take them and
        result int64 [3] = records returned (a multiple of n_channels), bytes consumed, position of the prefix at
        which the chain broke or -1.  max_records None: as many as the body can hold."""
        n_body = int(body.numel())
        if max_records is None:
            max_records = n_body // 5                  # a record is five bytes at least
        max_records = int(max_records)
        offsets = self._empty((max_records,), torch.int64)
        n_bytes = self._empty((max_records,), torch.int32)
        result = self._empty((3,), torch.int64)
        self._call("pacx_index_body", _ptr(body), ctypes.c_int64(n_body), int(n_channels), int(bool(final)),
                   ctypes.c_int64(max_records), _ptr(offsets), _ptr(n_bytes), _ptr(result), self._stream())
        return offsets, n_bytes, result

    def overlap_add(self, blocks, tail, flush):
        """Overlap-and-add + PCM of one batch of a longer stream (pacx_overlap_add_pcm).  blocks: float64
        [n_blocks*nCh, 2048] in stream order; tail: float64 [nCh, 1024], the half-block carried across the batch
        boundary, updated in place.  -> int16 [(n_blocks + flush)*1024, nCh]."""
        n_ch = int(tail.shape[0])
        assert tail.is_contiguous() and tail.dtype == torch.float64 and tail.shape[1] == N_LONG
        blocks = blocks.contiguous()
        n_blocks = blocks.shape[0] // n_ch
        pcm = self._empty(((n_blocks + int(bool(flush))) * N_LONG, n_ch), torch.int16)
        self._call("pacx_overlap_add_pcm", ctypes.c_int64(n_blocks), n_ch, _ptr(blocks), _ptr(tail), int(bool(flush)),
                   _ptr(pcm), self._stream())
        return pcm

    # --------------------------------------------------- quality of an encode
    def nmr(self, view, flags, dec_lines, overall_scale, status=None):
        """Noise-to-mask ratio of every band of every coded block (pacx_nmr_batch, include/pacx.h): view is the
        ORIGINAL PCM, flags the frame flags the blocks were coded with, dec_lines [n_cf, 1024] the decoders' `lines`
        (before / 2^overall), overall_scale int32 [n_cf, 8]; status (optional, int32 [n_cf]): frames without a defined
        payload get NaN.  -> dict of float64 [n_cf, band_stride]: noise (N_b), mask (M_b), nmr_db; unused slots NaN."""
        n_cf = view.n_cf
        fl = self.flags_tensor(flags, view.n_frames)
        dec_lines = dec_lines.contiguous().view(n_cf, N_LONG)
        overall_scale = overall_scale.contiguous().view(n_cf, _lib.SUB)
        assert dec_lines.dtype == torch.float64 and overall_scale.dtype == torch.int32
        if status is not None:
            status = status.contiguous()
            assert status.dtype == torch.int32 and status.numel() == n_cf
        out = {k: self._empty((n_cf, self.band_stride), torch.float64) for k in ("noise", "mask", "nmr_db")}
        self._call("pacx_nmr_batch", ctypes.byref(view.c), _ptr(fl), _ptr(dec_lines), _ptr(overall_scale), _ptr(status),
                   _ptr(out["noise"]), _ptr(out["mask"]), _ptr(out["nmr_db"]), self._stream())
        return out

    def nmr_summary(self, nmr_db, n_channels, flags=None, summary=None):
        """Adds the values of nmr_db [n_cf, band_stride] to `summary` (pacx_nmr_summary: int64 device tensor
        [2, 32, NMR_SUMMARY_WORDS] holding the library's uint64 words -- long blocks / short sub-blocks, per band
        index: count, count above 0 dB, maximum as an ordered key, 0.5 dB histogram); None: a zeroed one.  Chunks
        of a stream accumulate in one summary.  quality.Summary reads it."""
        nmr_db = nmr_db.contiguous()
        n_cf = nmr_db.shape[0]
        fl = self.flags_tensor(flags, n_cf // n_channels)
        if summary is None:
            summary = torch.zeros((2, _lib.NMR_MAX_BANDS, _lib.NMR_SUMMARY_WORDS), dtype=torch.int64, device=self.device)
        self._call("pacx_nmr_summary", ctypes.c_int64(n_cf), int(n_channels), _ptr(fl), _ptr(nmr_db), _ptr(summary),
                   self._stream())
        return summary

    # ------------------------------------------- function-level entry points
    def window(self, kind, x):
        """window * x for rows of x ([n, 2048] or [n, 256] float64 on the GPU)."""
        x = x.contiguous()
        y = torch.empty_like(x)
        self._call("pacx_window_batch", int(kind), ctypes.c_int64(x.shape[0]), _ptr(x), _ptr(y),
                   self._stream())
        return y

    def window_table(self, table, x):
        """table * x for rows of x ([n, len] float64 on the GPU) with a caller-evaluated
        table (host array or device tensor of len entries)."""
        x = x.contiguous()
        t = torch.as_tensor(np.ascontiguousarray(table, dtype=np.float64), device=self.device) \
            if not isinstance(table, torch.Tensor) else table.contiguous()
        assert t.numel() == x.shape[-1]
        y = torch.empty_like(x)
        self._call("pacx_window_table_batch", _ptr(t), int(t.numel()), ctypes.c_int64(x.numel() // t.numel()),
                   _ptr(x), _ptr(y), self._stream())
        return y

    def tables_exact(self):
        return bool(self.lib.pacx_tables_exact(self.h))

    def _elem(self, name, x, *ints):
        x = x.contiguous()
        out = self._empty(x.shape, torch.int64)
        self._call(name, ctypes.c_int64(x.numel()), _ptr(x), *[int(i) for i in ints], _ptr(out),
                   self._stream())
        return out

    def quantize_uniform(self, x, n_bits):
        return self._elem("pacx_quantize_uniform", x, n_bits)

    def scale_factor(self, x, n_scale_bits, n_mant_bits):
        return self._elem("pacx_scale_factor", x, n_scale_bits, n_mant_bits)

    def mantissa(self, x, scale, n_scale_bits, n_mant_bits):
        return self._elem("pacx_mantissa", x, scale, n_scale_bits, n_mant_bits)

    def mantissa_fp(self, x, scale, n_scale_bits, n_mant_bits):
        return self._elem("pacx_mantissa_fp", x, scale, n_scale_bits, n_mant_bits)

    def _delem(self, name, codes, *ints):
        codes = codes.contiguous()
        assert codes.dtype == torch.int64
        out = self._empty(codes.shape, torch.float64)
        self._call(name, ctypes.c_int64(codes.numel()), _ptr(codes), *[int(i) for i in ints], _ptr(out),
                   self._stream())
        return out

    def dequantize_uniform(self, codes, n_bits):
        """vDequantizeUniform (coder/quantize.py:82-95) of int64 codes on the device"""
        return self._delem("pacx_dequantize_uniform", codes, n_bits)

    def dequantize(self, mant, scale, n_scale_bits, n_mant_bits):
        """vDequantize (coder/quantize.py:254-274)"""
        return self._delem("pacx_dequantize", mant, scale, n_scale_bits, n_mant_bits)

    def dequantize_fp(self, mant, scale, n_scale_bits, n_mant_bits):
        return self._delem("pacx_dequantize_fp", mant, scale, n_scale_bits, n_mant_bits)

    def imdct(self, lines, short=False):
        """mdct.IMDCT for rows of 1024 lines (short: rows of 8 x 128) -> [n, 2048] samples, unwindowed
        (k_imdct_long / k_imdct_short of the decode path)."""
        lines = lines.contiguous().view(-1, N_LONG)
        out = self._empty((lines.shape[0], 2 * N_LONG), torch.float64)
        self._call("pacx_imdct_batch", ctypes.c_int64(lines.shape[0]), _lib.MDCT_SHORT if short else 0, _ptr(lines),
                   _ptr(out), self._stream())
        return out

    def mdct_direct(self, x, a, b, inverse=False):
        """MDCT / IMDCT by the defining sums for any a + b (rows of x): coder/mdct.py:14-77"""
        n_in = (a + b) // 2 if inverse else a + b
        n_out = a + b if inverse else (a + b) // 2
        x = x.contiguous().view(-1, n_in)
        out = self._empty((x.shape[0], n_out), torch.float64)
        self._call("pacx_mdct_direct_batch", ctypes.c_int64(x.shape[0]), int(a), int(b), int(bool(inverse)), _ptr(x),
                   _ptr(out), self._stream())
        return out

    def transient_detect(self, blocks, thresh=4.5):
        """parTransientDetect (coder/detect_transients.py:5-23, axis=1) of float64 blocks [n, nCh, len] on the
        device: uint8 [n], 2 = the mean is exactly zero (the reference returns 0), 1 / 0 = transient or not."""
        blocks = blocks.contiguous()
        n, n_ch, ln = blocks.shape
        out = self._empty((n,), torch.uint8)
        self._call("pacx_transient_detect_f64", ctypes.c_int64(n), int(n_ch), int(ln), _ptr(blocks),
                   ctypes.c_double(float(thresh)), _ptr(out), self._stream())
        return out

    def bit_alloc_generic(self, budget, max_mant_bits, n_lines, smr):
        """BitAlloc for rows of smr [n, nBands] with per-row budgets [n]."""
        smr = smr.contiguous()
        n, nb = smr.shape
        nl = torch.as_tensor(np.asarray(n_lines, dtype=np.int32), device=self.device)
        bits = self._empty((n, nb), torch.int32)
        self._call("pacx_bitalloc_generic", ctypes.c_int64(n), int(nb), _ptr(nl), _ptr(budget.contiguous()),
                   int(max_mant_bits), _ptr(smr), _ptr(bits), self._stream())
        return bits


class EncoderPool:
    """Several steps in flight: N handles (each with its own workspaces) on N HIP streams, for callers with many
    INDEPENDENT batches.  A handle serialises its calls -- its workspaces are shared between them -- and every kernel of
    the path leaves a third to a half of the vector issue slots idle, bound by latency chains at the occupancy its
    registers and LDS allow; kernels of another batch fill those slots (two batches side by side: +15-28 % on one
    MI355X; more than two add nothing).  What `bench.py` times by default.

        pool = EncoderPool(2, 48000, 128 / 48.0)
        for i, batch in enumerate(batches):
            k = pool.next()                       # round robin; waits (on the device) for what last ran in slot k
            with pool.slot(k) as enc:             # enc: that slot's Encoder; the body is queued on the slot's stream
                enc.encode_pack(batch.view, None, outs[k])
        pool.synchronize()

    The caller keeps one set of output buffers per slot and must not read slot k's outputs before pool.wait(k) (or
    synchronize()).  The reference runs its own workers side by side too (Pool(8), coder/pacfile.py:771-781)."""

    def __init__(self, n, *args, **kwargs):
        self.encs = [Encoder(*args, **kwargs) for _ in range(max(1, int(n)))]
        dev = self.encs[0].device
        self.streams = [torch.cuda.Stream(device=dev) for _ in self.encs]
        self.done = [torch.cuda.Event() for _ in self.encs]
        self._turn = 0
        self._gate = self._gate_stream = None
        self._used = [False] * len(self.encs)
        if len(self.encs) > 1:                       # two handles: their two streams each share a hardware queue, the fork pays
            for e in self.encs:
                e.set_side_fork(True)

    def __len__(self):
        return len(self.encs)

    def next(self):
        k = self._turn
        self._turn = (k + 1) % len(self.encs)
        return k

    def slot(self, k):
        pool = self

        class _Slot:
            def __enter__(self_inner):
                self_inner.ctx = torch.cuda.stream(pool.streams[k])
                self_inner.ctx.__enter__()
                return pool.encs[k]

            def __exit__(self_inner, *exc):
                pool.done[k].record(pool.streams[k])
                pool._used[k] = True
                return self_inner.ctx.__exit__(*exc)
        return _Slot()

    def align(self, delay_us=None):
        """Start the next calls of all slots at the same instant.  From an idle device the slots' first steps start as
        far apart as the host takes to queue one (tens of microseconds), and two free-running pipelines then settle
        into one of two stable relations -- in phase (like kernels side by side: 51.4 M cf/s on the headline batch)
        or in anti-phase (47.0 M), DESIGN.md 5.0.  A gate event behind a short spin on a third stream holds every
        slot's stream until all the first calls are queued; started together they stay in phase for a hundred steps or
        so (bench.py: 51.9 M cf/s over 100-step regions, 47.9 M over 200-step ones -- the pipelines drift into the other
        relation; calling this again mid-stream, where it is a barrier between the slots followed by the common start,
        did not bring the faster relation back in the measurements of round 3).  Costs delay_us (default
        PACX_POOL_GATE_US or 100) per call."""
        if len(self.encs) < 2:
            return
        if delay_us is None:
            delay_us = float(os.environ.get("PACX_POOL_GATE_US", "100"))
        if delay_us <= 0 or not hasattr(torch.cuda, "_sleep"):
            return
        dev = self.encs[0].device
        if self._gate is None:
            self._gate_stream = torch.cuda.Stream(device=dev)
            self._gate = torch.cuda.Event()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(self._gate_stream):          # calibrate the spin: cycles per microsecond
                torch.cuda._sleep(100_000)
                t0.record()
                torch.cuda._sleep(2_000_000)
                t1.record()
            t1.synchronize()
            self._cycles_per_us = 2_000_000 / max(t0.elapsed_time(t1) * 1e3, 1.0)
        with torch.cuda.stream(self._gate_stream):
            for k in range(len(self.encs)):             # mid-stream: a barrier between the slots (what they have queued
                if self._used[k]:                       # so far finishes), then the common start
                    self._gate_stream.wait_event(self.done[k])
            torch.cuda._sleep(int(delay_us * self._cycles_per_us))
            self._gate.record(self._gate_stream)
        for s in self.streams:
            s.wait_event(self._gate)

    def wait(self, k, stream=None):
        """make `stream` (default: the current one) wait for what was last queued in slot k"""
        (stream or torch.cuda.current_stream(self.encs[0].device)).wait_event(self.done[k])

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def close(self):
        for e in self.encs:
            e.close()
