"""PCM view layouts for the generic (strided / unaligned / float64) front end (test helper, no GPU).

make() lays the F frames of a stream view out in another way and poisons every element the view does not address: a
kernel that reads a wrong address inside the buffer reads +-32767 or NaN, never the neighbouring sample.  Every
layout is sized so that the right addressing stays inside the buffer; so do addressings with a smaller sample stride
or without the channel term (they only reach lower addresses)."""
import numpy as np

from oracle import pac_oracle as po

KINDS = ("planar", "interleaved", "shifted", "odd_rows", "odd_frames", "every_third", "broadcast",
         "f64_planar", "f64_interleaved", "f64_frames")
GENERIC_I16 = ("interleaved", "shifted", "odd_rows", "odd_frames", "every_third")
GENERIC_F64 = ("f64_planar", "f64_interleaved", "f64_frames")
GENERIC = GENERIC_I16 + GENERIC_F64
NO_POISON = ("planar", "f64_frames", "broadcast")


def poison(n, dtype):
    if dtype == np.float64:
        return np.full(n, np.nan)
    p = np.full(n, 32767, np.int16)              # not -32768: the codec reads that code as 0
    p[1::2] = -32767
    return p


def fast(dtype, offset, fs, cs, ss):
    """check_pcm's choice (csrc/pacx_api.hip) for a buffer whose first element is 16-byte aligned"""
    return dtype == np.int16 and ss == 1 and (2 * offset) % 16 == 0 and fs % 8 == 0 and cs % 8 == 0


def frames_of(planar, hop=1024):
    """[F, n_ch, 2 * hop]: frame f spans hops f, f + 1"""
    n_ch, n = planar.shape
    return np.stack([planar[:, f * hop:(f + 2) * hop] for f in range(n // hop - 1)])


def make(planar, kind, hop=1024):
    """-> (host_buffer, dtype, n_ch, F, frame_stride, channel_stride, sample_stride, element_offset)"""
    planar = np.ascontiguousarray(planar)
    assert planar.dtype == np.int16 and planar.ndim == 2
    n_ch, n = planar.shape
    assert n % hop == 0 and n >= 2 * hop
    F, N = n // hop - 1, 2 * hop
    dtype = np.float64 if kind.startswith("f64") else np.int16
    # the code -32768 becomes -0.0 in the oracle's conversion and in the kernels' (pacx_pcm16_to_f64) alike
    src = po.pcm16_to_fraction(planar) if dtype == np.float64 else planar
    src = np.ascontiguousarray(src, dtype=dtype)
    pre = 16 // np.dtype(dtype).itemsize          # a poisoned prefix of 16 bytes keeps the view's alignment
    if kind == "planar":
        buf, fs, cs, ss, off = src.ravel().copy(), hop, n, 1, 0
    elif kind in ("interleaved", "f64_interleaved"):
        buf, fs, cs, ss, off = np.concatenate((poison(pre, dtype), src.T.ravel())), hop * n_ch, 1, n_ch, pre
    elif kind == "shifted":
        buf, fs, cs, ss, off = np.concatenate((poison(1, dtype), src.ravel(), poison(7, dtype))), hop, n, 1, 1
    elif kind == "odd_rows":
        rows = poison(n_ch * (n + 3), dtype).reshape(n_ch, n + 3)
        rows[:, :n] = src
        buf, fs, cs, ss, off = rows.ravel(), hop, n + 3, 1, 0
    elif kind == "odd_frames":
        fr = poison(n_ch * F * (N + 4), dtype).reshape(n_ch, F, N + 4)
        fr[:, :, :N] = frames_of(src, hop).transpose(1, 0, 2)
        buf, fs, cs, ss, off = fr.ravel(), N + 4, F * (N + 4), 1, 0
    elif kind == "every_third":
        wide = poison(n_ch * n * 3, dtype).reshape(n_ch, n * 3)
        wide[:, ::3] = src
        buf, fs, cs, ss, off = wide.ravel(), 3 * hop, 3 * n, 3, 0
    elif kind == "broadcast":
        buf, fs, cs, ss, off = src[0].copy(), hop, 0, 1, 0
    elif kind == "f64_planar":
        buf, fs, cs, ss, off = np.concatenate((poison(pre, dtype), src.ravel())), hop, n, 1, pre
    elif kind == "f64_frames":
        buf, fs, cs, ss, off = frames_of(src, hop).ravel().copy(), n_ch * N, N, 1, 0
    else:
        raise ValueError(kind)
    assert buf.dtype == dtype and buf.ndim == 1
    assert off + last_index(n_ch, F, fs, cs, ss, hop) < len(buf)
    assert fast(dtype, off, fs, cs, ss) == (kind in ("planar", "broadcast")), kind
    return buf, dtype, n_ch, F, fs, cs, ss, off


def last_index(n_ch, F, fs, cs, ss, hop=1024):
    return (F - 1) * fs + (n_ch - 1) * cs + (2 * hop - 1) * ss


def addresses(n_ch, F, fs, cs, ss, off, hop=1024):
    """[F, n_ch, 2 * hop] element index of every sample the view addresses"""
    f, c, s = np.meshgrid(np.arange(F), np.arange(n_ch), np.arange(2 * hop), indexing="ij")
    return off + f * fs + c * cs + s * ss


def expected(planar, kind, hop=1024):
    """[F, n_ch, 2 * hop] what the view of this kind presents: the planar samples (broadcast: channel 0 throughout)"""
    fr = frames_of(np.ascontiguousarray(planar), hop)
    if kind == "broadcast":
        fr = np.repeat(fr[:, :1], fr.shape[1], axis=1)
    return po.pcm16_to_fraction(fr) if kind.startswith("f64") else fr


def view(A, enc, torch, planar, kind, hop=1024):
    """the layout on the device as an engine.PcmView: a slice of the uploaded buffer, so that data_ptr() carries the
    offset and the view's tensor keeps the whole storage alive"""
    buf, dtype, n_ch, F, fs, cs, ss, off = make(planar, kind, hop)
    whole = torch.as_tensor(buf, device=enc.device)
    v = A.engine.PcmView(whole[off:], n_ch, F, fs, cs, ss)
    assert whole.data_ptr() % 16 == 0
    assert bool(fast(dtype, off, fs, cs, ss)) == (kind in ("planar", "broadcast"))
    return v
