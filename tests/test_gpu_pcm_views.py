"""Strided, unaligned and float64 PCM views through every batched entry point.

check_pcm (csrc/pacx_api.hip) sends a view to the fast kernels only when it is int16 with unit sample stride, a
16-byte-aligned base and frame / channel strides that are multiples of 8; everything else runs the generic kernels
(k_mdct_long / k_mdct_short / k_side_* <DT, false>, the strided branch of k_transient) and the `if (!fast)` branches of
the entry points.  tests/pcm_layouts.py presents the same frames in ten layouts, poison between the samples.

Rules.
  Exact equality only between calls that run the same arithmetic: the int16 generic kinds among themselves, the
  float64 kinds among themselves, int16 against float64 for the MDCT (float64 holds the very doubles the int16 kernels
  convert to; the side chain windows int16 codes with a table of its own, so its results are compared within DB_TOL),
  and against the fast planar view where the kernel template is the same (short blocks, the side chain's peak counts,
  prewindowed long blocks, the integer transient detector).
  Where the arithmetic differs (the long-block FFT factorisations) each side is held to the oracle, with the bars the
  suite already has: MDCT_TOL of tests/test_gpu_parity.py for lines, equality for integer codes and bytes, WORST_TOL /
  NMR_TOL / DB_TOL / WINDOW of test_gpu_abr / band / nmr / rate for curves, NMR and the search.
"""
import ctypes
import functools

import numpy as np
import pytest

import nmr_model as nm
import pcm_layouts as pl
import rate_model as rm
import test_gpu_abr as ta
import test_gpu_band as tb
import test_gpu_nmr as tn
import test_gpu_rate as tr
from oracle import pac_oracle as po
from test_gpu_parity import DB_TOL, MDCT_TOL

pytestmark = pytest.mark.gpu

HOP = 1024
MATERIALS = ("windows", "three_channels_odd", "mono_odd", "silence_and_drop")
I16_KIND, F64_KIND = "every_third", "f64_interleaved"      # the pair held to the oracle; C1 ties the others to them


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    return a


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


# ------------------------------------------------------------------------------------------------------ material
def silence_and_drop_with_full_scale():
    """test_gpu_abr.silence_and_drop with the code -32768 (which the codec reads as 0) at positions 0, 511, 512 and 1023
    of hop 5, an ordinary hop, in every channel: the pairs the long MDCT's fold adds up"""
    pcm, sr = ta.silence_and_drop()
    pcm = pcm.copy()
    pcm[5 * HOP + np.array([0, 511, 512, 1023])] = -32768
    return pcm, sr


def silence_and_drop_three_channels():
    """7 hops, 3 channels -> 27 channel-frames: digital silence, a dropped short-coded hop, ordinary hops"""
    rng = np.random.default_rng(15)
    pcm = np.zeros((7 * HOP, 3), np.int16)
    pcm[HOP:2 * HOP] = rng.integers(-3000, 3000, (HOP, 3))
    pcm[3 * HOP + 900:4 * HOP] = rng.integers(-30000, 30000, (124, 3))
    pcm[4 * HOP:] = rng.integers(-3000, 3000, (3 * HOP, 3))
    pcm[6 * HOP + 300:6 * HOP + 306] = 30000            # a second attack: short-coded hops that are written
    return pcm, 48000


MAKE = {"windows": ta.windows, "three_channels_odd": ta.three_channels,
        "mono_odd": ta.SHAPES["mono_odd"][0], "silence_and_drop": silence_and_drop_with_full_scale,
        "silence_and_drop_3ch": silence_and_drop_three_channels}


def stream_planar(pcm):
    """pacfile.device_stream's layout on the host: zeros, the hops, the last hop again, zeros"""
    n, n_ch = pcm.shape
    buf = np.zeros((n_ch, n + 3 * HOP), np.int16)
    buf[:, HOP:HOP + n] = pcm.T
    buf[:, HOP + n:2 * HOP + n] = pcm[n - HOP:].T
    return buf


@functools.lru_cache(maxsize=None)
def material(name):
    """-> dict pcm, sr, planar, n_ch, F, and the oracle's run of the stream at 128 kb/s with block switching: flags
    [(last, cur, next)] per block, parts [block] = per channel the list of (sf, alloc, mant, overall) or None for a
    dropped hop, records [block][ch] = payload bytes, data = the .pac bytes"""
    pcm, sr = MAKE[name]()
    pcm = np.ascontiguousarray(pcm)
    col = []
    data = po.encode_stream(pcm, sr, 128, True, collect=col)
    p = po.make_params(sr, pcm.shape[1], 128)
    flags = [tuple(bool(x) for x in f) for f, _ in col]
    parts = [q for _, q in col]
    records = [None if q is None else [po.pack_channel_block(p, f, q[ch])[1] for ch in range(pcm.shape[1])]
               for f, q in zip(flags, parts)]
    planar = stream_planar(pcm)
    m = {"pcm": pcm, "sr": sr, "planar": planar, "n_ch": pcm.shape[1], "F": len(flags), "flags": flags, "parts": parts,
         "records": records, "data": data, "p": p,
         "packed": np.array([l * 1 + c * 2 + n * 4 for (l, c, n) in flags], np.uint8)}
    assert m["F"] == planar.shape[1] // HOP - 1 == len(pcm) // HOP + 2
    return m


def test_materials_are_what_they_claim():
    kinds = {f for f in material("windows")["flags"]}
    assert {(False, False, True), (True, False, False), (True, False, True), (False, True, False)} <= kinds
    assert sum(f[1] for f in material("windows")["flags"]) == 2
    m = material("three_channels_odd")
    assert m["n_ch"] == 3 and (m["n_ch"] * m["F"]) % 2 == 1 and any(f[1] for f in m["flags"])
    assert material("mono_odd")["n_ch"] == 1 and material("mono_odd")["F"] % 2 == 1
    m = material("silence_and_drop")
    assert any(q is None for q in m["parts"]) and (m["pcm"] == -32768).sum() == 8
    assert not m["flags"][5][1] and not m["flags"][6][1]              # hop 5 lies in two long blocks
    m = material("silence_and_drop_3ch")
    assert m["n_ch"] * m["F"] == 27 and any(q is None for q in m["parts"])
    assert any(f[1] and q is not None for f, q in zip(m["flags"], m["parts"]))
    for name in MAKE:
        assert material(name)["F"] * material(name)["n_ch"] <= 27


_DEV = {}


def on_gpu(A, torch, name, kind, enc=None):
    """the material's view of this kind on the device (cached per encoder device), and its flags tensor"""
    m = material(name)
    enc = enc or scalar_enc(A, m)
    key = (name, kind)
    if key not in _DEV:
        _DEV[key] = pl.view(A, enc, torch, m["planar"], kind)
    if ("flags", name) not in _DEV:
        _DEV[("flags", name)] = torch.as_tensor(m["packed"], device=enc.device)
    return _DEV[key], _DEV[("flags", name)]


def scalar_enc(A, m):
    return A.context.encoder(m["sr"], 128 / (m["sr"] / 1000))


def vq_enc(A, m, kbps):
    return A.context.encoder(m["sr"], kbps / (m["sr"] / 1000), use_vq=True, use_sbr=kbps < 128)


def bits(t):
    """a device tensor as integers: float64 compared bit for bit"""
    a = t.cpu().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else a


# ------------------------------------------------------------------------------- what of an output is defined
def line_mask(enc, alloc, short):
    """[n_cf, 1024] bool: lines of bands with a non-zero allocation (alloc [n_cf, band_stride], short [n_cf] bool)"""
    n_cf = alloc.shape[0]
    mask = np.zeros((n_cf, HOP), bool)
    bl, bs = enc.sfBands, enc.sfBandsShort
    for i in range(n_cf):
        if not short[i]:
            for b in range(bl.nBands):
                if alloc[i, b]:
                    mask[i, bl.lowerLine[b]:bl.upperLine[b] + 1] = True
        else:
            for sb in range(8):
                for b in range(bs.nBands):
                    if alloc[i, sb * bs.nBands + b]:
                        mask[i, sb * 128 + bs.lowerLine[b]:sb * 128 + bs.upperLine[b] + 1] = True
    return mask


def slot_mask(enc, short):
    """[n_cf, band_stride] bool: band slots in use"""
    mask = np.zeros((len(short), enc.band_stride), bool)
    mask[~short, :enc.sfBands.nBands] = True
    mask[short, :8 * enc.sfBandsShort.nBands] = True
    return mask


def defined(enc, out, flags, n_ch):
    """the defined part of an encode's outputs as a dict of host arrays: payload up to n_bytes, overall[:, 0] of long
    and all eight of short channel-frames, band slots in use, mantissas of coded bands; of a dropped hop (or a frame
    the reference cannot code) only status, n_bytes and the overall scales"""
    host = {k: v.cpu().numpy() for k, v in out.items() if v is not None and hasattr(v, "cpu") and k != "flags"}
    n_cf = host["status"].shape[0]
    fl = np.zeros(n_cf // n_ch, np.uint8) if flags is None else flags.cpu().numpy()
    short = np.repeat((fl & 2) != 0, n_ch)
    status = host["status"].astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal((status & 1) != 0, short)
    gone = (status & (2 | 64)) != 0
    res = {"status": status}
    ov = host["overall"].copy()
    ov[~short, 1:] = 0
    res["overall"] = ov
    slots = slot_mask(enc, short) & ~gone[:, None]
    for k in ("bit_alloc", "scale_factor", "budget"):
        if k in host:
            a = host[k].copy()
            if k == "budget":
                a[~short, 1:] = 0
                a[gone] = 0
            else:
                a[~slots] = 0
            res[k] = a
    if "mantissa" in host and "scale_factor" in host:
        mant = host["mantissa"].copy()
        mant[~(line_mask(enc, res["bit_alloc"], short) & ~gone[:, None])] = 0
        res["mantissa"] = mant
    if "n_bytes" in host:
        nb = host["n_bytes"].copy()
        assert (nb[gone] == 0).all() and (nb >= 0).all() and (nb <= host["payload"].shape[1]).all()
        pay = host["payload"].copy()
        pay[np.arange(pay.shape[1])[None, :] >= nb[:, None]] = 0
        res["n_bytes"], res["payload"] = nb, pay
    return res


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (what, k, int(np.sum(x != y)))


def decoder_lines(enc, out, n_ch):
    """the decoders' lines of an encode_pack's payloads, as quality._Accumulator feeds pacx_nmr_batch"""
    codes = enc.unpack(out["payload"], out["n_bytes"])
    extra = {}
    enc.decode(codes, n_ch, want_pcm=False, extra=extra)
    return extra["lines"], codes["overall"], codes["status"] | extra["status"]


# ---------------------------------------------------------------------------------------------------- C1
def everything(A, torch, name, kind, given):
    """every entry point on one view of the material -> {what: host array or dict of them}.  given: what the planar
    run hands to the entry points that take an encode's results (decoder lines, budgets, an allocation)"""
    m = material(name)
    enc = scalar_enc(A, m)
    view, flags = on_gpu(A, torch, name, kind)
    n_ch, cap = m["n_ch"], 320 / (m["sr"] / 1000)
    r = {}
    for what, kw in (("mdct", {}), ("mdct flags", {"flags": flags}), ("mdct short", {"short": True}),
                     ("mdct kbd", {"kbd": True}), ("mdct prewindowed", {"prewindowed": True}),
                     ("mdct short kbd", {"short": True, "kbd": True})):
        lines, scale = enc.mdct(view, want_scale=True, **kw)
        r[what], r[what + " scale"] = bits(lines), bits(scale)
    for short in (False, True):
        lines = enc.mdct(view, short=short)
        smr, thr, npk = enc.smr(view, lines, short=short, want_threshold=True, want_peaks=True)
        r[f"smr {short}"], r[f"thr {short}"], r[f"peaks {short}"] = bits(smr), bits(thr), bits(npk)
    r["encode"] = defined(enc, enc.encode(view), None, n_ch)
    r["encode flags"] = defined(enc, enc.encode(view, flags), flags, n_ch)
    r["encode_pack"] = defined(enc, enc.encode_pack(view, flags, want_mantissa=True), flags, n_ch)
    r["encode_pack no flags"] = defined(enc, enc.encode_pack(view, None, want_mantissa=True), None, n_ch)
    for kbps in (128, 96):
        r[f"encode_vq {kbps}"] = defined(vq_enc(A, m, kbps), vq_enc(A, m, kbps).encode_vq(view, flags), flags, n_ch)
    got = enc.nmr(view, flags, given["lines"], given["overall"], given["status"])
    for k in ("noise", "mask", "nmr_db"):
        r["nmr " + k] = bits(got[k])
    r["encode_pack_nmr"] = defined(enc, enc.encode_pack_nmr(view, flags, -3.0, cap, want_mantissa=True), flags, n_ch)
    r["encode_pack_budget"] = defined(enc, enc.encode_pack_budget(view, flags, given["budget"], want_mantissa=True),
                                      flags, n_ch)
    r["encode_pack_alloc"] = defined(enc, enc.encode_pack_alloc(view, flags, given["alloc"], want_mantissa=True),
                                     flags, n_ch)
    c = enc.rate_curve(view, flags, cap)
    for k in ("worst", "bits", "steps"):
        r["rate_curve " + k] = bits(c[k])
    c = enc.band_curve(view, flags, cap)
    for k in ("nmr", "cap", "cap_alloc"):
        r["band_curve " + k] = bits(c[k])
    torch.cuda.synchronize()
    return r


def given_by_planar(A, torch, name):
    key = ("given", name)
    if key not in _DEV:
        m = material(name)
        enc = scalar_enc(A, m)
        view, flags = on_gpu(A, torch, name, "planar")
        packed = enc.encode_pack(view, flags)
        lines, overall, status = decoder_lines(enc, packed, m["n_ch"])
        searched = enc.encode_pack_nmr(view, flags, -3.0, 320 / (m["sr"] / 1000))
        status = (packed["status"] | status) & A.quality._NO_PAYLOAD               # as quality._Accumulator.chunk
        status = torch.where(packed["n_bytes"] > 0, status, torch.full_like(status, A._lib.ST_ZERO_SUBBLOCK))
        _DEV[key] = {"lines": lines, "overall": overall, "status": status, "budget": searched["budget"].clone(),
                     "alloc": searched["bit_alloc"].clone()}
    return _DEV[key]


def assert_same_run(a, b, what, only=None):
    for k in a:
        if only is not None and not only(k):
            continue
        if isinstance(a[k], dict):
            same(a[k], b[k], f"{what}: {k}")
        else:
            assert np.array_equal(a[k], b[k]), (what, k, int(np.sum(a[k] != b[k])))


@pytest.mark.parametrize("name", MATERIALS)
def test_generic_kinds_agree_bit_for_bit(A, torch, name):
    """C1: the int16 layouts interleaved, shifted, odd_rows, odd_frames and every_third run the same kernels on the
    same samples, and so do the three float64 layouts: within each group every defined output of every entry point is
    identical.  Between the groups the MDCT is the same arithmetic too (the float64 views hold the very doubles the
    int16 kernels convert to), but the side chain is not: for int16 it multiplies the integer code by a Hann table that
    carries the 2 / 65535 (hann_sample, csrc/k_psy.hip), for float64 the plain table by the fraction, so SMRs and
    thresholds differ in their last bits (each is within DB_TOL of the oracle, tests/test_gpu_parity.py, hence within
    twice that of the other).  Asserted between the groups: lines and overall scales bit for bit, SMRs and thresholds
    within 2 DB_TOL, the integer codes and bytes that test_scalar_codes_and_bytes_against_the_oracle and
    test_gain_shape_bytes_against_the_oracle tie to the oracle on both sides, and encode_pack_alloc, which reads no SMR.
    Against the fast planar view: the short blocks (lines, scales, codes, status), the side chain's peak counts and
    prewindowed long lines."""
    m = material(name)
    given = given_by_planar(A, torch, name)
    runs = {kind: everything(A, torch, name, kind, given) for kind in pl.GENERIC}
    first, first_f64 = runs[pl.GENERIC_I16[0]], runs[pl.GENERIC_F64[0]]
    for kind in pl.GENERIC_I16[1:]:
        assert_same_run(first, runs[kind], f"{name}: {pl.GENERIC_I16[0]} / {kind}")
    for kind in pl.GENERIC_F64[1:]:
        assert_same_run(first_f64, runs[kind], f"{name}: {pl.GENERIC_F64[0]} / {kind}")
    assert_same_run(first, first_f64, f"{name}: int16 / float64",
                    only=lambda k: k.startswith(("mdct", "encode_vq")) or k in ("encode", "encode flags", "encode_pack",
                                                                                "encode_pack no flags", "encode_pack_alloc"))
    for k in ("smr False", "smr True", "thr False", "thr True"):
        x, y = first[k].view(np.float64), first_f64[k].view(np.float64)
        fin = np.isfinite(x)
        assert np.array_equal(fin, np.isfinite(y)) and np.array_equal(x[~fin], y[~fin], equal_nan=True), (name, k)
        err = float(np.max(np.abs(x[fin] - y[fin]))) if fin.any() else 0.0
        print(f"{name}: {k}: int16 and float64 side chains differ by at most {err:.3g} dB")
        assert err <= 2 * DB_TOL, (name, k, err)
    fast = everything(A, torch, name, "planar", given)
    assert_same_run(fast, first, f"{name}: planar / generic",
                    only=lambda k: k in ("mdct short", "mdct short scale", "mdct short kbd", "mdct short kbd scale",
                                         "mdct prewindowed", "mdct prewindowed scale", "peaks False", "peaks True"))
    # short-coded channel-frames of the mixed batches: codes, status and bytes
    short = np.repeat([f[1] for f in m["flags"]], m["n_ch"])
    assert short.any()
    for what in ("encode flags", "encode_pack", "encode_vq 128", "encode_vq 96", "encode_pack_nmr", "encode_pack_budget",
                 "encode_pack_alloc"):
        for k in fast[what]:
            assert np.array_equal(fast[what][k][short], first[what][k][short]), (name, what, k)
    # the flags the batches were coded with are the detector's
    enc = scalar_enc(A, m)
    planar = torch.as_tensor(m["planar"], device=enc.device)
    tr_, fl = enc.transient_flags(planar, len(m["pcm"]) // HOP)
    assert np.array_equal(fl.cpu().numpy(), m["packed"])


def test_broadcast_is_channel_zero_twice(A, torch):
    """channel_stride = 0: both channels of the stereo view are the mono result of channel 0"""
    m = material("windows")
    enc = scalar_enc(A, m)
    both, flags = on_gpu(A, torch, "windows", "broadcast")
    assert both.c.channel_stride == 0 and both.n_channels == 2
    mono = pl.view(A, enc, torch, m["planar"][:1], "planar")
    for call in (lambda v, n: defined(enc, enc.encode(v, flags), flags, n),
                 lambda v, n: defined(enc, enc.encode_pack(v, flags, want_mantissa=True), flags, n),
                 lambda v, n: {"lines": enc.mdct(v, flags).cpu().numpy(), "short": enc.mdct(v, short=True).cpu().numpy()}):
        two, one = call(both, 2), call(mono, 1)
        for ch in range(2):
            same({k: v[ch::2] for k, v in two.items()}, one, f"broadcast channel {ch}")


# ------------------------------------------------------------------------------------- transient detector
def hop_view(A, torch, enc, planar, kind):
    """the hops of a layout as pacx_transient_flags takes them (Encoder.transient_flags builds the planar one)"""
    buf, dtype, n_ch, F, fs, cs, ss, off = pl.make(planar, kind)
    whole = torch.as_tensor(buf, device=enc.device)
    dt = A._lib.PCM_F64 if dtype == np.float64 else A._lib.PCM_I16
    start = off + HOP * ss                                   # hop h is the second half of frame h
    assert start + (F - 3) * fs + (n_ch - 1) * cs + (HOP - 1) * ss < len(buf)
    return whole, A._lib.PacxPcm(whole.data_ptr() + start * whole.element_size(), dt, n_ch, F - 2, fs, cs, ss)


@pytest.mark.parametrize("name", ["mono_odd", "windows", "three_channels_odd"])
def test_transient_flags_of_every_int16_layout(A, torch, name):
    """integer arithmetic: the strided branch of k_transient gives the planar view's bytes for 1, 2 and 3 channels"""
    m = material(name)
    enc = scalar_enc(A, m)
    n_hops = m["F"] - 2
    planar = torch.as_tensor(m["planar"], device=enc.device)
    want_tr, want_fl = (t.cpu().numpy() for t in enc.transient_flags(planar, n_hops))
    assert np.array_equal(want_fl, m["packed"]) and want_tr.any()
    for kind in pl.GENERIC_I16:
        keep, hops = hop_view(A, torch, enc, m["planar"], kind)
        tr_ = torch.full((n_hops,), 0x5A, dtype=torch.uint8, device=enc.device)
        fl = torch.full((n_hops + 2,), 0x5A, dtype=torch.uint8, device=enc.device)
        enc._call("pacx_transient_flags", ctypes.byref(hops), A.engine._ptr(tr_), A.engine._ptr(fl), enc._stream())
        assert np.array_equal(tr_.cpu().numpy(), want_tr), (name, kind)
        assert np.array_equal(fl.cpu().numpy(), want_fl), (name, kind)


def test_transient_flags_refusals(A, torch):
    m = material("windows")
    enc = scalar_enc(A, m)
    out = torch.zeros(16, dtype=torch.uint8, device=enc.device)
    keep, hops = hop_view(A, torch, enc, m["planar"], "f64_planar")
    assert enc.lib.pacx_transient_flags(enc.h, ctypes.byref(hops), A.engine._ptr(out), A.engine._ptr(out),
                                        None) == A._lib.E_ARG
    nine = np.zeros((9, 4 * HOP), np.int16)
    keep, hops = hop_view(A, torch, enc, nine, "odd_rows")
    assert hops.n_channels == 9 and hops.n_frames == 1
    assert enc.lib.pacx_transient_flags(enc.h, ctypes.byref(hops), A.engine._ptr(out), A.engine._ptr(out),
                                        None) == A._lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any()


# ---------------------------------------------------------------------------------------------------- C2
def oracle_lines(m, kbd=False):
    """long [F, n_ch, 1024] with the window the flags select (kbd: the KBD window whatever the flags), short
    [F, n_ch, 8, 128] sine-windowed sub-blocks (kbd likewise), of every frame"""
    frac = po.pcm16_to_fraction(pl.frames_of(m["planar"]))
    long_ = np.empty((m["F"], m["n_ch"], HOP))
    short = np.empty((m["F"], m["n_ch"], 8, 128))
    for f, (l, c, n) in enumerate(m["flags"]):
        for ch in range(m["n_ch"]):
            x = frac[f, ch]
            w = po.kbd_window(2 * HOP) * x if kbd else po.apply_window(x, l, False, n)
            long_[f, ch] = po.mdct_forward(w, HOP, HOP)[:HOP]
            for j, sub in enumerate(nm.sub_blocks(x)):
                ws = po.kbd_window(256) if kbd else po.sine_window(256)
                short[f, ch, j] = po.mdct_forward(ws * sub, 128, 128)[:128]
    return long_, short


def worst_line_error(got, want):
    """max over blocks of max |got - want| / max |want|; a silent block must be zeros"""
    got, want = got.reshape(-1, want.shape[-1]), want.reshape(-1, want.shape[-1])
    ref = np.max(np.abs(want), axis=1)
    err = np.max(np.abs(got - want), axis=1)
    assert not got[ref == 0].any()
    return float(np.max(err[ref > 0] / ref[ref > 0])) if (ref > 0).any() else 0.0


@pytest.mark.parametrize("name", MATERIALS)
def test_generic_lines_against_the_oracle(A, torch, name):
    """lines of the generic kernels against mdct_forward(window * fraction): sine, start, stop and start-stop long
    windows as the flags select them, KBD, and the short sub-blocks, within MDCT_TOL of the block maximum"""
    m = material(name)
    enc = scalar_enc(A, m)
    want_long, want_short = oracle_lines(m)
    kbd_long, kbd_short = oracle_lines(m, kbd=True)
    cur = np.array([f[1] for f in m["flags"]])
    kinds = {0: "sine", 1: "stop", 4: "start", 5: "start-stop"}
    seen = {}
    for kind in (I16_KIND, F64_KIND):
        view, flags = on_gpu(A, torch, name, kind)
        lines = enc.mdct(view, flags).cpu().numpy().reshape(m["F"], m["n_ch"], HOP)
        for code, label in kinds.items():
            sel = ((m["packed"] & 5) == code) & ~cur
            if sel.any():
                seen[label] = max(seen.get(label, 0.0), worst_line_error(lines[sel], want_long[sel]))
        got = enc.mdct(view, short=True).cpu().numpy().reshape(m["F"], m["n_ch"], 8, 128)
        seen["short"] = max(seen.get("short", 0.0), worst_line_error(got, want_short))
        got = enc.mdct(view, kbd=True).cpu().numpy().reshape(m["F"], m["n_ch"], HOP)
        seen["kbd"] = max(seen.get("kbd", 0.0), worst_line_error(got, kbd_long))
        got = enc.mdct(view, short=True, kbd=True).cpu().numpy().reshape(m["F"], m["n_ch"], 8, 128)
        seen["kbd short"] = max(seen.get("kbd short", 0.0), worst_line_error(got, kbd_short))
    print(f"{name}: largest line error of the generic kernels, of the block maximum: " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(seen.items())))
    if name == "windows":
        assert {"sine", "stop", "start", "start-stop", "short", "kbd"} <= set(seen)
    assert max(seen.values()) <= MDCT_TOL, seen


def check_codes(A, enc, m, out, what):
    """an encode's outputs against the oracle's parts: overall scales, scale factors, allocations, mantissas"""
    host = {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "flags"}
    for f, (flags, parts) in enumerate(zip(m["flags"], m["parts"])):
        for ch in range(m["n_ch"]):
            i = f * m["n_ch"] + ch
            st = int(host["status"][i]) & 0xFFFFFFFF
            assert (st & 1) == int(flags[1]) and bool(st & 2) == (parts is None), (what, f, ch, st)
            if parts is None:
                continue
            for j, (sf, alloc, mant, overall) in enumerate(parts[ch]):
                got = A.codec.unpack_short(enc, host, i, j) if flags[1] else A.codec.unpack_long(enc, host, i)
                assert got[3] == overall, (what, f, ch, j, "overall")
                assert got[1].tolist() == list(alloc), (what, f, ch, j, "alloc")
                assert got[0].tolist() == sf.tolist(), (what, f, ch, j, "scale factors")
                assert got[2].tolist() == mant.tolist(), (what, f, ch, j, "mantissas")


def check_records(m, out, records, what):
    n_bytes, payload = out["n_bytes"].cpu().numpy(), out["payload"].cpu().numpy()
    for f, recs in enumerate(records):
        for ch in range(m["n_ch"]):
            i = f * m["n_ch"] + ch
            if recs is None:
                assert n_bytes[i] == 0, (what, f, ch)
            else:
                assert payload[i, :n_bytes[i]].tobytes() == recs[ch], (what, f, ch)


@pytest.mark.parametrize("name", MATERIALS)
def test_scalar_codes_and_bytes_against_the_oracle(A, torch, name):
    """encode / encode_pack through an int16 and a float64 generic view, and through the fast view, are the oracle's
    integers and record bytes for every block of the material: none is left out"""
    m = material(name)
    enc = scalar_enc(A, m)
    for kind in (I16_KIND, F64_KIND, "planar"):
        view, flags = on_gpu(A, torch, name, kind)
        check_codes(A, enc, m, enc.encode(view, flags), f"{name} {kind} encode")
        out = enc.encode_pack(view, flags, want_mantissa=True)
        check_codes(A, enc, m, out, f"{name} {kind} encode_pack")
        check_records(m, out, m["records"], f"{name} {kind} encode_pack")
        body, total = enc.gather_body(out["payload"], out["n_bytes"])
        head = len(m["data"]) - sum(4 + len(r) for recs in m["records"] if recs for r in recs)
        assert m["data"][head:] == body[:int(total.item())].cpu().numpy().tobytes(), (name, kind)


@functools.lru_cache(maxsize=None)
def vq_records(name, kbps):
    from oracle import pac_oracle_vq as pv
    m = material(name)
    col = []
    data = pv.encode_stream_vq(m["pcm"], m["sr"], kbps, collect=col)
    assert [tuple(bool(x) for x in f) for f, _ in col] == m["flags"]
    recs, _ = nm.records(data)
    out, at = [], 0
    for _, parts in col:
        if parts is None:
            out.append(None)
        else:
            out.append([data[o:o + n] for o, n in recs[at:at + m["n_ch"]]])
            at += m["n_ch"]
    assert at == len(recs)
    return out


@pytest.mark.parametrize("kbps", [96, 128])
@pytest.mark.parametrize("name", MATERIALS)
def test_gain_shape_bytes_against_the_oracle(A, torch, name, kbps):
    """encode_vq (96 kb/s: with SBR, the side chain folds max|FFT| into the overall scale) gives
    oracle.pac_oracle_vq's record bytes through generic and fast views"""
    m = material(name)
    enc = vq_enc(A, m, kbps)
    want = vq_records(name, kbps)
    for kind in (I16_KIND, F64_KIND, "planar"):
        view, flags = on_gpu(A, torch, name, kind)
        out = enc.encode_vq(view, flags)
        assert not (out["status"].cpu().numpy() & A._lib.ST_VQ_UNDEFINED).any()
        check_records(m, out, want, f"{name} {kind} {kbps} kb/s")


def view_of(A, torch, kind):
    return lambda enc, pcm: pl.view(A, enc, torch, stream_planar(np.ascontiguousarray(pcm)), kind)


@pytest.mark.parametrize("kind", [I16_KIND, F64_KIND])
@pytest.mark.parametrize("name", ["windows", "three_channels_odd"])
def test_rate_curve_against_the_model(A, torch, name, kind):
    """test_gpu_abr's comparison of the curve (bits and steps equal, worst within WORST_TOL, sentinels kept)"""
    pcm, sr, bs, cap, a, model = ta.shape_case(name)
    host, dev, enc, view, flags = ta.gpu_curve(A, pcm, sr, bs, cap, view_of=view_of(A, torch, kind))
    ta.compare_curve(f"{name} {kind}", a, cap, model, host, flags)


@pytest.mark.parametrize("kind", [I16_KIND, F64_KIND])
@pytest.mark.parametrize("name", ["mono_odd", "silence_and_drop"])
def test_band_curve_against_the_model(A, torch, name, kind):
    """test_gpu_band's comparisons of the curve and the pick (NMR_TOL, the 1e-4 dB WINDOW)"""
    pcm, sr, bs, target, cap, a, model = tb.shape_case(name)
    g = tb.gpu_curve(A, f"{name} through {kind}", pcm, sr, bs, cap, view_of=view_of(A, torch, kind))
    tb.check_flags(a, g["flags"])
    tb.compare_curve(model, g, f"{name} {kind}")
    pick, ref, near = tb.compare_pick(A, model, g, target, f"{name} {kind}")
    assert not near.any()
    data, out = tb.alloc_stream(A, g, pcm, pick["bit_alloc"])
    assert data == tb.bm.encode(a, pick["bit_alloc"], len(pcm))


@pytest.mark.parametrize("kind", [I16_KIND, F64_KIND])
@pytest.mark.parametrize("name", ["windows", "mono_odd"])
def test_search_against_the_model(A, torch, name, kind):
    """encode_pack_nmr: test_gpu_rate's comparison of the budgets with the model's search outside the tie WINDOW, and
    the model encoder's bytes from those budgets"""
    pcm, sr, bs, target, cap, a = tr.shape_case(name)
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, cap, bs, None)
    view = view_of(A, torch, kind)(enc, pcm)
    out = enc.encode_pack_nmr(view, flags, float(target), cp.targetBitsPerSample)
    n_ch = pcm.shape[1]
    info = {"budget": out["budget"].cpu().numpy().reshape(-1, n_ch, 8),
            "capped": (out["status"].cpu().numpy().reshape(-1, n_ch) & A._lib.ST_RATE_CAP) != 0}
    tr.compare_budgets(a, info, target, cap, f"{name} {kind}")
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    data = A.pacfile.header_bytes(cp) + body[:int(total.item())].cpu().numpy().tobytes()
    assert data == rm.encode(a, info["budget"], len(pcm))


@pytest.mark.parametrize("kind", [I16_KIND, F64_KIND])
@pytest.mark.parametrize("name", ["windows", "three_channels_odd"])
def test_nmr_against_the_model(A, torch, name, kind):
    """pacx_nmr_batch with the ORIGINAL in a generic view: test_gpu_nmr's comparison with nmr_model (DB_TOL)"""
    m = material(name)
    enc = scalar_enc(A, m)
    view, flags = on_gpu(A, torch, name, kind)
    out = enc.encode_pack(view, flags)
    acc = A.quality._Accumulator(enc, m["F"], m["n_ch"])
    acc.chunk(0, view, flags, out["payload"], out["n_bytes"], out["status"])
    written = out["n_bytes"].view(m["F"], m["n_ch"])[:, 0].cpu().numpy() > 0
    record, _ = A.quality.record_map(m["packed"], ~written, m["n_ch"])
    rep = acc.report(enc, m["packed"], record)
    model = nm.model(m["pcm"], m["data"], True)
    assert tn.compare(rep, model, 2e-12, 0.0, f"{name} {kind}") == 0


# ---------------------------------------------------------------------------------------------------- C3
def prefilled(torch, out, byte):
    for t in out.values():
        if hasattr(t, "view") and hasattr(t, "is_cuda"):
            t.view(torch.uint8).fill_(byte)
    return out


def curve_defined(enc, c, n_ch, band):
    host = {k: c[k].cpu().numpy() for k in (("nmr", "cap", "cap_alloc") if band else ("worst", "bits", "steps"))}
    if band:
        live = host["cap"] >= 0
        short = live[:, 1]
        slots = slot_mask(enc, short) & live.any(axis=1)[:, None]
        host["nmr"] = np.where(slots[:, :, None], host["nmr"], 0.0)
        host["cap_alloc"] = np.where(slots, host["cap_alloc"], 0)
    else:
        used = ta.used_mask({"worst": host["worst"], "steps": host["steps"], "sub_stride": c["sub_stride"]})
        host["worst"], host["bits"] = np.where(used, host["worst"], 0.0), np.where(used, host["bits"], 0)
    return host


ENTRIES = ("encode", "encode_pack", "encode_vq", "encode_pack_nmr", "rate_curve", "band_curve")


def run_entry(A, torch, enc, entry, view, flags, byte):
    """one entry point into out= tensors prefilled with `byte` -> the defined part of what it left"""
    n_cf, n_ch, dev = view.n_cf, view.n_channels, enc.device
    cap = 320 / (enc.sample_rate / 1000)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    if entry == "encode":
        return defined(enc, enc.encode(view, flags, prefilled(torch, enc.alloc_outputs(n_cf), byte)), flags, n_ch)
    if entry == "encode_pack":
        out = prefilled(torch, enc.alloc_outputs(n_cf, with_payload=True), byte)
        return defined(enc, enc.encode_pack(view, flags, out, want_mantissa=True), flags, n_ch)
    if entry == "encode_vq":
        out = {"overall": i32(n_cf, 8), "bit_alloc": i32(n_cf, enc.band_stride), "status": i32(n_cf),
               "payload": torch.zeros((n_cf, enc.payload_stride), dtype=torch.uint8, device=dev), "n_bytes": i32(n_cf)}
        return defined(enc, enc.encode_vq(view, flags, prefilled(torch, out, byte)), flags, n_ch)
    if entry == "encode_pack_nmr":
        out = enc.alloc_outputs(n_cf, with_payload=True)
        out["budget"] = i32(n_cf, 8)
        return defined(enc, enc.encode_pack_nmr(view, flags, -3.0, cap, prefilled(torch, out, byte), want_mantissa=True),
                       flags, n_ch)
    if entry == "rate_curve":
        row, _ = enc.rate_curve_layout(cap)
        out = {"worst": torch.zeros((n_cf, row), dtype=torch.float64, device=dev), "bits": i32(n_cf, row),
               "steps": i32(n_cf, 8)}
        return curve_defined(enc, enc.rate_curve(view, flags, cap, prefilled(torch, out, byte)), n_ch, False)
    out = {"nmr": torch.zeros((n_cf, enc.band_stride, A._lib.BAND_CAND), dtype=torch.float64, device=dev),
           "cap": i32(n_cf, 8), "cap_alloc": i32(n_cf, enc.band_stride)}
    return curve_defined(enc, enc.band_curve(view, flags, cap, prefilled(torch, out, byte)), n_ch, True)


@pytest.mark.parametrize("order", ["fast mixed, then generic long", "generic mixed, then fast long"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_no_state_carried_between_paths(A, torch, entry, order):
    """C3: a block-switched batch of 27 channel-frames (status words with SHORT and ZERO_SUBBLOCK, eight overall
    scales per frame) on one path, then a smaller all-long batch on the other path into outputs prefilled with 0x5A:
    its defined outputs are those of the same call on a fresh handle into zero-filled outputs"""
    big, small = material("silence_and_drop_3ch"), material("mono_odd")
    kw = {"use_vq": True, "use_sbr": True} if entry == "encode_vq" else {}
    rate = (96 if entry == "encode_vq" else 128) / 48.0
    first_kind, second_kind = ("planar", "shifted") if order.startswith("fast") else ("interleaved", "planar")
    used, fresh = A.engine.Encoder(48000, rate, **kw), A.engine.Encoder(48000, rate, **kw)
    try:
        big_view = pl.view(A, used, torch, big["planar"], first_kind)
        big_flags = torch.as_tensor(big["packed"], device=used.device)
        left = run_entry(A, torch, used, entry, big_view, big_flags, 0)
        status = left.get("status")
        if status is not None:
            assert (status & 1).any() and (status & 2).any()
        small_view = pl.view(A, used, torch, small["planar"], second_kind)
        assert small_view.n_cf < big_view.n_cf
        got = run_entry(A, torch, used, entry, small_view, None, 0x5A)
        want = run_entry(A, torch, fresh, entry, small_view, None, 0)
        same(got, want, f"{entry}: {order}")
        if "status" in got:
            assert not (got["status"] & 3).any()
    finally:
        torch.cuda.synchronize()
        used.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------- C5
GUARD_K, GUARD_CYCLES = 17, 37.3          # the frame kept: boundary 2^18 - 1 of the 20-bit code, 37.3 cycles per block


@functools.lru_cache(maxsize=None)
def guard_frame(k=GUARD_K, cycles=GUARD_CYCLES):
    """a float64 sine whose long-block maximum (sine window, the oracle's MDCT) sits on the ScaleFactor boundary
    (2^(k+1) - 1) / (2^20 - 1): the two adjacent doubles of the amplitude returned straddle the change of the oracle's
    ScaleFactor of its own maximum -> (frame [2048] at the lower amplitude, relative distance of the two maxima)"""
    t = np.arange(2 * HOP)
    shape = np.sin(2 * np.pi * cycles * (t + 0.5) / (2 * HOP))
    win = po.sine_window(2 * HOP)

    def peak(amp):
        return float(np.max(np.abs(po.mdct_forward(win * (amp * shape), HOP, HOP)[:HOP])))

    def sf(amp):
        return po.scale_factor(peak(amp), 4)

    s = 2 ** 20 - 1
    amp = 0.5 * ((2 ** (k + 1) - 1) / s) / peak(0.5)
    lo, hi = amp * (1 - 1e-9), amp * (1 + 1e-9)
    assert 0 < hi < 1 and sf(lo) == sf(hi) + 1                       # ScaleFactor falls as the maximum grows
    while np.nextafter(lo, 2.0) < hi:
        mid = 0.5 * (lo + hi)
        if sf(mid) == sf(lo):
            lo = mid
        else:
            hi = mid
    assert sf(lo) == sf(hi) + 1
    return lo * shape, abs(peak(hi) - peak(lo)) / peak(lo)


def guard_status(A, torch, guard, flags, k=GUARD_K, cycles=GUARD_CYCLES):
    frame, gap = guard_frame(k, cycles)
    assert gap < 1e-14                                              # far inside the guard's 1e-12 of the maximum
    enc = A.engine.Encoder(48000, 128 / 48.0, guard=guard)
    try:
        blocks = torch.as_tensor(frame.reshape(1, 1, 2 * HOP), device=enc.device)
        fl = None if flags is None else torch.as_tensor(np.array([flags], np.uint8), device=enc.device)
        out = enc.encode(A.engine.PcmView.frames(blocks), fl)
        status = int(out["status"].cpu().numpy()[0]) & 0xFFFFFFFF
        mx = float(enc.mdct(A.engine.PcmView.frames(blocks)).abs().max())
    finally:
        enc.close()
    return status, mx


@pytest.mark.parametrize("flags", [None, 0])
def test_guard_flag_through_a_generic_view(A, torch, flags):
    """C5: include/pacx.h promises PACX_ST_GUARD for a block whose maximum sits on a ScaleFactor boundary, whatever
    the view's layout.  The frame kept is k = 17 at 37.3 cycles per block, float64 on PcmView.frames (the generic
    k_mdct_long): on the build before k_mdct_long took the status pointer this test failed with status 0 (nothing
    else flags the frame), with and without frame flags."""
    status, mx = guard_status(A, torch, True, flags)
    half = ((2 ** 20 - 1) * mx + 1) / 2
    print(f"block maximum {mx!r}: (s mx + 1) / 2 = 2^{GUARD_K} {half - 2 ** GUARD_K:+.3g}, status {status}")
    assert abs(half - 2 ** GUARD_K) < 1e-6
    assert status & A._lib.ST_GUARD, status
    assert not guard_status(A, torch, False, flags)[0] & A._lib.ST_GUARD      # a handle without guard: the bit stays clear


# ----------------------------------------------------------------------------------------------------- D
def test_pcm_view_refuses_views_that_leave_their_storage(A, torch):
    """tensors only, no kernel: one element too far in each stride, and a slice that is legal only through the storage
    behind it"""
    V = A.engine.PcmView
    dev = torch.device("cuda", torch.cuda.current_device())
    F, C, fs, cs, ss = 3, 2, 4100, 9000, 2
    need = (F - 1) * fs + (C - 1) * cs + 2047 * ss + 1
    exact = torch.zeros(need, dtype=torch.int16, device=dev)
    V(exact, C, F, fs, cs, ss)
    for bad in ((fs + 1, cs, ss), (fs, cs + 1, ss), (fs, cs, ss + 1)):
        with pytest.raises(ValueError, match="storage"):
            V(exact, C, F, *bad)
    with pytest.raises(ValueError, match="storage"):
        V(exact[1:], C, F, fs, cs, ss)
    with pytest.raises(ValueError, match="storage"):
        V(torch.zeros(need, dtype=torch.float64, device=dev)[1:], C, F, fs, cs, ss)
    V(exact, C, 0, 10 ** 9, 10 ** 9, 10 ** 9)                          # zero frames always pass
    # a slice shorter than the view, legal because of the storage behind it
    whole = torch.zeros(need + 5, dtype=torch.int16, device=dev)
    piece = whole[5:5 + 16]
    assert piece.numel() < need
    v = V(piece, C, F, fs, cs, ss)
    assert v.c.data == whole.data_ptr() + 10
    with pytest.raises(ValueError, match="storage"):
        V(whole[6:6 + 16], C, F, fs, cs, ss)
    # the stream and frames constructors fit exactly
    V.stream(torch.zeros((2, 4 * HOP), dtype=torch.int16, device=dev))
    V.frames(torch.zeros((3, 2, 2 * HOP), dtype=torch.float64, device=dev))


def test_negative_strides_stay_refused(A, torch):
    m = material("mono_odd")
    enc = scalar_enc(A, m)
    planar = torch.as_tensor(m["planar"], device=enc.device)
    for strides in ((-HOP, planar.shape[1], 1), (HOP, -8, 1), (HOP, planar.shape[1], -1)):
        with pytest.raises(A.PacxError, match="stride"):
            enc.mdct(A.engine.PcmView(planar, 1, 2, *strides))
