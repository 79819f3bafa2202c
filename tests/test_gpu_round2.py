"""GPU parity tests added in round 2: KBDWindow (coder/window.py:45-57) through the C ABI,
decode of malformed records, oracle comparison on a batch large enough for the
multi-iteration paths of the persistent kernels (>= 32 768 channel-frames)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu
MDCT_TOL = 2e-12       # relative to max |X| of the block


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    return a


@pytest.fixture(scope="module")
def kbd():
    return np.load(os.path.join(GOLDEN, "kbd.npz"))


# ------------------------------------------------------------------- KBD window
def test_kbd_window_values_bit_equal(A, torch, kbd):
    """window.KBDWindow through pacx_window_batch (resident alpha = 4 tables) and
    pacx_window_table_batch (any alpha / length) against the reference's values."""
    for n in (2048, 256):
        assert np.array_equal(A.window.KBDWindow(np.ones(n)), kbd[f"kbd_{n}"])
        assert np.array_equal(A.window.KBDWindow(kbd[f"x_{n}"]), kbd[f"kbd_x_{n}"])
    assert np.array_equal(A.window.KBDWindow(kbd["rand_x"]), kbd["rand_kbd_x"])
    assert np.array_equal(A.window.KBDWindow(np.ones(1024)), kbd["kbd_1024"])
    assert np.array_equal(A.window.KBDWindow(kbd["x_1024"]), kbd["kbd_x_1024"])
    assert np.array_equal(A.window.KBDWindow(np.ones(2048), alpha=2.5), kbd["kbd_2048_alpha2p5"])
    assert np.array_equal(A.window.KBDWindow(np.ones(512)), kbd["kbd_512_alpha4"])


def test_mdct_of_kbd_windowed_block(A, torch, kbd):
    """MDCT(KBDWindow(x), N//2, N//2) of the six-tone block, the expression at
    coder/bitalloc.py:161, three ways: PACX_MDCT_KBD on float64 input (window fused into the
    kernel), mdct.MDCT on the GPU-windowed block, and the short-block size."""
    enc = A.context.encoder(48000, 128 / 48.0)
    want = kbd["mdct_kbd_x_2048"]
    ref = np.max(np.abs(want))
    x = torch.as_tensor(kbd["x_2048"], device=enc.device).view(1, 1, 2048)
    got = enc.mdct(A.engine.PcmView.frames(x), kbd=True)[0].cpu().numpy()
    assert np.max(np.abs(got - want)) <= MDCT_TOL * ref
    got2 = A.mdct.MDCT(A.window.KBDWindow(kbd["x_2048"]), 1024, 1024)
    assert np.max(np.abs(got2 - want)) <= MDCT_TOL * ref
    # short: the 256-sample block parked at sub-block 0 (samples 448..704)
    frame = np.zeros(2048)
    frame[448:448 + 256] = kbd["x_256"]
    xs = torch.as_tensor(frame, device=enc.device).view(1, 1, 2048)
    gs = enc.mdct(A.engine.PcmView.frames(xs), short=True, kbd=True)[0, 0].cpu().numpy()
    ws = kbd["mdct_kbd_x_256"]
    assert np.max(np.abs(gs - ws)) <= MDCT_TOL * np.max(np.abs(ws))
    # int16 input goes through the same kernel: against the oracle on the rounded codes
    codes = np.rint(32767 * kbd["x_2048"]).astype(np.int16)
    xi = torch.as_tensor(codes, device=enc.device).view(1, 1, 2048)
    gi = enc.mdct(A.engine.PcmView.frames(xi), kbd=True)[0].cpu().numpy()
    wi = po.mdct_forward(po.kbd_window(2048) * po.pcm16_to_fraction(codes), 1024, 1024)
    assert np.max(np.abs(gi - wi)) <= MDCT_TOL * np.max(np.abs(wi))
    with pytest.raises(A.PacxError):
        enc.mdct(A.engine.PcmView.frames(x), flags=[(0, 0, 1)], kbd=True)


def test_builtin_tables_equal_uploaded_ones(A, torch):
    """A handle created with NULL table pointers (what a C host does) must code exactly as
    the Python host's handle: same .pac payload bytes, pacx_tables_exact() == 1."""
    import ctypes
    L = A._lib
    lib = A.load()
    for sr in (48000, 44100):
        enc = A.context.encoder(sr, 128 / (sr / 1000))
        assert enc.tables_exact()
        cfg = L.PacxConfig()
        cfg.abi_version, cfg.device, cfg.sample_rate = L.PACX_ABI_VERSION, enc.device.index, sr
        cfg.n_lines_long, cfg.n_lines_short, cfg.n_scale_bits, cfg.n_mant_size_bits = 1024, 128, 4, 12
        bl = (ctypes.c_int32 * 25)()
        bs = (ctypes.c_int32 * 25)()
        nl, ns = ctypes.c_int32(), ctypes.c_int32()
        assert lib.pacx_default_bands(sr, 1024, bl, ctypes.byref(nl)) == 0
        assert lib.pacx_default_bands(sr, 128, bs, ctypes.byref(ns)) == 0
        assert list(bl[:nl.value]) == enc.sfBands.nLines.tolist()
        cfg.n_bands_long, cfg.n_bands_short = nl.value, ns.value
        cfg.band_lines_long = ctypes.cast(bl, L.c_int32_p)
        cfg.band_lines_short = ctypes.cast(bs, L.c_int32_p)
        cfg.target_bits_per_sample = 128 / (sr / 1000)
        h = ctypes.c_void_p()
        assert lib.pacx_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.pacx_last_error(None)
        try:
            assert lib.pacx_tables_exact(h) == 1
            pcm = A.synth.stream(16, 2, sample_rate=sr)
            planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
            view = A.engine.PcmView.stream(planar)
            want = {k: (v.clone() if v is not None else None) for k, v in enc.encode_pack(view).items()}
            bare = A.engine.Encoder.__new__(A.engine.Encoder)      # same calls on the bare handle
            bare.__dict__.update(enc.__dict__)
            bare.h = h
            got = bare.encode_pack(view)
            bare.h = None
            for k in ("overall", "scale_factor", "bit_alloc", "n_bytes"):
                assert torch.equal(got[k], want[k]), (sr, k)
            nb = want["n_bytes"].cpu().numpy()
            pg, pw = got["payload"].cpu().numpy(), want["payload"].cpu().numpy()
            for i in range(len(nb)):                   # a slot is only defined up to its n_bytes
                assert pg[i, :nb[i]].tobytes() == pw[i, :nb[i]].tobytes(), (sr, i)
        finally:
            lib.pacx_destroy(h)
    # a rate without built-in Bark/threshold tables says so
    cfg.sample_rate = 32000
    bl32 = (ctypes.c_int32 * 25)()
    assert lib.pacx_default_bands(32000, 1024, bl32, ctypes.byref(nl)) == 0
    cfg.n_bands_long, cfg.band_lines_long = nl.value, ctypes.cast(bl32, L.c_int32_p)
    assert lib.pacx_default_bands(32000, 128, bs, ctypes.byref(ns)) == 0
    cfg.n_bands_short = ns.value
    cfg.target_bits_per_sample = 4.0
    h = ctypes.c_void_p()
    assert lib.pacx_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.pacx_last_error(None)
    assert lib.pacx_tables_exact(h) == 0
    lib.pacx_destroy(h)


# ------------------------------------------------------- malformed input, decode side
def _stream_and_pac(A, vq):
    ex = load_excerpt("castanet")
    pcm = ex["pcm"][:12 * 1024]
    sr = int(ex["sr"])
    return A.pacfile.encode_stream(pcm, sr, 128, block_switching=True, use_vq=vq, use_sbr=False)


@pytest.mark.parametrize("vq", [False, True])
def test_truncated_and_corrupt_pac_raise(A, torch, vq):
    """The reference stops with 'Only read a partial block of coded PACFile data'
    (coder/pacfile.py:203-205) on a file cut short; a record whose fields cannot be what
    the coder wrote (an allocation field above maxMantBits, fields past the record's end)
    must do the same here instead of steering the bit cursor out of the record."""
    pac = _stream_and_pac(A, vq)
    good = A.pacfile.decode_stream(pac)
    assert good.shape[0] > 0
    for cut in (len(pac) - 1, len(pac) - 200, len(pac) // 2 + 1):
        with pytest.raises(RuntimeError, match="partial block"):
            A.pacfile.decode_stream(pac[:cut])
    # a length field that points past the end of the file
    cp, pos = A.pacfile.parse_header(pac)
    bad = bytearray(pac)
    bad[pos:pos + 4] = (len(pac)).to_bytes(4, "little")
    with pytest.raises(RuntimeError, match="partial block"):
        A.pacfile.decode_stream(bytes(bad))
    # an impossible allocation in the first band of the first record: 12 bits of ones
    # right after the 3 flag bits and the 4-bit overall scale (coder/pacfile.py:404-447)
    bad = bytearray(pac)
    first = pos + 4
    fl = bad[first] >> 5
    assert not (fl & 2), "first block of the excerpt is a long block"
    bits = int.from_bytes(bad[first:first + 4], "big")
    bits |= 0xFFF << (32 - 7 - 12)
    bad[first:first + 4] = bits.to_bytes(4, "big")
    with pytest.raises(RuntimeError, match="partial block"):
        A.pacfile.decode_stream(bytes(bad))


def test_unpack_status_per_record(A, torch):
    """pacx_unpack_batch: PACX_ST_MALFORMED on exactly the records that are cut short, zeros
    for their codes, the intact neighbours untouched."""
    enc = A.context.encoder(48000, 128 / 48.0)
    pcm = A.synth.stream(8, 2)
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    out = enc.encode_pack(A.engine.PcmView.stream(planar), want_mantissa=True)
    n_bytes = out["n_bytes"].clone()
    short = [3, 10]
    for i in short:
        n_bytes[i] = n_bytes[i] // 2                       # the record ends in mid-band
    n_bytes[5] = 0
    back = enc.unpack(out["payload"], n_bytes)
    st = back["status"].cpu().numpy()
    assert [int(i) for i in np.nonzero(st & A._lib.ST_MALFORMED)[0]] == [3, 5, 10]
    for k in ("overall", "scale_factor", "bit_alloc", "mantissa"):
        got, want = back[k].cpu().numpy(), out[k].cpu().numpy()
        for i in range(16):
            if i in (3, 5, 10):
                assert not got[i].any(), (k, i)
            else:
                assert np.array_equal(got[i], want[i]), (k, i)


# ------------------------------------------- oracle comparison on a large batch
def test_large_batch_sampled_against_oracle(A, torch):
    """BASELINE configs[1] x 4 = 32 768 channel-frames in ONE call: every wave of
    k_mdct_long_x2p runs more than two iterations, the mask / tail kernels walk several units
    per wave and the body gather switches to its chunked scan.  97 channel-frames spread over
    the batch are encoded by the oracle and compared bit for bit (codes and payload bytes);
    the .pac body is checked record by record at those frames."""
    n_frames = 16384
    base = A.synth.stream(4096, 2)
    gains = [1.0, 0.71, 0.5, 0.83]
    pcm = np.concatenate([np.rint(base * g).astype(np.int16) for g in gains])
    enc = A.context.encoder(48000, 128 / 48.0)
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    out = enc.encode_pack(A.engine.PcmView.stream(planar), want_mantissa=True)
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    host = {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "flags"}
    n_cf = 2 * n_frames
    assert host["n_bytes"].shape[0] == n_cf == 32768
    total = int(total.item())
    assert total == int(host["n_bytes"].astype(np.int64).sum()) + 4 * n_cf
    offs = np.concatenate(([0], np.cumsum(host["n_bytes"].astype(np.int64) + 4)))
    body = body[:total].cpu().numpy()
    p = po.make_params(48000, 2, 128)
    halo = np.concatenate((np.zeros((1024, 2), np.int16), pcm))
    for i in np.unique(np.concatenate((np.linspace(0, n_cf - 1, 89).astype(int),
                                       [1, 4095, 8191, 8192, 16383, 16384, 32766, 32767]))):
        f, ch = divmod(int(i), 2)
        sf, ba, mant, ov = po.encode_channel(po.pcm16_to_fraction(halo[f * 1024:f * 1024 + 2048, ch]), p)
        r = A.codec.unpack_long(enc, host, i)
        assert r[3] == ov and r[1].tolist() == ba.tolist(), i
        assert r[0].tolist() == sf.tolist() and r[2].tolist() == mant.tolist(), i
        nb_want, want = po.pack_channel_block(p, (0, 0, 0), [(sf, ba, mant, ov)])
        n = int(host["n_bytes"][i])
        assert n == nb_want == len(want), i
        assert host["payload"][i, :n].tobytes() == want, i
        rec = body[offs[i]:offs[i + 1]].tobytes()
        assert rec == len(want).to_bytes(4, "little") + want, i


# ------------------------------------------------ fused mask + tail kernel
@pytest.mark.parametrize("mixed", [False, True])
def test_fused_tail_equals_separate_kernels(A, torch, monkeypatch, mixed):
    """k_mask<1024, true> (SMRs, BitAlloc, scale factors, mantissas and payload of a long frame in
    one wave) against the same stages as separate kernels behind a boundary (PACX_FUSE_TAIL=0:
    k_mask<1024, false> + k_tail_long): every output bit for bit, on an all-long batch and on a
    block-switched one (long frames through the fused kernel, short ones through k_tail_short)."""
    if mixed:
        ex = load_excerpt("castanet")
        sr, pcm = int(ex["sr"]), ex["pcm"][:48 * 1024]
    else:
        sr, pcm = 48000, A.synth.stream(300, 2)

    def handle(fuse):                          # the override is read when a handle is created
        monkeypatch.setenv("PACX_FUSE_TAIL", fuse)
        return A.engine.Encoder(sr, 128 / (sr / 1000))
    sep, fused = handle("0"), handle("1")
    monkeypatch.delenv("PACX_FUSE_TAIL")
    planar = A.pacfile.device_stream(sep, pcm)
    view = A.engine.PcmView.stream(planar)
    flags = sep.transient_flags(planar, len(pcm) // 1024)[1] if mixed else None

    def run(enc):
        out = enc.encode_pack(view, flags, want_mantissa=True)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items() if v is not None}
    try:
        ref, got = run(sep), run(fused)
    finally:
        sep.close()
        fused.close()
    for k in ("overall", "scale_factor", "bit_alloc", "mantissa", "status", "n_bytes"):
        assert torch.equal(got[k], ref[k]), k
    nb = ref["n_bytes"].cpu().numpy()
    pg, pr = got["payload"].cpu().numpy(), ref["payload"].cpu().numpy()
    for i in range(len(nb)):
        assert pg[i, :nb[i]].tobytes() == pr[i, :nb[i]].tobytes(), i
    if mixed:
        assert (ref["status"].cpu().numpy() & 1).any() and not (ref["status"].cpu().numpy() & 1).all()


# ----------------------------------------------------------- PACX_ST_GUARD
def test_guard_flag_on_a_corpus_sample(A, torch):
    """PACX_ST_GUARD marks channel-frames with a rounding decision near its boundary (a mantissa
    or scale-factor quantiser input next to an even integer, coder/quantize.py:73; a BitAlloc
    value next to k + 1/2, coder/bitalloc.py:103).  On a sample of BASELINE configs[4]'s corpus
    (tiles at several levels): few frames are flagged, the oracle agrees bit for bit on un-flagged
    frames spread over the sample -- and, so far, on the flagged ones too (the flag is a margin,
    not an error)."""
    S = A.synth
    base = S.stream_float(512, 2)
    pcm = np.concatenate([S.to_int16(base, S.tile_scale(t)) for t in (0, 5, 10, 15)])      # 2048 hops
    enc = A.engine.Encoder(48000, 128 / 48.0, guard=True)              # pacx_config.guard = 1
    plain = A.context.encoder(48000, 128 / 48.0)                       # default handle: no flag, same codes
    planar = torch.as_tensor(S.planar_with_halo(pcm), device=enc.device)
    out = enc.encode_pack(A.engine.PcmView.stream(planar), want_mantissa=True)
    host = {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "flags"}
    ref = plain.encode_pack(A.engine.PcmView.stream(planar), want_mantissa=True)
    assert not (ref["status"].cpu().numpy() & A._lib.ST_GUARD).any()
    for k in ("overall", "scale_factor", "bit_alloc", "mantissa", "n_bytes"):
        assert torch.equal(out[k], ref[k]), k
    st = host["status"].astype(np.uint32)
    flagged = np.nonzero(st & A._lib.ST_GUARD)[0]
    n_cf = len(st)
    assert n_cf == 4096
    assert len(flagged) < 0.05 * n_cf, f"{len(flagged)} of {n_cf} channel-frames flagged"
    assert not (st & ~np.uint32(A._lib.ST_GUARD | A._lib.ST_ALLOC_CAP)).any()
    p = po.make_params(48000, 2, 128)
    halo = np.concatenate((np.zeros((1024, 2), np.int16), pcm))
    clean = np.setdiff1d(np.linspace(0, n_cf - 1, 40).astype(int), flagged)
    for i in list(clean) + list(flagged[:12]):
        f, ch = divmod(int(i), 2)
        sf, ba, mant, ov = po.encode_channel(po.pcm16_to_fraction(halo[f * 1024:f * 1024 + 2048, ch]), p)
        r = A.codec.unpack_long(enc, host, i)
        assert r[3] == ov and r[1].tolist() == ba.tolist(), i
        assert r[0].tolist() == sf.tolist() and r[2].tolist() == mant.tolist(), i
    print(f"PACX_ST_GUARD: {len(flagged)} of {n_cf} channel-frames flagged")
    enc.close()


# ------------------------------------------- BASELINE configs[4]: one rank's shard
def test_corpus_shard_equals_its_sub_shards(A, torch):
    """One eighth of the 1 048 576-frame corpus (what one of eight ranks encodes: 131 072 stereo
    frames = 262 144 channel-frames in ONE call) against the same hops encoded as eight
    16 384-frame sub-shards with their one-hop halos: the .pac bodies must concatenate to the
    same bytes.  This is the property the multi-GPU sharding rests on, at full shard size (the
    large-batch paths: chunked body scan, many iterations per persistent wave)."""
    S = A.synth
    lo, hi = 131072 * 3, 131072 * 4                      # rank 3 of 8: tiles 96..127, every level
    base = S.stream_float(S.TILE_HOPS, 2)
    enc = A.engine.Encoder(48000, 128 / 48.0, guard=True)

    def body_of(a, b):
        planar = torch.as_tensor(S.corpus_shard(a, b, base=base), device=enc.device)
        view = A.engine.PcmView.stream(planar)
        out = enc.alloc_outputs(view.n_cf, with_payload=True)
        out["mantissa"] = None
        enc.encode_pack(view, None, out)
        body, total = enc.gather_body(out["payload"], out["n_bytes"],
                                      capacity=A.dist.slot_bytes(view.n_cf, 128 / 48.0))
        n = int(total.item())
        st = out["status"].cpu().numpy()
        return body[:n].clone(), st
    whole, st_whole = body_of(lo, hi)
    parts, sts = [], []
    step = (hi - lo) // 8
    for k in range(8):
        b, s = body_of(lo + k * step, lo + (k + 1) * step)
        parts.append(b)
        sts.append(s)
    cat = torch.cat(parts)
    assert cat.numel() == whole.numel()
    assert torch.equal(cat, whole)
    assert np.array_equal(np.concatenate(sts), st_whole)
    flagged = int(np.count_nonzero(st_whole & A._lib.ST_GUARD))
    print(f"corpus shard: {whole.numel()} body bytes for {2 * (hi - lo)} channel-frames, {flagged} flagged PACX_ST_GUARD")
    enc.close()


# ------------------------------------------- scalar mantissas + SBR (useVQ off, useSBR on)
def _sbr_scalar_cases():
    import json
    return json.load(open(os.path.join(GOLDEN, "sbr_scalar.json")))


@pytest.mark.parametrize("case", _sbr_scalar_cases(), ids=lambda e: f"{e['excerpt']}_{e['kbps_per_channel']}")
def test_scalar_sbr_files_follow_the_reference(A, torch, case):
    """The branch of EncodeSingleChannel_SBR the shipped driver never selects (coder/codec.py:529-555):
    where the reference finishes the file the GPU path writes the same bytes (hash of the reference's
    own output, tests/golden/sbr_scalar.json), where it raises -- an omitted band got bits -- the
    kernels flag the block (PACX_ST_REF_RAISES) and the mirror raises the reference's TypeError."""
    import hashlib
    ex = np.load(os.path.join(GOLDEN, f"excerpt_{case['excerpt']}.npz"))
    pcm, sr = ex["pcm"][:case["hops"] * 1024], int(ex["sr"])
    kbps, bs = case["kbps_per_channel"], case["block_switching"]
    if case["outcome"] == "raised":
        with pytest.raises(TypeError, match="item assignment"):
            A.pacfile.encode_stream(pcm, sr, kbps, bs, use_sbr=True)
        return
    pac = A.pacfile.encode_stream(pcm, sr, kbps, bs, use_sbr=True)
    assert len(pac) == case["bytes"]
    assert hashlib.sha256(pac).hexdigest() == case["sha256"]
    # and such a file decodes (no omitted band is coded: plain path, coder/pacfile.py:659-668)
    got = A.pacfile.decode_stream(pac)
    assert list(got.shape) == case["decoded_shape"]
    assert hashlib.sha256(np.ascontiguousarray(got).astype("<i2").tobytes()).hexdigest() == case["decoded_sha256"]


def test_scalar_sbr_block_mirrors(A, torch):
    """codec.Encode_SBR with useVQ off for one long block (the oracle's encode_channel_sbr on the same
    samples), PACFile.Encode's routing (long -> Encode_SBR, short -> Encode), and the file-object loop
    (PACFile.WriteDataBlock) against the batched encode."""
    import io
    ex = np.load(os.path.join(GOLDEN, "excerpt_castanet.npz"))
    pcm, sr = ex["pcm"][:24 * 1024], int(ex["sr"])
    cp = A.audiofile.CodingParams()
    cp.sampleRate, cp.nChannels = sr, 2
    cp.nMDCTLines = cp.nSamplesPerBlock = 1024
    cp.nScaleBits, cp.nMantSizeBits = 4, 12
    cp.targetBitsPerSample = 96 / (sr / 1000)
    cp.useSBR, cp.useVQ = True, False
    cp.numSamples = len(pcm)
    cp.sfBands = A.psychoac.ScaleFactorBands(A.psychoac.AssignMDCTLinesFromFreqLimits(1024, sr))
    cp.sfBandsShort = A.psychoac.ScaleFactorBands(A.psychoac.AssignMDCTLinesFromFreqLimits(128, sr))
    p = po.make_params(sr, 2, 96)
    p.useSBR = True
    p.omittedBands = list(po.omitted_bands(p.sfBands))
    frac = np.stack([po.pcm16_to_fraction(pcm[:2048, c]) for c in range(2)])
    for flags in ((False, False, False), (False, False, True), (True, False, False)):
        sf, ba, mant, ov = A.codec.Encode_SBR([frac[0], frac[1]], cp, *flags)
        for c in range(2):
            want = po.encode_channel_sbr(frac[c], p, *flags)
            assert np.array_equal(sf[c], want[0]) and np.array_equal(ba[c], want[1]) and ov[c] == want[3]
            n = len(mant[c])
            assert np.array_equal(mant[c], want[2][:n]) and not np.any(want[2][n:])
    # a frame on which the reference raises: a loud harpsichord block
    hx = np.load(os.path.join(GOLDEN, "excerpt_harpsichord.npz"))
    hp = po.make_params(int(hx["sr"]), 2, 96)
    hp.useSBR = True
    hp.omittedBands = list(po.omitted_bands(hp.sfBands))
    cph = A.audiofile.CodingParams()
    cph.__dict__.update(cp.__dict__)
    cph.sampleRate = int(hx["sr"])
    cph.targetBitsPerSample = 96 / (cph.sampleRate / 1000)
    cph.sfBands = A.psychoac.ScaleFactorBands(A.psychoac.AssignMDCTLinesFromFreqLimits(1024, cph.sampleRate))
    cph.sfBandsShort = A.psychoac.ScaleFactorBands(A.psychoac.AssignMDCTLinesFromFreqLimits(128, cph.sampleRate))
    hit = False
    for h in range(1, 12):
        blk = [po.pcm16_to_fraction(hx["pcm"][(h - 1) * 1024:(h + 1) * 1024, c]) for c in range(2)]
        try:
            po.encode_channel_sbr(blk[0], hp)
            po.encode_channel_sbr(blk[1], hp)
        except TypeError:
            with pytest.raises(TypeError, match="item assignment"):
                A.codec.Encode_SBR(blk, cph)
            hit = True
            break
    assert hit
    # the file-object loop writes what the batched call writes
    want = A.pacfile.encode_stream(pcm, sr, 96, True, use_sbr=True)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.pac")
        f = A.pacfile.PACFile(path)
        cp2 = A.audiofile.CodingParams()
        cp2.__dict__.update(cp.__dict__)
        f.OpenForWriting(cp2)
        look = np.zeros((2, 2048))
        last = cur = False
        n_hops = len(pcm) // 1024
        for h in range(n_hops + 1):
            if h < n_hops:
                data = np.stack([po.pcm16_to_fraction(pcm[h * 1024:(h + 1) * 1024, c]) for c in range(2)])
                look = np.concatenate((data, look[:, 1024:]), axis=1)
                nxt = bool(po.transient_detect(look))
            else:
                nxt = False
            f.WriteDataBlock([look[c, :1024] for c in range(2)], cp2, last, cur, nxt)
            last, cur = cur, nxt
        f.Close(cp2)
        assert open(path, "rb").read() == want


# ------------------------------------------- transient detector: exact ties of peak / avg against 4.5
TIE_BUFSIZE = 8192                     # NumPy's buffer: np.add.reduce starts a second pairwise run there (PACX_NP_BUFSIZE)
TIE_A_MIN = {6: 866, 8: 525}           # peak columns from which n_ch * (a + 500) > 8192 (8 * (524 + 500) is 8192 itself)


def _tie_hop(rng, n_ch, a_min=0):
    """one hop [1024, n_ch] of int16 whose peak-to-average ratio is EXACTLY 4.5 in rational arithmetic:
    peak code P = 9 q in channel 0 at column a >= a_min, upto = a + 500 columns counted (zeros past 1024), the codes
    of all channels over those columns summing to 2 P n / 9 with n = n_ch * upto.  The detector's upto is the LARGEST
    first-maximum column of any channel plus 500, so the first maximum of every channel but 0 is moved to a column
    not after a (two codes of that channel change places; the sum stays), and its codes past the counted columns
    stay at or below that maximum: a tie whatever the number of channels."""
    while True:
        q = int(rng.integers(1, 40))
        P = 9 * q
        a = int(rng.integers(a_min, 1024))
        upto = min(a + 500, 2048)
        cols = min(upto, 1024)
        n_free = n_ch * cols - 1
        rest = 2 * q * n_ch * upto - P
        if rest < 0 or rest > (P - 1) * n_free:
            continue
        base, extra = divmod(rest, n_free)
        vals = np.full(n_free, base, dtype=np.int64)
        vals[rng.permutation(n_free)[:extra]] += 1
        for _ in range(8):                            # shuffle mass around between drawn pairs, the sum stays
            order = rng.permutation(n_free)
            i, j = order[:n_free // 2], order[n_free // 2:2 * (n_free // 2)]
            d = rng.integers(0, P, len(i))
            ok = (vals[i] + d <= P - 1) & (vals[j] - d >= 0)
            vals[i] += np.where(ok, d, 0)
            vals[j] -= np.where(ok, d, 0)
        m = np.zeros((n_ch, 1024), dtype=np.int64)
        flat = np.delete(np.arange(n_ch * cols), a)   # (channel, column) of the free codes, channel-major; (0, a) left out
        m[flat // cols, flat % cols] = vals
        m[0, a] = P
        m[0, cols:] = rng.integers(0, P, 1024 - cols)
        for ch in range(1, n_ch):
            first, to = int(np.argmax(m[ch, :cols])), int(rng.integers(0, a + 1))
            if first > a:
                m[ch, first], m[ch, to] = m[ch, to], m[ch, first]
            m[ch, cols:] = rng.integers(0, m[ch, :cols].max() + 1, 1024 - cols)
        assert m[:, :cols].sum() == 2 * q * n_ch * upto and m.max() == P and int(np.argmax(m[0])) == a
        assert np.argmax(m, axis=1).max() == a
        sign = rng.choice([-1, 1], size=m.shape)
        return (m * sign).T.astype(np.int16)


def _tie_reference(A, pcm, n_ch):
    """detect_transients.hop_transients (the reference expression on float64) of every hop of int16 [n * 1024, n_ch]"""
    n_hops = len(pcm) // 1024
    return A.detect_transients.hop_transients(
        np.stack([A.pcmfile.codes_to_fraction(pcm[:, ch]) for ch in range(n_ch)]).reshape(n_ch, n_hops, 1024).transpose(1, 0, 2))


def _tie_counts(pcm, n_ch):
    """(upto, exact tie) of every hop, as the detector counts: upto = the largest first-maximum column of any channel
    plus 500; a tie where 2 P n = 9 S for the peak code P, n = n_ch * upto and S the sum of the codes counted"""
    mag = np.abs(pcm.astype(np.int64)).reshape(-1, 1024, n_ch)
    upto = np.minimum(mag.argmax(axis=1).max(axis=1) + 500, 2048)
    counted = np.arange(1024)[None, :, None] < upto[:, None, None]
    return upto, 2 * mag.max(axis=(1, 2)) * n_ch * upto == 9 * (mag * counted).sum(axis=(1, 2))


def _tie_decisions(A, enc, planar, n_hops):
    tr, _ = enc.transient_flags(planar, n_hops)
    return tr.cpu().numpy().astype(bool)


@pytest.mark.parametrize("n_ch", [1, 2, 3, 5, 6, 8])
def test_transient_detector_exact_ties(A, torch, n_ch):
    """Quiet passages of small codes put peak / avg exactly on the detector's threshold now and then (a parity
    soak found one stream in two thousand): coder/detect_transients.py:20-21 then goes by the rounding of its
    pairwise float mean.  k_transient decides by integers and redoes that mean in NumPy's order at a tie:
    600 constructed ties per channel count, decisions equal to the reference expression's.  One and two channels take
    the kernel's register body, three and more its strided one.  With six and eight channels 200 further ties have
    their peak so late that n_ch * upto passes 8192 elements, where NumPy's sum is made of more than one pairwise run;
    and the two-channel ties are given once more as a view one sample off its alignment, which the strided body
    serves.  That every hop is a tie in integers is asserted.  (Until the strided body was tested, _tie_hop let the
    other channels have their maximum after channel 0's, which moves upto -- 267 of the 600 two-channel hops were
    ties -- and shuffled codes in a Python loop, 15 s for that case.)"""
    rng = np.random.default_rng(2024 + n_ch)
    hops = [_tie_hop(rng, n_ch) for _ in range(600)]
    pcm = np.concatenate(hops)
    want = _tie_reference(A, pcm, n_ch)
    enc = A.context.encoder(48000, 128 / 48.0)
    tr, _ = enc.transient_flags(A.pacfile.device_stream(enc, pcm), len(hops))
    got = tr.cpu().numpy().astype(bool)
    assert got.tolist() == want.tolist(), f"{int((got != want).sum())} of {len(hops)} tie hops decided differently"
    print(f"exact ties, {n_ch} channel(s): {int(want.sum())} of {len(hops)} are transients to the reference")
    assert _tie_counts(pcm, n_ch)[1].all()
    if n_ch == 2:                          # the strided body at the channel count the register body normally serves
        aligned = A.pacfile.device_stream(enc, pcm)
        flat = torch.zeros(aligned.numel() + 8, dtype=torch.int16, device=enc.device)
        off = flat[1:1 + aligned.numel()].view(aligned.shape)
        off.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2 and off.is_contiguous()
        got = _tie_decisions(A, enc, off, len(hops))
        assert got.tolist() == want.tolist(), \
            f"{int((got != want).sum())} of {len(hops)} tie hops decided differently through the view off its alignment"
    if n_ch in TIE_A_MIN:
        hops = [_tie_hop(rng, n_ch, TIE_A_MIN[n_ch]) for _ in range(200)]
        pcm = np.concatenate(hops)
        upto, ties = _tie_counts(pcm, n_ch)
        assert ties.all() and (n_ch * upto > TIE_BUFSIZE).all() and n_ch * (TIE_A_MIN[n_ch] - 1 + 500) <= TIE_BUFSIZE
        want = _tie_reference(A, pcm, n_ch)
        got = _tie_decisions(A, enc, A.pacfile.device_stream(enc, pcm), len(hops))
        assert got.tolist() == want.tolist(), \
            f"{int((got != want).sum())} of {len(hops)} tie hops past NumPy's buffer border decided differently"
        print(f"exact ties past {TIE_BUFSIZE} elements, {n_ch} channels: {int(want.sum())} of {len(hops)} are transients")


# ------------------------------------------- an exactly zero MDCT line and the reference's SPL(0) rule
def test_exactly_zero_line_takes_the_references_spl_rule(A, torch):
    """coder/psychoac.py:13-24: SPL() replaces an intensity that is EXACTLY zero by 1e-8 (+16 dB) before the log,
    while 1e-40 ends on the -30 dB floor.  A block whose last hop is written twice ([a, a], what the reference's
    driver does at the end of every file) with a sparse a has lines that are zero in exact arithmetic; this build's
    FFT returns 0.0 for them (pocketfft leaves 1e-21: the parity soak's 'zero-line' class).
    Whatever the FFT returns, k_mask must apply the reference's rule to it: the oracle's CalcSMRs fed the PRODUCT's
    lines gives the product's SMRs, and the exact zeros are what carries the band maxima (+16 dB against -30)."""
    a = np.zeros(1024, np.int16)
    a[[3, 18, 73, 97, 147, 416, 998]] = -1
    a[[21, 505, 680]] = 1
    blk = np.concatenate((a, a))                                        # seed 102376 of the soak, channel 1
    enc = A.context.encoder(48000, 96 / 48.0)
    view = A.engine.PcmView.frames(torch.as_tensor(blk, device=enc.device).view(1, 1, 2048))
    lines, scale = enc.mdct(view, want_scale=True)
    smr = enc.smr(view, lines).cpu().numpy()[0]
    lines, ov = lines.cpu().numpy()[0], int(scale.cpu().numpy()[0])
    assert np.count_nonzero(lines == 0.0) >= 1 and np.max(np.abs(lines)) > 0
    p = po.make_params(48000, 2, 96)
    data = po.pcm16_to_fraction(blk)
    want = po.calc_smrs(data, lines * (1 << ov), ov, 48000, p.sfBands)
    nb = p.sfBands.nBands
    assert np.max(np.abs(smr[:nb] - want)) < 1e-9
    floor_only = po.calc_smrs(data, np.where(lines == 0.0, 1e-30, lines) * (1 << ov), ov, 48000, p.sfBands)
    assert np.max(want - floor_only) > 40.0                             # the rule decides some band by ~46 dB


# ------------------------------------------- sample rates the reference's band table does not reach
@pytest.mark.parametrize("sr", [16000, 30000])
def test_sample_rate_with_an_empty_band_raises_like_the_reference(A, sr):
    """Below 31 kHz the 25-band table has bands above Nyquist, without lines; the reference raises ValueError from
    np.amax over the empty band in CalcSMRs (coder/psychoac.py:289) on its first block, and so do the oracle and
    the host mirror (the C ABI refuses such a layout at pacx_create: PACX_E_ARG 'band with no lines')."""
    pcm = A.synth.stream(4, 2, 48000, seed=3)
    with pytest.raises(ValueError, match="zero-size array"):
        po.encode_stream(pcm, sr, 96, False)
    with pytest.raises(ValueError, match="zero-size array"):
        A.pacfile.encode_stream(pcm, sr, 96)


def test_lowest_sample_rate_the_band_table_reaches(A):
    """31.5 kHz: the last band still has lines (16 long, 2 short): bytes against the oracle, block switching on"""
    pcm = A.synth.stream(6, 2, 48000, seed=4)
    pcm[3 * 1024 + 100:3 * 1024 + 140] = 28000
    assert A.pacfile.encode_stream(pcm, 31500, 96, True) == po.encode_stream(pcm, 31500, 96, True)
