"""The gain-shape decoders (k_vq_dec, k_vq_dec_frame, k_sbr_recon, then the IMDCT / overlap-add kernels) on the drawn
streams of tests/vq_code_streams.py: records the format defines and no encoder writes from audio -- allocations on both
sides of the frame decoder's node store, angle index 0 and the largest angle, children of exactly 0 / 32 / 33 bits,
K = 0 leaves, the first and last index of a codebook, leaves of 2, 3 and 4 lines with the largest K their 32 bits
allow (K = 2^30: beyond the oracle's own codebook layer, decoded by tests/pvq_model.py), negative gains, gain index 0 and
all ones, omitted bands coded one by one, with zero and negative values and over empty low bands, short frames inside an
SBR file, 44.1 and 32 kHz, 1 and 3 channels, header widths 3 / 4.  Well-formed records only; the reference is the
oracle's own reader and decoder on the same bytes (vq_code_streams.decode_float_vq).

Every case runs with the default routing (k_vq_dec_frame, k_vq_dec for the channel-frames beyond its node store) and with
PACX_VQ_DEC_FRAME=0 (k_vq_dec for every frame).  A record drawn freely is beyond the store, so every other frame of a
case is drawn to fit it, and tests/test_vq_code_streams.py asserts that what the case's name says occurs in frames that
fit: the default run takes each case's edges through the frame decoder's own index walk, leaf normalisation, combine and
gain stages, the other run through the band decoder's.

Bars.  Header codes are integers: equal; status 0.  The lines of EVERY block, after SBR reconstruction where it applies,
are within 1e-12 of the block's own peak of the oracle's lines (the bar of test_gpu_vq.test_decode_lines_vs_oracle, no
block skipped); a block whose reference lines are all zero is all zero.  int16 PCM is equal sample for sample:
tests/test_vq_code_streams.py shows that no sample of the oracle's output lies within a hundred times that bar of a step
of the quantiser.  `theta_wide` holds angles of more than 62 bits, which the oracle decodes and the kernels refuse
(DESIGN section 7): exactly those channel-frames carry PACX_ST_VQ_UNDEFINED, and decode_stream raises."""
import functools

import numpy as np
import pytest

import vq_code_streams as vs
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv

pytestmark = pytest.mark.gpu

MODES = (None, "0")                   # PACX_VQ_DEC_FRAME: the default routing, the band decoder for every block


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


@pytest.fixture
def fresh_handles(A):
    """the PACX_* overrides are read when a handle is created: a test that sets them starts and ends with an empty
    handle cache, so that no forced handle leaks into later tests"""
    A.context.clear()
    yield
    A.context.clear()


def _set_env(A, monkeypatch, env):
    for k in ("PACX_VQ_FRAME", "PACX_VQ_BFS", "PACX_VQ_DEC_FRAME"):
        if env.get(k) is not None:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    A.context.clear()                              # decode_stream creates handles that read them


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(int16 PCM of oracle.decode_stream_vq, blocks [n_cf, 2048], lines [n_cf, 1024], samples, peak, infos), once"""
    samples, peak, blocks, lines, infos = vs.decode_float_vq(vs.case(name).pac)
    return po.fraction_to_pcm16(samples), blocks, lines, samples, peak, infos


def handle(A, c):
    """the handle pacfile.decode_stream uses for the case's header"""
    cp, pos = A.pacfile.parse_header(c.pac)
    assert pos == c.header_len and cp.useVQ and bool(cp.useSBR) == c.use_sbr
    enc = A.context.encoder_for_params(cp)
    assert enc.band_stride == c.band_stride and enc.payload_stride >= max(c.sizes, default=0)
    return enc


def check(A, c, out, lines_want, what):
    """Encoder.decode_vq's dict against the drawn header codes and the oracle's lines, block by block"""
    for k in ("flags", "overall", "bit_alloc"):
        have = out[k].cpu().numpy()
        want = getattr(c, k)
        assert have.shape == want.shape and have.dtype == want.dtype, (what, k)
        assert np.array_equal(have, want), (what, k, np.argwhere(have != want)[:4].tolist())
    status = out["status"].cpu().numpy()
    assert np.array_equal(status != 0, c.undefined), (what, status.tolist())
    assert np.all(status[c.undefined] == A._lib.ST_VQ_UNDEFINED), (what, status.tolist())
    lines = out["lines"].cpu().numpy()
    assert lines.shape == lines_want.shape == (len(c.flags), 1024)
    for i in range(len(lines)):
        if c.undefined[i]:
            continue
        peak = np.max(np.abs(lines_want[i]))
        err = np.max(np.abs(lines[i] - lines_want[i]))
        assert err <= 1e-12 * peak, (what, i, int(c.flags[i]), err, peak)      # peak 0: the block is all zero


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n in vs.NAMES if n != "no_hops"])      # a batch call wants records
def test_lines_of_every_block(A, monkeypatch, fresh_handles, name, mode):
    """Encoder.decode_vq(want_lines=True) on the file's bytes with offsets (payloads at every byte alignment), and in
    slot layout with 0xA5 after each record in its slot"""
    import torch
    c = vs.case(name)
    _set_env(A, monkeypatch, {"PACX_VQ_DEC_FRAME": mode})
    enc = handle(A, c)
    lines_want = oracle(name)[2]
    n_cf = len(c.records)
    sizes = torch.as_tensor(c.sizes, device=enc.device)
    offs = c.header_len + 4 + np.concatenate(([0], np.cumsum(c.sizes[:-1].astype(np.int64) + 4)))[:n_cf]
    body = torch.frombuffer(bytearray(c.pac) + bytearray(8), dtype=torch.uint8).to(enc.device)
    out = enc.decode_vq(body, sizes, c.n_ch, offsets=torch.as_tensor(offs.astype(np.int64), device=enc.device),
                        want_lines=True)
    check(A, c, out, lines_want, "stream")
    if not c.undefined.any():
        assert np.array_equal(out["pcm"].cpu().numpy(), oracle(name)[0])
    slots = np.full((n_cf, enc.payload_stride), 0xA5, np.uint8)
    for i, rec in enumerate(c.records):
        slots[i, :len(rec)] = np.frombuffer(rec, np.uint8)
    out = enc.decode_vq(torch.as_tensor(slots, device=enc.device), sizes, c.n_ch, want_lines=True)
    check(A, c, out, lines_want, "slots")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", vs.NAMES)
def test_decode_stream(A, monkeypatch, fresh_handles, name, mode):
    """pacfile.decode_stream whole, in the smallest chunks the streamed decoder takes (one hop of longest records) and
    in chunks of about a hop and a half of this stream"""
    c = vs.case(name)
    want = oracle(name)[0]
    _set_env(A, monkeypatch, {"PACX_VQ_DEC_FRAME": mode})
    smallest = c.n_ch * (handle(A, c).payload_stride + 4)
    hop_bytes = (len(c.pac) - c.header_len) / max(c.hops, 1)
    chunks = [None] + sorted({smallest, max(smallest, int(1.5 * hop_bytes))})
    for chunk in chunks:
        if c.undefined.any():
            with pytest.raises(RuntimeError, match="PACX_ST_VQ_UNDEFINED"):
                A.pacfile.decode_stream(c.pac, chunk_bytes=chunk)
            continue
        got = A.pacfile.decode_stream(c.pac, chunk_bytes=chunk)
        assert got.dtype == np.int16 and got.shape == want.shape == ((c.hops + 1) * 1024, c.n_ch), chunk
        assert np.array_equal(got, want), (chunk, int(np.sum(got != want)))


def test_node_edge_routes_agree(A, monkeypatch, fresh_handles):
    """long blocks on both sides of the frame decoder's node store in one launch: the two routing modes give the same
    lines bit for bit, block by block (each is compared with the oracle in test_lines_of_every_block).  The API does
    not expose which route a block took, so none is inferred."""
    import torch
    c = vs.case("node_edge")
    outs = []
    for mode in MODES:
        _set_env(A, monkeypatch, {"PACX_VQ_DEC_FRAME": mode})
        enc = handle(A, c)
        offs = c.header_len + 4 + np.concatenate(([0], np.cumsum(c.sizes[:-1].astype(np.int64) + 4)))
        body = torch.frombuffer(bytearray(c.pac) + bytearray(8), dtype=torch.uint8).to(enc.device)
        out = enc.decode_vq(body, torch.as_tensor(c.sizes, device=enc.device), c.n_ch,
                            offsets=torch.as_tensor(offs, device=enc.device), want_lines=True, want_blocks=True)
        outs.append((out["lines"].cpu().numpy(), out["blocks"].cpu().numpy(), out["pcm"].cpu().numpy()))
    blocks_want = oracle("node_edge")[1]
    for i in range(len(c.flags)):
        assert np.array_equal(outs[0][0][i], outs[1][0][i]), i
        assert np.array_equal(outs[0][1][i], outs[1][1][i]), i
        peak = np.max(np.abs(blocks_want[i]))
        assert np.max(np.abs(outs[0][1][i] - blocks_want[i])) <= 1e-12 * peak > 0, i
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][2], oracle("node_edge")[0])


# ---------------------------------------------------------------------------------------------------- block API
@pytest.mark.parametrize("name", ["mixed", "sbr_partial"])
def test_block_api(A, tmp_path, name):
    """PACFile.OpenForReading / ReadDataBlock over the whole file, and PACFile.Decode (codec.Decode / Decode_SBR) called
    the way the reference's getDecodedBlock calls it -- flags, overall scale and allocations already read, `pb` a bit
    cursor at the first coded band -- on a long, a short and (sbr_partial) an SBR block, at the 1e-12 bar; the cursor
    ends where the oracle's reader ends"""
    c = vs.case(name)
    _, _, _, samples, peak, _ = oracle(name)
    path = tmp_path / (name + ".pac")
    path.write_bytes(c.pac)
    f = A.pacfile.PACFile(str(path))
    cp = f.OpenForReading()
    hops = []
    while True:
        data = f.ReadDataBlock(cp)
        if not data:
            break
        hops.append(np.stack(data, axis=1))
    f.fp.close()
    got = np.concatenate(hops)
    assert got.shape == samples.shape
    assert np.all(np.abs(got - samples) <= 1e-12 * peak), float(np.max(np.abs(got - samples)))

    class Cursor:                      # the reference's PackedBits, as far as Decode uses it
        def __init__(self, data):
            self.br = po.BitReader(data)

        def ReadBits(self, n):
            return self.br.get(n)

    cp, _ = A.pacfile.parse_header(c.pac)
    cp.omittedBands = A.pacfile.omitted_bands(cp.sfBands) if cp.useSBR else []
    p = c.p
    picks = [int(np.flatnonzero((c.flags & 2) == 0)[-1]), int(np.flatnonzero((c.flags & 2) == 2)[0])]
    picks += [cf for cf in range(len(c.flags)) if c.units[cf][0]["sbr"]][:1]
    seen = set()
    for cf in picks:
        blk = c.records[cf] + b"\0" * 8
        cur, ref = Cursor(blk), po.BitReader(blk)
        last_t, cur_t, next_t = (cur.ReadBits(1) for _ in range(3))
        ref.get(3)
        bands = cp.sfBandsShort if cur_t else cp.sfBands
        cp.nMDCTLines = 128 if cur_t else 1024
        p.nMDCTLines = p.nSamplesPerBlock = cp.nMDCTLines
        try:
            for _ in range(8 if cur_t else 1):
                with vs.model_leaves():
                    want = pv.decode_block_vq(ref, p, last_t, cur_t, next_t)
                overall = cur.ReadBits(cp.nScaleBits)
                alloc = []
                for b in range(bands.nBands):
                    a = cur.ReadBits(cp.nMantSizeBits)
                    alloc.append(a + 1 if a else 0)
                pf = A.pacfile.PACFile.__new__(A.pacfile.PACFile)
                got = pf.Decode(None, alloc, None, overall, cur, cp, last_t, cur_t, next_t)
                sbr = bool(cp.useSBR and not cur_t and np.any(np.array(alloc)[np.array(cp.omittedBands, dtype=int)] != 0))
                seen.add("sbr" if sbr else ("short" if cur_t else "long"))
                assert got.shape == want.shape
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)) > 0
                assert cur.br.pos == ref.pos           # the cursor ends where the oracle's reader ends
        finally:
            cp.nMDCTLines = 1024
            p.nMDCTLines = p.nSamplesPerBlock = 1024
    assert seen == ({"long", "short", "sbr"} if name == "sbr_partial" else {"long", "short"})
