"""The scalar decoders (k_unpack, k_imdct_long, k_imdct_short, k_ola_pcm / k_ola_tail_pcm) and the packer (k_pack) on the
hand-written code sets of tests/code_streams.py: records the format defines and no encode of real audio reaches -- 16-bit
mantissas in every band, every mix of allocations, scale factor and overall scale 15, sign-only mantissas, blocks far
above full scale, all eight flag triples, 96 kHz with its uncovered lines, an empty body, header widths other than 4 / 12.
Well-formed records only; the reference is the oracle's own reader and decoder on the same bytes.

Bars.  Codes, record bytes and sizes are integers: equal.  A block is within 1e-12 of its own peak of the oracle's (the
bar of tests/test_gpu_decode.py).  int16 PCM is equal sample for sample: tests/test_code_streams.py shows that no sample of
the oracle's output lies within a hundred times that bar of a step of the quantiser.

The handles are the package's cached ones, fetched anew in every test (other modules close and remake them), or made
and closed here."""
import functools

import numpy as np
import pytest

import code_streams as cs
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

CANARY = 0xC3


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(int16 PCM of oracle.decode_stream, blocks [n_cf, 2048], samples before the quantiser, peak per sample), once"""
    samples, peak, blocks = cs.decode_float(cs.case(name).pac)
    return po.fraction_to_pcm16(samples), blocks, samples, peak


def handle(A, c):
    """the handle pacfile.decode_stream uses for the case's header"""
    cp, pos = A.pacfile.parse_header(c.pac)
    assert pos == c.header_len
    enc = A.context.encoder_for_params(cp)
    assert enc.band_stride == c.band_stride and enc.payload_stride >= max(c.sizes, default=0)
    return enc


def device_codes(enc, c):
    import torch
    codes = {k: torch.as_tensor(getattr(c, k), device=enc.device)
             for k in ("flags", "overall", "scale_factor", "bit_alloc", "mantissa")}
    codes["status"] = torch.zeros(len(c.flags), dtype=torch.int32, device=enc.device)
    return codes


def check_codes(c, got, what):
    """Encoder.unpack's dict against the drawn codes: every field whole, status 0 everywhere"""
    for k in ("flags", "overall", "scale_factor", "bit_alloc", "mantissa"):
        have = got[k].cpu().numpy()
        want = getattr(c, k)
        assert have.shape == want.shape and have.dtype == want.dtype, (what, k)
        assert np.array_equal(have, want), (what, k, np.argwhere(have != want)[:4].tolist())
    assert not got["status"].cpu().numpy().any(), what


# ------------------------------------------------------------------------------------------------------ streams
@pytest.mark.parametrize("name", cs.NAMES)
def test_decode_stream(A, name):
    c = cs.case(name)
    want = oracle(name)[0]
    got = A.pacfile.decode_stream(c.pac)
    assert got.dtype == np.int16 and got.shape == want.shape == ((c.hops + 1) * 1024, c.n_ch)
    assert np.array_equal(got, want), int(np.sum(got != want))


@pytest.mark.parametrize("name", cs.NAMES)
def test_decode_stream_in_chunks(A, name):
    """the smallest chunk the streamed decoder takes (one hop of longest records) and one of about a hop and a half
    of this stream: records straddle the chunks and k_ola_tail_pcm carries the half-block across them"""
    c = cs.case(name)
    want = oracle(name)[0]
    smallest = c.n_ch * (handle(A, c).payload_stride + 4)
    hop_bytes = (len(c.pac) - c.header_len) / max(c.hops, 1)
    for chunk in sorted({smallest, max(smallest, int(1.5 * hop_bytes))}):
        got = A.pacfile.decode_stream(c.pac, chunk_bytes=chunk)
        assert got.dtype == np.int16 and got.shape == want.shape, chunk
        assert np.array_equal(got, want), (chunk, int(np.sum(got != want)))


# -------------------------------------------------------------------------------------------------------- codes
@pytest.mark.parametrize("name", cs.NAMES)
def test_unpack_gives_the_drawn_codes(A, name):
    import torch
    c = cs.case(name)
    enc = handle(A, c)
    n_cf = len(c.records)
    sizes = torch.as_tensor(c.sizes, device=enc.device)
    # slot layout; what follows a record in its slot is not the record's
    slots = np.full((n_cf, enc.payload_stride), 0xA5, np.uint8)
    for i, rec in enumerate(c.records):
        slots[i, :len(rec)] = np.frombuffer(rec, np.uint8)
    check_codes(c, enc.unpack(torch.as_tensor(slots, device=enc.device), sizes), "slots")
    # the file's bytes with offsets: payloads at every byte alignment
    offs = c.header_len + 4 + np.concatenate(([0], np.cumsum(c.sizes[:-1].astype(np.int64) + 4)))[:n_cf]
    body = torch.frombuffer(bytearray(c.pac) + bytearray(8), dtype=torch.uint8).to(enc.device)
    check_codes(c, enc.unpack(body, sizes, torch.as_tensor(offs.astype(np.int64), device=enc.device)), "stream")


@pytest.mark.parametrize("name", cs.NAMES)
def test_decode_of_the_codes(A, name):
    """Encoder.decode on the drawn codes: EVERY block within 1e-12 of its own peak of the oracle's (short frames
    assembled as oracle.decode_stream does), and the PCM of the same call"""
    c = cs.case(name)
    enc = handle(A, c)
    pcm_want, blocks_want = oracle(name)[:2]
    blocks, pcm = enc.decode(device_codes(enc, c), c.n_ch, want_blocks=True)
    blocks = blocks.cpu().numpy()
    assert blocks.shape == blocks_want.shape
    for i in range(len(blocks)):
        peak = np.max(np.abs(blocks_want[i]))
        err = np.max(np.abs(blocks[i] - blocks_want[i]))
        assert err <= 1e-12 * peak, (i, int(c.flags[i]), err, peak)
    assert np.array_equal(pcm.cpu().numpy(), pcm_want)


@pytest.mark.parametrize("name", cs.NAMES)
def test_pack_writes_the_oracles_records(A, name):
    import torch
    c = cs.case(name)
    enc = handle(A, c)
    n_cf, stride = len(c.records), enc.payload_stride
    codes = device_codes(enc, c)
    if c.frame_flags is not None:
        n_ch = c.n_ch
        codes["flags"] = torch.as_tensor(c.frame_flags, device=enc.device)
    else:
        n_ch = 1                              # flags differ within a hop: every channel-frame is its own frame
    out = {"payload": torch.full((n_cf, stride), CANARY, dtype=torch.uint8, device=enc.device),
           "n_bytes": torch.full((n_cf,), -1, dtype=torch.int32, device=enc.device)}
    payload, n_bytes = enc.pack(codes, n_ch, out)
    host, sizes = payload.cpu().numpy(), n_bytes.cpu().numpy()
    assert np.array_equal(sizes, c.sizes)
    for i, rec in enumerate(c.records):
        assert host[i, :len(rec)].tobytes() == rec, i
        written = 4 * ((len(rec) + 3) // 4)                 # the packer stores whole 32-bit words
        assert (host[i, written:] == CANARY).all(), (i, len(rec))
    body, total = enc.gather_body(payload, n_bytes)
    n = int(total.item())
    assert n == len(c.pac) - c.header_len and body[:n].cpu().numpy().tobytes() == c.pac[c.header_len:]


# ---------------------------------------------------------------------------------------------------- block API
def test_block_api_mixed(A, tmp_path):
    """PACFile.OpenForReading / ReadDataBlock over `mixed` (flags that differ between the channels of a hop), and
    codec.Decode on one long and one short block, against the oracle at the 1e-12 bar"""
    c = cs.case("mixed")
    _, _, samples, peak = oracle("mixed")
    path = tmp_path / "mixed.pac"
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

    p = po.make_params(c.sample_rate, 1, 128)
    one = A.audiofile.CodingParams()
    one.__dict__.update(A.pacfile.parse_header(c.pac)[0].__dict__)
    one.nChannels = 1
    cf_long, cf_short = (int(np.flatnonzero((c.flags & 2) == v)[0]) for v in (0, 2))
    fl = int(c.flags[cf_long])
    sf, alloc, _, overall = c.parts[cf_long][0]
    got = A.codec.Decode(sf, alloc, c.mantissa[cf_long], overall, None, one, fl & 1, 0, fl >> 2)
    want = po.decode_block(p, sf, alloc, c.mantissa[cf_long], overall, fl & 1, 0, fl >> 2)
    assert got.shape == (2048,) and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)) > 0
    fl = int(c.flags[cf_short])
    sub = 5
    sf, alloc, _, overall = c.parts[cf_short][sub]
    mant = c.mantissa[cf_short, sub * 128:(sub + 1) * 128]
    one.nMDCTLines = one.nSamplesPerBlock = p.nMDCTLines = p.nSamplesPerBlock = 128
    got = A.codec.Decode(sf, alloc, mant, overall, None, one, fl & 1, 1, fl >> 2)
    want = po.decode_block(p, sf, alloc, mant, overall, fl & 1, 1, fl >> 2)
    assert got.shape == (256,) and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)) > 0


# ------------------------------------------------------------------------------------------- the slot's capacity
def test_create_refuses_widths_whose_longest_record_overruns_the_slot(A):
    """16-bit size fields: 20 header bits per band.  At 32 kHz (7 short bands) an all-16-bit short frame takes 2193
    bytes, one more than a payload slot and than the packers' LDS array: pacx_create refuses the handle, nothing is
    launched on it.  At 48 kHz (6 short bands, 2173 bytes) the same widths give a handle, and `w4_16` runs on it."""
    import torch
    with pytest.raises(A._lib.PacxError, match=r"pacx_create failed \(-2\).*2193 bytes") as e:
        A.engine.Encoder(32000, 128 / 32.0, n_scale_bits=4, n_mant_size_bits=16)
    assert A._lib.E_UNSUPPORTED == -2 and "2192" in str(e.value)
    assert cs.longest_record(32000, (4, 16), True) == 2193
    enc = A.engine.Encoder(48000, 128 / 48.0, n_scale_bits=4, n_mant_size_bits=16)
    try:
        c = cs.case("w4_16")
        assert enc.payload_stride == 2192 >= max(c.sizes) == 2173 == cs.longest_record(48000, (4, 16), True)
        body = torch.frombuffer(bytearray(c.pac) + bytearray(8), dtype=torch.uint8).to(enc.device)
        offs = c.header_len + 4 + np.concatenate(([0], np.cumsum(c.sizes[:-1].astype(np.int64) + 4)))
        got = enc.unpack(body, torch.as_tensor(c.sizes, device=enc.device), torch.as_tensor(offs, device=enc.device))
        check_codes(c, got, "w4_16")
        pcm = enc.decode(got, c.n_ch).cpu().numpy()
        assert np.array_equal(pcm, oracle("w4_16")[0])
    finally:
        enc.close()
