"""The hand-written code sets of tests/code_streams.py on the CPU: the oracle's reader gives back the drawn codes, its
decoder takes every case, the census the cases promise holds, the table of longest records is what the format's
arithmetic gives, and no sample of the oracle's output sits near enough to a step of the PCM quantiser for the IMDCT's
rounding on the GPU to flip a code (tests/test_gpu_code_streams.py compares int16 PCM sample for sample)."""
import os
import re
import struct

import numpy as np
import pytest

import code_streams as cs
from conftest import ROOT
from oracle import pac_oracle as po


@pytest.fixture(scope="module")
def floats():
    """decode_float of every case, once"""
    return {name: cs.decode_float(cs.case(name).pac) for name in cs.NAMES}


def payload_stride():
    text = open(os.path.join(ROOT, "audio-codec_amd", "csrc", "pacx_dev.h")).read()
    return int(re.search(r"#define PACX_PAYLOAD_STRIDE (\d+)", text).group(1))


@pytest.mark.parametrize("name", cs.NAMES)
def test_oracle_reads_back_the_drawn_codes(name):
    c = cs.case(name)
    p = c.p
    n_cf = c.hops * c.n_ch
    assert len(c.records) == n_cf == len(c.flags) and c.sizes.tolist() == [len(r) for r in c.records]
    assert c.overall.shape == (n_cf, 8) and c.mantissa.shape == (n_cf, 1024)
    assert c.scale_factor.shape == c.bit_alloc.shape == (n_cf, c.band_stride)
    assert c.band_stride == max(p.sfBands.nBands, 8 * p.sfBandsShort.nBands)
    # the file: the oracle's header, then '<L nBytes' + payload per channel-frame
    q, _, pos = po.parse_header(c.pac)
    assert pos == c.header_len and (q.sampleRate, q.nChannels, q.nScaleBits, q.nMantSizeBits) == \
        (c.sample_rate, c.n_ch) + c.widths
    assert c.pac[pos:] == b"".join(struct.pack("<L", len(r)) + r for r in c.records)
    top = cs.max_alloc(c.widths[1])
    for cf, rec in enumerate(c.records):
        br = po.BitReader(rec)
        fl = br.get(1) | br.get(1) << 1 | br.get(1) << 2
        assert fl == c.flags[cf]
        cur = (fl >> 1) & 1
        bands = p.sfBandsShort if cur else p.sfBands
        nb, n_lines = bands.nBands, (128 if cur else 1024)
        p.nMDCTLines = n_lines
        try:
            units = [po.parse_block_body(br, p, bool(cur)) for _ in range(8 if cur else 1)]
        finally:
            p.nMDCTLines = 1024
        assert len(rec) == (br.pos + 1 + 7) // 8           # the size rule: 3 flag bits + body + 1, rounded up
        for s, (sf, alloc, mant, overall) in enumerate(units):
            assert overall == c.overall[cf, s] < 1 << c.widths[0]
            assert list(sf) == c.scale_factor[cf, s * nb:(s + 1) * nb].tolist() and max(sf) < 1 << c.widths[0]
            assert list(alloc) == c.bit_alloc[cf, s * nb:(s + 1) * nb].tolist()
            assert all(a == 0 or 2 <= a <= top for a in alloc)
            assert np.array_equal(mant, c.mantissa[cf, s * n_lines:(s + 1) * n_lines])
        used = len(units) * nb
        assert not c.overall[cf, len(units):].any() and not c.scale_factor[cf, used:].any() and \
            not c.bit_alloc[cf, used:].any()
    if c.frame_flags is not None:
        assert np.array_equal(np.repeat(c.frame_flags, c.n_ch), c.flags)


@pytest.mark.parametrize("name", cs.NAMES)
def test_oracle_decodes_every_case(name, floats):
    """oracle.decode_stream takes the file, and decode_float is that decoder up to the PCM conversion"""
    c = cs.case(name)
    want = po.decode_stream(c.pac)
    samples, peak, blocks = floats[name]
    assert want.dtype == np.int16 and want.shape == ((c.hops + 1) * 1024, c.n_ch) == samples.shape == peak.shape
    assert np.array_equal(po.fraction_to_pcm16(samples), want)
    assert blocks.shape == (c.hops * c.n_ch, 2048)
    b = blocks.reshape(c.hops, c.n_ch, 2048)
    pk = np.max(np.abs(b), axis=2) if c.hops else np.zeros((0, c.n_ch))
    for h in range(c.hops + 1):
        both = np.maximum(pk[h - 1] if h else 0.0, pk[h] if h < c.hops else 0.0)
        assert np.array_equal(peak[h * 1024:(h + 1) * 1024], np.broadcast_to(both, (1024, c.n_ch)))
        got = (b[h - 1, :, 1024:] if h else 0.0) + (b[h, :, :1024] if h < c.hops else 0.0)
        assert np.array_equal(samples[h * 1024:(h + 1) * 1024], np.broadcast_to(np.transpose(got), (1024, c.n_ch)))


def coded_bands(c):
    """(allocation, the band's mantissas) of every coded band of every block of a case"""
    for parts in c.parts:
        bands = c.p.sfBandsShort if len(parts) == 8 else c.p.sfBands
        for (_, alloc, mant, _) in parts:
            at = 0
            for b in np.flatnonzero(alloc):
                yield int(alloc[b]), np.asarray(mant[at:at + bands.nLines[b]])
                at += bands.nLines[b]
            assert at == len(mant)


def test_census(floats):
    mixed, flags8 = cs.case("mixed"), cs.case("flags8")
    assert (mixed.hops, mixed.n_ch) == (6, 2) and (flags8.hops, flags8.n_ch) == (8, 1)
    assert mixed.frame_flags is None                        # flags drawn per hop AND per channel
    assert flags8.flags.tolist() == list(range(8))          # the eight triples in order
    both = {k: v | cs.census(flags8)[k] for k, v in cs.census(mixed).items()}
    assert both["alloc"] == {0} | set(range(2, 17))
    assert both["scale_factor"] == set(range(16)) == both["overall"]
    assert both["flags"] == set(range(8))
    assert cs.census(mixed)["mod4"] == {0, 1, 2, 3}         # payloads start at every byte alignment of the file
    starts = mixed.header_len + 4 + np.concatenate(([0], np.cumsum(mixed.sizes[:-1] + 4)))
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}

    for name in ("max_long", "max_short", "max_long_sr32", "max_short_sr32"):
        c = cs.case(name)
        assert (c.hops, c.n_ch) == (3, 1) and cs.census(c)["alloc"] == {16}
        assert set(c.sizes.tolist()) == {cs.longest_record(c.sample_rate, c.widths, "short" in name)}
    assert cs.census(cs.case("empty_blocks"))["alloc"] == {0}
    c = cs.case("empty_one_band")
    assert [int(np.sum(r)) for r in c.bit_alloc] == [2] * len(c.bit_alloc)     # one band at 2 bits in every record
    assert min(cs.case("empty_blocks").sizes) == (3 + 4 + 17 * 16 + 1 + 7) // 8    # the shortest record at 48 kHz
    for name in ("empty_blocks", "empty_one_band", "sign_only", "loud", "quiet"):
        assert {0, 2} <= set(int(f) & 2 for f in cs.case(name).flags), name         # long and short blocks

    for a, mant in coded_bands(cs.case("sign_only")):
        assert (mant == 1 << (a - 1)).all()                 # the sign bit and nothing else
    assert not floats["sign_only"][0].any()                 # every line is -0.0: silence

    c = cs.case("loud")
    got = cs.census(c)
    assert got["overall"] == {0} == got["scale_factor"] and 0 not in got["alloc"]
    signs = set()
    for a, mant in coded_bands(c):
        assert (mant & ((1 << (a - 1)) - 1) == (1 << (a - 1)) - 1).all()      # full magnitude
        signs |= set((mant >> (a - 1)).tolist())
    assert signs == {0, 1}
    pcm = po.fraction_to_pcm16(floats["loud"][0])
    assert pcm.max() == 32767 and pcm.min() == -32767
    assert np.mean(np.abs(floats["loud"][0]) >= 1.0) >= 0.1 and np.mean(np.abs(pcm.astype(int)) == 32767) >= 0.1

    got = cs.census(cs.case("quiet"))
    assert got["overall"] == {15} == got["scale_factor"] and got["alloc"] == {2}

    assert (cs.case("ch1").n_ch, cs.case("ch3").n_ch) == (1, 3) and cs.case("ch1").hops == cs.case("ch3").hops == 3
    assert cs.case("one_hop").hops == 1 and len(cs.case("one_hop").records) == 2
    assert cs.case("no_hops").hops == 0 and len(cs.case("no_hops").pac) == cs.case("no_hops").header_len
    for name, sr, nb in (("sr32", 32000, 20), ("sr441", 44100, 18), ("sr96", 96000, 13)):
        c = cs.case(name)
        assert c.sample_rate == sr and c.p.sfBands.nBands == nb
        assert struct.unpack("<L", c.pac[26:30])[0] == nb    # the long layout travels in the header
    c = cs.case("sr96")
    assert c.p.sfBands.upperLine[-1] == 511 and not c.mantissa[:, 512:][(c.flags & 2) == 0].any()
    assert any(c.mantissa[cf, :512].any() for cf in range(len(c.flags)) if not c.flags[cf] & 2)
    for name, widths in (("w3_4", (3, 4)), ("w2_5", (2, 5)), ("w4_16", (4, 16))):
        c = cs.case(name)
        assert c.widths == widths and c.hops == 4 and c.sample_rate == 48000
        assert struct.unpack("<HH", c.pac[18:22]) == widths
        got = cs.census(c)
        assert max(got["alloc"]) == 16 and max(got["scale_factor"]) == (1 << widths[0]) - 1 == max(got["overall"])
    assert max(cs.case("w4_16").sizes) == 2173 == cs.longest_record(48000, (4, 16), True)


def test_allocation_limit_of_narrow_size_fields():
    """a size field of n bits carries code + 1 up to 2^n, never more than 16"""
    assert [cs.max_alloc(n) for n in (1, 2, 3, 4, 5, 12, 16)] == [2, 4, 8, 16, 16, 16, 16]


# (long, short) bytes of the record with every band at the largest allocation: oracle.block_bits and the size rule
LONGEST = {
    (24000, (4, 12)): (2089, 2181), (32000, (4, 12)): (2089, 2165), (44100, (4, 12)): (2085, 2149),
    (48000, (4, 12)): (2083, 2149), (96000, (4, 12)): (1051, 1077),
    (24000, (4, 16)): (2099, 2213), (32000, (4, 16)): (2099, 2193), (44100, (4, 16)): (2094, 2173),
    (48000, (4, 16)): (2092, 2173), (96000, (4, 16)): (1058, 1089),
    (48000, (3, 4)): (2064, 2094), (48000, (2, 5)): (2064, 2093),
}


def test_longest_record_table():
    for (sr, widths), want in LONGEST.items():
        assert (cs.longest_record(sr, widths, False), cs.longest_record(sr, widths, True)) == want, (sr, widths)
    p32, p24 = po.make_params(32000, 1, 128), po.make_params(24000, 1, 128)
    assert (p32.sfBands.nBands, p32.sfBandsShort.nBands) == (20, 7) and p24.sfBandsShort.nBands == 8
    # what a payload slot holds: everything at the reference's widths 4 / 12 (the longest is 24 kHz's short frame),
    # the narrow widths of the cases, and 16-bit size fields down to 44.1 kHz -- but not at 32 and 24 kHz, where
    # pacx_create refuses the handle
    slot = payload_stride()
    assert slot == 2192
    fits = {k: max(v) <= slot for k, v in LONGEST.items()}
    assert max(max(v) for (sr, w), v in LONGEST.items() if w == (4, 12)) == 2181
    assert [k for k, ok in fits.items() if not ok] == [(24000, (4, 16)), (32000, (4, 16))]
    assert LONGEST[(24000, (4, 16))][1] == 2213 and LONGEST[(32000, (4, 16))][1] == 2193


@pytest.mark.parametrize("name", cs.NAMES)
def test_no_sample_near_a_quantiser_step(name, floats):
    """Tie condition.  The GPU's samples may differ from the oracle's by 1e-12 of the block peak; with a window of
    1e-10 * max(1, peak), a hundred times that, x + w and x - w map to the same int16 code for EVERY sample."""
    samples, peak, _ = floats[name]
    assert cs.tie_exceptions(samples, peak) == 0
    assert cs.SEEDS[name] == cs.case(name).seed
