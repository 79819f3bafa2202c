"""The drawn gain-shape streams of tests/vq_code_streams.py on the CPU, before anything runs on a GPU: the oracle's
reader gives back the drawn header codes and ends every band exactly where its allocation says, its decoder takes every
case, every case reaches what its name says (the census, zero exceptions), no gain is wider than the decoders take, the
longest gain-shape record fits a payload slot, the seeds are the first that satisfy the tie condition, and the oracle
with pvq_model's leaves gives the PCM the REFERENCE's own decoder made of four of the streams
(tests/golden/vq_code_streams.npz, written by tests/golden/make_vq_code_streams.py)."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import pvq_model as pm
import vq_code_streams as vs
from conftest import GOLDEN, ROOT
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv


@pytest.fixture(scope="module")
def floats():
    """decode_float_vq of every case, once"""
    return {name: vs.decode_float_vq(vs.case(name).pac) for name in vs.NAMES}


def payload_stride():
    text = open(os.path.join(ROOT, "audio-codec_amd", "csrc", "pacx_dev.h")).read()
    return int(re.search(r"#define PACX_PAYLOAD_STRIDE (\d+)", text).group(1))


def nodes(c, kind):
    return [nd for _, _, _, nd in vs.nodes_of(c, kind)]


@pytest.mark.parametrize("name", vs.NAMES)
def test_oracle_reads_back_the_drawn_codes(name, floats):
    """header codes, and the reader's position: after every band alloc * lines bits further (an omitted band of an SBR
    block counts one line), at the end of the record the sum of its fields"""
    c = vs.case(name)
    p = c.p
    n_cf = c.hops * c.n_ch
    infos = floats[name][4]
    assert len(c.records) == n_cf == len(c.flags) == len(infos) and c.sizes.tolist() == [len(r) for r in c.records]
    assert c.overall.shape == (n_cf, 8) and c.bit_alloc.shape == (n_cf, c.band_stride)
    assert c.band_stride == max(p.sfBands.nBands, 8 * p.sfBandsShort.nBands)
    head = struct.unpack("<LHLLHHHH", c.pac[4:26])
    assert (head[0], head[1], head[4], head[5], head[6], head[7]) == (c.sample_rate, c.n_ch) + c.widths + \
        (int(c.use_sbr), 1)
    assert c.pac[c.header_len:] == b"".join(struct.pack("<L", len(r)) + r for r in c.records)
    top = vs.max_alloc(c.widths[1])
    for cf, info in enumerate(infos):
        fl = int(c.flags[cf])
        assert c.records[cf][0] >> 5 == (fl & 1) << 2 | (fl & 2) | (fl >> 2)          # MSB first: last, cur, next
        cur = (fl >> 1) & 1
        bands = p.sfBandsShort if cur else p.sfBands
        nb = bands.nBands
        units = info["units"]
        assert len(units) == (8 if cur else 1) == len(c.units[cf])
        bits = 3
        size_rule = 4
        for s, u in enumerate(units):
            assert u["overall"] == c.overall[cf, s] < 1 << c.widths[0]
            assert u["alloc"] == c.bit_alloc[cf, s * nb:(s + 1) * nb].tolist() == list(c.units[cf][s]["alloc"])
            assert all(a == 0 or 2 <= a <= top for a in u["alloc"])
            assert u["sbr"] == c.units[cf][s]["sbr"]
            assert [(b, want, want) for (b, want, _) in u["ends"]] == u["ends"]      # every band: read == alloc * lines
            assert [b for (b, _, _) in u["ends"]] == [b for (b, _, _) in c.units[cf][s]["bands"]]
            assert [w for (_, w, _) in u["ends"]] == [int(u["alloc"][b]) * n for (b, n, _) in c.units[cf][s]["bands"]]
            bits += c.widths[0] + nb * c.widths[1] + sum(w for (_, w, _) in u["ends"])
            size_rule += pv.block_bits_vq(p, u["alloc"], bool(cur))
        assert info["end_bit"] == bits
        assert info["n_bytes"] == (size_rule + 7) // 8 >= (bits + 7) // 8
        assert not c.overall[cf, len(units):].any() and not c.bit_alloc[cf, len(units) * nb:].any()


@pytest.mark.parametrize("name", vs.NAMES)
def test_oracle_decodes_every_case(name, floats):
    """oracle.decode_stream_vq (with the model's leaves) takes the file, and decode_float_vq is that decoder up to the
    PCM conversion"""
    c = vs.case(name)
    want = vs.decode_stream_vq(c.pac)
    samples, peak, blocks, lines, _ = floats[name]
    assert want.dtype == np.int16 and want.shape == ((c.hops + 1) * 1024, c.n_ch) == samples.shape == peak.shape
    assert np.array_equal(po.fraction_to_pcm16(samples), want)
    assert blocks.shape == (c.hops * c.n_ch, 2048) and lines.shape == (c.hops * c.n_ch, 1024)
    assert np.isfinite(samples).all() and np.isfinite(lines).all()
    b = blocks.reshape(c.hops, c.n_ch, 2048)
    for h in range(c.hops + 1):
        got = (b[h - 1, :, 1024:] if h else 0.0) + (b[h, :, :1024] if h < c.hops else 0.0)
        assert np.array_equal(samples[h * 1024:(h + 1) * 1024], np.broadcast_to(np.transpose(got), (1024, c.n_ch)))


@pytest.mark.parametrize("name", vs.NAMES)
def test_no_sample_near_a_quantiser_step(name, floats):
    """Tie condition, for the reference output alone: with a window of 1e-10 * max(1, peak), a hundred times the bar of
    the lines, x + w and x - w map to the same int16 code for EVERY sample"""
    samples, peak = floats[name][:2]
    assert vs.tie_exceptions(samples, peak) == 0
    assert vs.SEEDS[name] == vs.case(name).seed


@pytest.mark.parametrize("name", vs.NAMES)
def test_seed_is_the_first_clean_one(name):
    assert vs.find_seed(name) == vs.SEEDS[name]


# ------------------------------------------------------------------------------------------------------- census
@pytest.mark.parametrize("name", vs.NAMES)
def test_no_angle_on_a_rounding_edge(name):
    """no split's bit share hangs on the last place of log2(tan()): the argument of mid_side_alloc's floor() keeps
    1e-9 from every whole number (an ulp of it is some 1e-13), so a decoder with another maths library shares the bits
    alike"""
    assert vs.census(vs.case(name))["floor_margin"] >= 1e-9


def test_census_layouts_and_allocations():
    mixed = vs.case("mixed")
    got = vs.census(mixed)
    assert (mixed.hops, mixed.n_ch) == (6, 2)
    assert got["flags"] == set(range(8))                                   # all eight flag triples
    assert any(mixed.flags[2 * h] != mixed.flags[2 * h + 1] for h in range(6))     # differing within a hop
    assert got["alloc"] == {0} | set(range(2, 17)) and got["mod4"] == {0, 1, 2, 3}
    assert got["gain_negative"] > 50 and got["k0_leaves"] > 0 and got["zero_children"] > 0

    slot = payload_stride()
    for name in ("max_long", "max_short", "max_long_sr32", "max_short_sr32"):
        c = vs.case(name)
        got = vs.census(c)
        assert got["alloc"] == {16} and c.sample_rate == (32000 if "sr32" in name else 48000)
        assert all(bool(f & 2) == ("short" in name) for f in c.flags)
        assert set(c.sizes.tolist()) == {vs.longest_record_vq(c.sample_rate, c.widths, "short" in name)}
    # at the widths 4 / 12 the longest gain-shape record fits the slot at every rate the decoders take
    longest = {sr: (vs.longest_record_vq(sr), vs.longest_record_vq(sr, short=True)) for sr in (32000, 44100, 48000)}
    assert longest == {32000: (2089, 2165), 44100: (2085, 2149), 48000: (2083, 2149)}
    assert max(max(v) for v in longest.values()) <= slot == 2192

    c = vs.case("low_long")
    got = vs.census(c)
    assert got["alloc"] == {2, 3} and not (c.flags & 2).any()
    assert got["k0_leaves"] >= 5 and got["zero_children"] >= 10

    assert (vs.case("ch1").n_ch, vs.case("ch3").n_ch) == (1, 3) and vs.case("ch1").hops == vs.case("ch3").hops == 3
    assert vs.case("one_hop").hops == 1 and len(vs.case("one_hop").records) == 2
    assert vs.case("no_hops").hops == 0 and len(vs.case("no_hops").pac) == vs.case("no_hops").header_len
    for name in ("ch1", "ch3"):
        assert {0, 2} <= set(int(f) & 2 for f in vs.case(name).flags)
    c = vs.case("w3_4")
    assert c.widths == (3, 4) and struct.unpack("<HH", c.pac[18:22]) == (3, 4)
    got = vs.census(c)
    assert max(got["alloc"]) == 16 and max(got["overall"]) == 7                    # allocation 16 through code 15


def test_both_sides_of_the_frame_decoders_store():
    """k_vq_dec_frame takes a channel-frame of at most NODE_CAP nodes and BUF_CAP buffer doubles, k_vq_dec the rest
    (and every frame with PACX_VQ_DEC_FRAME=0).  Outside the HEAVY recipes every light frame fits, there are long and
    short ones among them, and in the BOTH_SIDES recipes every frame drawn freely lies beyond -- so the default run of
    the GPU tests decodes each case's edges with the frame decoder AND the band decoder.  The counts are the kernel's:
    a node per split, leaf and half without bits; pow2ceil(lines) doubles per band with a shape."""
    assert (vs.NODE_CAP, vs.BUF_CAP) == (304, 1536)
    text = open(os.path.join(ROOT, "audio-codec_amd", "csrc", "k_vq_dec.hip")).read()
    assert re.search(r"#define VQDF_NCAP (\d+)", text).group(1) == "304"
    assert re.search(r"#define VQDF_BUF (\d+)", text).group(1) == "1536"
    for name in vs.NAMES:
        c = vs.case(name)
        recipe = vs.SPECS[name][5]
        for cf, units in enumerate(c.units):
            assert c.n_nodes[cf] == sum(len(nd) - 1 for u in units for (_, _, nd) in u["bands"])
            assert c.buf[cf] == sum(1 << (n - 1).bit_length() for u in units for (_, n, nd) in u["bands"] if len(nd) > 1)
        assert c.fits.tolist() == [bool(n <= 304 and b <= 1536) for n, b in zip(c.n_nodes, c.buf)]
        assert max(c.buf, default=0) <= 1536, name                 # at these layouts the node store alone decides
        fit, beyond = vs.sides(c)
        if recipe in vs.HEAVY or not len(c.flags):
            assert not c.light.any()
            continue
        assert c.light.any() and c.fits[c.light].all(), name
        if c.hops >= 2:
            assert {0, 2} <= set(int(c.flags[cf]) & 2 for cf in fit), name
        if recipe in vs.BOTH_SIDES:
            assert not c.fits[~c.light].any() and beyond, name
            if c.hops >= 2 and c.n_ch > 1:
                assert {0, 2} <= set(int(c.flags[cf]) & 2 for cf in beyond), name
    # the frames at one allocation: low_long fits, every band at 16 does not
    assert vs.case("low_long").fits.all()
    for name in ("max_long", "max_short", "max_long_sr32", "max_short_sr32"):
        assert not vs.case(name).fits.any() and min(vs.case(name).n_nodes) > 700


def test_census_node_edge():
    """one allocation for all bands of a long block, 2..16 in turn: the blocks lie on both sides of the frame decoder's
    store of 304 nodes, and the hops of three channels mix them"""
    c = vs.case("node_edge")
    assert (c.hops, c.n_ch) == (6, 3)
    assert sorted(vs.NODE_EDGE_ROW) == list(range(2, 17))
    for cf in range(15):
        assert not c.flags[cf] & 2 and set(c.bit_alloc[cf, :17].tolist()) == {vs.NODE_EDGE_ROW[cf]}
    assert c.flags[16] & 2 and set(c.bit_alloc[15, :17].tolist()) == {2} and set(c.bit_alloc[17, :17].tolist()) == {3}
    count = c.n_nodes.tolist()
    by_alloc = [count[vs.NODE_EDGE_ROW.index(a)] for a in range(2, 17)]
    assert by_alloc == sorted(by_alloc) and by_alloc[0] < 200 and by_alloc[2] < 304 < by_alloc[4] and by_alloc[14] > 700
    for h in range(2):
        assert min(count[3 * h:3 * h + 3]) < 304 < max(count[3 * h:3 * h + 3])     # hops 0, 1 hold blocks of either side
    assert count[15] < 200 and count[17] < 250 and c.fits[15] and c.fits[17]       # beside the last hop's short frame
    assert c.fits[:15].tolist() == [a <= 4 for a in vs.NODE_EDGE_ROW]


def test_census_angles():
    for name in ("theta_zero", "theta_wide"):
        c = vs.case(name)
        splits = nodes(c, "split")
        assert len(splits) > 50 and all(nd[5] == 0 and nd[6] == 0 for nd in splits)          # index 0: mid gets 0 bits
        assert vs.census(c)["zero_children"] >= len(splits)
    c = vs.case("theta_zero")
    assert max(vs.census(c)["theta_bits"]) <= vs.THETA_LIMIT and not c.undefined.any()
    assert {0, 2} <= set(int(f) & 2 for f in c.flags)

    c = vs.case("theta_wide")
    wide = [nd for nd in nodes(c, "split") if nd[4] > vs.THETA_LIMIT]
    assert len(wide) >= 4 and c.undefined.tolist() == [not f & 2 for f in c.flags] and 0 < c.undefined.sum() < len(c.flags)

    c = vs.case("theta_max")
    splits = nodes(c, "split")
    assert all(nd[5] & ((1 << (nd[4] - 1)) - 1) == (1 << (nd[4] - 1)) - 1 for nd in splits)  # the largest magnitude
    assert set(nd[5] >> (nd[4] - 1) for nd in splits) == {0, 1}                              # either sign bit
    clamped = [nd for nd in splits if nd[6] == 0 and nd[7] > 0]
    assert len(clamped) > 50                                               # the tan clamp: nothing left for mid

    # either rule on both kernels: frames that fit hold them too
    for name in ("theta_zero", "theta_max"):
        c = vs.case(name)
        fit = vs.sides(c)[0]
        assert len([nd for _, _, _, nd in vs.nodes_of(c, "split", fit)]) > 50, name
        assert {0, 2} <= set(int(c.flags[cf]) & 2 for cf in fit), name

    c = vs.case("theta_32_33")
    for side in vs.sides(c):
        got = vs.searched(vs.census(c, side))
        assert set(got) == {"mid 32", "mid 33", "side 32", "side 33", "side 0"} and min(got.values()) >= 2, got
    assert min(vs.searched(vs.census(c)).values()) >= 5
    # a 2-line node with more than 32 bits: the angle takes all of them, both halves are zeros, the oracle decodes a
    # zero vector (and so do the kernels: the lines of these frames are compared like all others)
    two = [nd for nd in nodes(c, "split") if nd[2] == 2]
    assert len(two) == vs.census(c)["all_angle_nodes"] >= 3
    assert all(nd[3] > 32 and nd[4] == nd[3] and nd[6] == nd[7] == 0 for nd in two)
    assert vs.census(c, vs.sides(c)[0])["all_angle_nodes"] >= 1


def test_census_leaves():
    c = vs.case("leaf_edges")
    leaves = [nd for nd in nodes(c, "leaf") if nd[4] > 0]
    got = vs.leaf_kinds(c)
    assert all(v >= 50 for v in got.values()), got
    for side in vs.sides(c):                                       # and each of them on either side of the node store
        got = vs.leaf_kinds(c, side)
        assert len(got) == 7 and all(v >= 10 for v in got.values()), got
        for table in (0, 2):
            part = [cf for cf in side if c.flags[cf] & 2 == table]
            assert all(v >= 2 for v in vs.leaf_kinds(c, part).values()), (table, vs.leaf_kinds(c, part))
    assert vs.census(c)["k0_leaves"] + len(leaves) == len(nodes(c, "leaf"))
    # paired bottom leaves (both children of a split small leaves of <= 32 lines) and lone ones
    splits = nodes(c, "split")
    paired = sum(1 for nd in splits if 0 < nd[6] <= 32 and 0 < nd[7] <= 32 and 2 <= -(-nd[2] // 2) <= 32)
    lone = sum(1 for nd in splits if (0 < nd[6] <= 32) != (0 < nd[7] <= 32))
    assert paired > 50 and lone > 20

    top = {2: 1 << 30, 3: 32767, 4: 1172}
    assert top == {l: pm.pulses_for_bits(l, 32)[0] for l in (2, 3, 4)}
    for name in ("tiny_leaves", "tiny_leaves_sr32"):
        c = vs.case(name)
        seen = {}
        for cf, _, _, nd in vs.nodes_of(c, "leaf"):
            if nd[2] <= 4 and nd[4] == top[nd[2]]:
                assert nd[5] == 32
                table = "short" if c.flags[cf] & 2 else "long"
                seen.setdefault((nd[2], table), []).append((nd[6], nd[7]))
        # leaves of 2, 3 and 4 lines with the largest K their 32 bits allow, under the long and the short band table
        assert set(seen) == {(l, t) for l in (2, 3, 4) for t in ("long", "short")}, (name, sorted(seen))
        for l in (2, 3, 4):
            both = seen[(l, "long")] + seen[(l, "short")]
            assert len(both) >= 8, (name, l)
            assert any(i == 0 for i, _ in both) and any(i == n - 1 for i, n in both), (name, l)
            assert any(n // 4 < i < 3 * (n // 4) for i, n in both), (name, l)      # and indices over the whole codebook
        # all of it in frames the frame decoder takes
        fit = vs.census(c, vs.sides(c)[0])
        assert len(fit["full_tiny_tables"]) == 6 and len(fit["tiny_ends"]) == 6, name
    assert vs.case("tiny_leaves_sr32").sample_rate == 32000


def test_census_gains():
    c = vs.case("gain_edges")
    kinds = {0: [], 1: []}
    for cf, _, _, nd in vs.nodes_of(c, "gain"):
        kinds[(cf // c.n_ch) % 2].append(nd)
    assert len(kinds[0]) > 50 and all(nd[3] >> (nd[2] - 1) == 1 for nd in kinds[0])          # the sign bit on every gain
    zeros = sum(1 for nd in kinds[1] if nd[3] == 0)
    ones = sum(1 for nd in kinds[1] if nd[3] == (1 << nd[2]) - 1)
    assert zeros + ones == len(kinds[1]) and zeros > 30 and ones > 30
    assert {0, 2} <= set(int(f) & 2 for f in c.flags)
    for side in vs.sides(c):                                       # on either side of the node store, long and short
        for table in (0, 2):
            neg = vs.census(c, [cf for cf in side if (cf // c.n_ch) % 2 == 0 and c.flags[cf] & 2 == table])
            alt = vs.census(c, [cf for cf in side if (cf // c.n_ch) % 2 == 1 and c.flags[cf] & 2 == table])
            assert neg["gains"] == neg["gain_negative"] >= 5, (table, neg["gains"])
            assert alt["gain_zero"] >= 3 and alt["gain_ones"] >= 3 and alt["gain_zero"] + alt["gain_ones"] == alt["gains"]
    # widths over ALL cases.  No well-formed record has a gain of 0 bits: a coded band has alloc >= 2, and
    # gain_shape_alloc gives its gain floor(alloc + log2(lines) / 2) >= 2 bits before the shape's unused bits are added
    # (the decoders' clamp of bits_gain to 0 is unreachable); none is wider than the decoders' 64
    widths = set()
    for name in vs.NAMES:
        widths |= vs.census(vs.case(name))["gain_bits"]
    assert min(widths) == 2 and max(widths) == 23 <= vs.GAIN_LIMIT, (min(widths), max(widths))


def test_census_odd_bands():
    c = vs.case("odd_bands")
    got = vs.census(c)
    assert got["split_depths_odd"] >= set(range(6)), got["split_depths_odd"]       # the padded left half at every depth
    longs = [cf for cf in range(len(c.flags)) if not c.flags[cf] & 2 and not c.light[cf]]
    assert longs and all(c.bit_alloc[cf, 16] == 16 for cf in longs) and c.p.sfBands.nLines[16] == 363
    assert any(nd[2] == 363 and nd[3] > 5700 for nd in nodes(c, "split"))
    assert {0, 2} <= set(int(f) & 2 for f in c.flags)
    fit, beyond = vs.sides(c)
    assert vs.census(c, fit)["split_depths_odd"] >= set(range(5)) and vs.census(c, beyond)["split_depths_odd"] >= set(range(6))


def test_census_sbr(floats):
    cut = {"sbr_sr441": 557, "sbr_sr32": 608}
    env_counts = set()
    for name in vs.NAMES:
        if not name.startswith("sbr_"):
            continue
        c = vs.case(name)
        om = c.p.omittedBands
        assert c.use_sbr and (c.flags & 2).tolist() == [0, 0, 2, 2, 0, 0]              # short frames between the SBR blocks
        assert c.p.sfBands.lowerLine[om[0]] == cut.get(name, 512)
        plan = vs.SBR_PLANS[vs.SPECS[name][5]]
        infos = floats[name][4]
        lines = floats[name][3]
        for k, cf in enumerate((0, 1, 4, 5)):
            subset, rule, low = plan[k]
            u = c.units[cf][0]
            coded = [b for b in om if u["alloc"][b]]
            assert u["sbr"] == bool(coded) == infos[cf]["units"][0]["sbr"]
            if subset != "some":
                assert coded == {"first": om[:1], "last": om[-1:], "all": om, "none": []}[subset]
            if low == "empty":
                assert not np.any(u["alloc"][:om[0]]) and not lines[cf, :512].any()
            gains = [nodes_[-1] for (b, n, nodes_) in u["bands"] if b in om]
            assert all(n == 1 for (b, n, _) in u["bands"] if b in om) and len(gains) == len(coded)
            if rule == "zero":
                assert all(g[3] == 0 for g in gains) and infos[cf]["units"][0]["env_nonzero"] == 0
                assert not lines[cf, cut.get(name, 512):].any()                       # a zero envelope zeroes the top
            if rule == "neg":
                assert all(g[3] >> (g[2] - 1) for g in gains)
            if u["sbr"]:
                env_counts.add(infos[cf]["units"][0]["env_nonzero"])
        assert vs.census(c)["sbr_blocks"] == sum(1 for s, _, _ in plan if s != "none")
    assert sum(1 for s, _, _ in vs.SBR_PLANS["sbr_partial"] if s != "all") == 3    # only some omitted bands coded
    # the envelope holds one value per coded omitted band and zeros: 2 bands at 48 and 44.1 kHz, 3 at 32 kHz.  The
    # oracle takes its sparse Gaussian at <= 8 non-zero entries, so the dense form is unreachable from a well-formed
    # gain-shape record at these layouts; `sbr_sparse_dense` covers 0, 1 and 2 entries
    assert env_counts == {0, 1, 2, 3}
    c = vs.case("sbr_sparse_dense")
    assert sorted(floats["sbr_sparse_dense"][4][cf]["units"][0]["env_nonzero"] for cf in (0, 1, 4, 5)) == [1, 1, 1, 2]
    assert len(vs.case("sbr_sr32").p.omittedBands) == 3
    # empty low bands: the transposed lines are all zero but the last, which the interpolation takes half from line
    # 512 -- the first omitted band's own value; a band of zeros is left alone by the `max > 0` guard
    for cf in (0, 1, 4, 5):
        assert not floats["sbr_empty_low"][3][cf][:1023].any()
    assert floats["sbr_empty_low"][3][0][1023] != 0 and not floats["sbr_empty_low"][3][4].any()


# ---------------------------------------------------------------------------------- the reference's own decoder
@pytest.mark.parametrize("name", vs.FIXTURE_CASES)
def test_oracle_with_model_leaves_equals_the_reference_decoder(name):
    """the four streams the reference's PACFile reader and decoder were run on (no leaf above K = 4096, so that its
    codebook layer finishes): it takes every one, and the oracle with pvq_model's leaves gives its PCM sample for
    sample -- negative gains, gain index 0 and all ones, angle index 0 throughout, omitted bands coded one by one"""
    gold = np.load(os.path.join(GOLDEN, "vq_code_streams.npz"))
    c = vs.fixture_case(name)
    assert zlib.crc32(c.pac) == int(gold["crc_" + name])
    assert str(gold["error_" + name]) == ""
    want = gold["pcm_" + name]
    got = vs.decode_stream_vq(c.pac)
    assert got.dtype == want.dtype == np.int16 and got.shape == want.shape == ((c.hops + 1) * 1024, c.n_ch)
    assert np.array_equal(got, want), int(np.sum(got != want))
    assert max(nd[4] for nd in nodes(c, "leaf")) <= vs.FIXTURE_K_LIMIT
    got = vs.census(c)
    assert got["gain_negative"] > 10 and (name != "sbr_partial" or got["sbr_blocks"] == 3)
