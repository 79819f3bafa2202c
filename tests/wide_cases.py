"""The cases of tests/golden/wide.part*.npz: 4 to 8 channels and sample rates above 96 kHz (test helper, NumPy only;
tests/golden/make_wide.py writes the fixture with the oracle, this module names the cases, makes their PCM, reads the
fixture and states what makes every case worth having).

  case     (sample rate, channels, seed): five hops of soak_programmes.programme(seed, 5, channels, rate) -- integer
           arithmetic alone, the same int16 PCM on every machine.  Where the programme has no dropped hop of the kind
           below, plant() writes a silent stretch into channel 1 and a click into channel 0 of hop 1.
  every case has
           a transient hop by the oracle's detector, and
           a dropped hop: a short-coded block with an all-zero sub-block in a channel that is NOT channel 0 (the
           reference's writer leaves such a block out of the file in every channel)
  coders   `long` scalar mantissas without block switching, `bs` scalar block-switched, `vq` gain-shape without SBR
           (all three at 128 kb/s per channel), `vqsbr` gain-shape with spectral band replication at 96 kb/s

  per case `tag` and coder:  pac_<coder>_<tag> the oracle's file;  dec_<coder>_<tag> its decoder's int16 PCM, or
                             raises_<coder>_<tag> the name of what it raised (the SBR decoder above 48 kHz: IndexError)
  per case:                  sha_<tag> sha256 of the PCM, tr_<tag> the detector's decision hop by hop
  per rate-control case:     the models' arrays, see RATE_ARRAYS
"""
import functools
import hashlib

import numpy as np

import golden_io
import soak_programmes as sp
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv

FIXTURE = "wide"                        # tests/golden/wide.part*.npz (tests/golden_io.py)
HOP, SHORT, SUB = 1024, 128, 8
N_HOPS = 5
N_BLOCKS = N_HOPS + 2                   # every hop, the last hop again, Close

# (sample rate, channels, seed)
CHANNEL_CASES = [(48000, 4, 41_014), (48000, 5, 41_031), (48000, 6, 41_283), (48000, 8, 41_262)]
RATE_CASES = [(64000, 2, 42_070), (88200, 2, 42_089), (176400, 2, 42_180), (192000, 2, 42_195)]
BOTH_CASES = [(192000, 8, 43_439), (64000, 5, 43_137)]
CASES = CHANNEL_CASES + RATE_CASES + BOTH_CASES
REGENERATED = [(48000, 8, 41_262), (192000, 2, 42_195)]       # tests/test_wide_cases.py makes these two from scratch
RATE_CONTROL = BOTH_CASES + [(48000, 8, 41_262), (176400, 2, 42_180)]

# coder -> (kb/s per channel, block switching, gain-shape, SBR)
CODERS = {"long": (128, False, False, False), "bs": (128, True, False, False), "vq": (128, True, True, False),
          "vqsbr": (96, True, True, True)}
STREAMS = [(case, coder) for case in CASES for coder in CODERS]

# long bands, lines they hold, short bands, lines they hold (oracle.band_table)
BANDS = {48000: (17, 1024, 6, 128), 64000: (15, 768, 5, 96), 88200: (13, 557, 4, 70), 176400: (9, 279, 2, 35),
         192000: (9, 256, 2, 32)}

CAP_KBPS = 160                          # the cap of the rate-control tests: J of the models stays small
TARGETS = (-3.0, -6.0)                  # dB; TARGETS[0] is the one of encode_pack_nmr
VQ_HOPS = 2                             # the gain-shape band curve: the first two hops
WINDOW = 1e-4                           # dB: the tie window of tests/test_gpu_rate.py and tests/test_gpu_band.py
RATE_ARRAYS = ("abr_worst", "abr_bits", "abr_steps", "band_nmr", "band_cap", "band_cap_alloc", "search_budget",
               "search_capped", "search_margin", "vq_nmr", "vq_cap", "vq_cap_alloc", "vq_written")


def tag_of(case):
    return "%d_%dch" % case[:2]


def case_id(case):
    return tag_of(case)


def stream_id(stream):
    return tag_of(stream[0]) + "_" + stream[1]


# ------------------------------------------------------------------------------------------------- the PCM
def transients(pcm):
    """the oracle's detector on every hop as the driver feeds it: the hop, then zeros"""
    n_ch = pcm.shape[1]
    out = []
    for h in range(len(pcm) // HOP):
        look = np.zeros((n_ch, 2 * HOP))
        for ch in range(n_ch):
            look[ch, :HOP] = po.pcm16_to_fraction(pcm[h * HOP:(h + 1) * HOP, ch])
        out.append(bool(po.transient_detect(look)))
    return out


def block_flags(tr):
    """(last, cur, next) of the N_BLOCKS blocks the driver submits"""
    flags, last_t, cur_t = [], False, False
    for h in range(len(tr) + 1):
        nxt = tr[h] if h < len(tr) else False
        flags.append((last_t, cur_t, nxt))
        last_t, cur_t = cur_t, nxt
    return flags + [(False, False, False)]


def zero_sub_blocks(pcm):
    """[(block, channel, sub-block)] of every all-zero sub-block of every block, short-coded or not"""
    n, n_ch = pcm.shape
    buf = np.zeros(((len(pcm) // HOP + 3) * HOP, n_ch), np.int16)
    buf[HOP:HOP + n] = pcm
    buf[HOP + n:2 * HOP + n] = pcm[n - HOP:]
    out = []
    for f in range(len(pcm) // HOP + 2):
        for ch in range(n_ch):
            for j in range(SUB):
                at = f * HOP + 448 + SHORT * j
                if not buf[at:at + 2 * SHORT, ch].any():
                    out.append((f, ch, j))
    return out


def dropped_blocks(pcm, tr=None):
    """{block: channels with an all-zero sub-block} of the short-coded blocks the writer leaves out"""
    flags = block_flags(transients(pcm) if tr is None else tr)
    out = {}
    for f, ch, _ in zero_sub_blocks(pcm):
        if flags[f][1]:
            out.setdefault(f, set()).add(ch)
    return out


def has_both(pcm):
    tr = transients(pcm)
    return any(tr) and any(chs - {0} for chs in dropped_blocks(pcm, tr).values())


def plant(pcm):
    """a click in channel 0 of hop 1 and digital silence in channel 1 over its samples 400 ... 719, which holds all of
    sub-block 0 (samples 448 ... 703) of block 2"""
    pcm = pcm.copy()
    pcm[HOP + 400:HOP + 720, 1] = 0
    pcm[HOP + 800:HOP + 806, 0] = 30000
    return pcm


@functools.lru_cache(maxsize=None)
def material(case):
    """(pcm int16 [5120, channels] read-only, planted) of a case"""
    sr, n_ch, seed = case
    pcm = sp.programme(seed, N_HOPS, n_ch, sr)
    planted = not has_both(pcm)
    if planted:
        pcm = plant(pcm)
    pcm.setflags(write=False)
    return pcm, planted


def digest(pcm):
    return hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------- the oracle
def oracle_encode(case, coder, collect=None):
    pcm, _ = material(case)
    kbps, bs, vq, sbr = CODERS[coder]
    if vq:
        assert sbr == (kbps < 128)                    # encode_stream_vq's own rule gives the coder's setting
        return pv.encode_stream_vq(pcm, case[0], kbps, True, collect=collect)
    return po.encode_stream(pcm, case[0], kbps, bs, collect=collect)


def oracle_decode(coder, data):
    """(int16 PCM, None) or (None, the name of what the oracle's decoder raised)"""
    try:
        return (pv.decode_stream_vq(data) if CODERS[coder][2] else po.decode_stream(data)), None
    except Exception as e:                            # the reference's Decode_SBR above 48 kHz
        return None, type(e).__name__


def alloc_ties(budget, max_mant_bits, n_lines, smr):
    """oracle.bit_alloc's loop once more, watching its np.round: the number of passes without a flip level in which
    some live band's value lies exactly half way between two integers (with a flip level one band is put there by
    construction)"""
    n_lines, smr = np.asarray(n_lines), np.asarray(smr)
    bits = np.zeros(len(n_lines), dtype=int)
    dropped = np.zeros(len(n_lines), dtype=bool)
    n_flip = passes = ties = 0
    while True:
        live = np.logical_not(dropped)
        total = np.sum(n_lines[live])
        if total == 0:
            total += 1e-12
        want = budget / total + (1.0 / po.DB_PER_BIT) * (smr[live] - np.sum(n_lines[live] * smr[live]) / total)
        frac = want - np.floor(want) - 0.5
        ladder = np.sort(frac[frac > 0])
        if n_flip > len(ladder):
            n_flip -= 1
        else:
            level = 0. if n_flip == 0 else ladder[n_flip - 1]
            v = want - level
            ties += int(n_flip == 0 and np.any(v - np.floor(v) == 0.5))
            bits[live] = np.round(v)
        bits[bits > max_mant_bits] = max_mant_bits
        dropped = bits < 2
        bits[dropped] = 0
        stable = np.logical_xor(dropped, live).all()
        spent = np.sum(np.multiply(bits, n_lines))
        if stable & (spent <= budget):
            break
        if stable & (spent > budget):
            n_flip += 1
        passes += 1
        if passes > 200:
            break
    return ties, bits


def budget_ties(case, coder):
    """Units of a scalar stream in whose BitAlloc np.round meets an exact tie -- budget / lines exactly k + 0.5 for a
    band at the mean SMR of the live bands, as in a unit whose SMRs are all equal.  np.round breaks such a tie to
    even and the last bit of the division decides; the product raises PACX_ST_GUARD for it (the soak's `guard`
    class).  -> [(block, channel, unit, budget)]"""
    import rate_model as rm
    sr, n_ch, _ = case
    kbps, bs, vq, _ = CODERS[coder]
    assert not vq
    a = rate_analysis(case) if bs else rm.analysis(material(case)[0], sr, False)
    p = po.make_params(sr, n_ch, kbps)
    out = []
    for f, row in enumerate(a["units"]):
        for ch, us in enumerate(row or []):
            for j, u in enumerate(us):
                p.nMDCTLines = p.nSamplesPerBlock = SHORT if u.short else HOP
                budget = po.bit_budget(p, *u.flags)
                p.nMDCTLines = p.nSamplesPerBlock = HOP
                ties, bits = alloc_ties(budget, 16, u.bands.nLines, u.smr)
                assert np.array_equal(bits, po.bit_alloc(budget, 16, u.bands.nBands, u.bands.nLines, u.smr))
                if ties:
                    out.append((f, ch, j, budget))
    return out


# ------------------------------------------------------------------------------------------------- the fixture
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = golden_io.load_npz(FIXTURE)
    return _fixture


def reference(case, coder):
    return bytes(fixture()["pac_%s_%s" % (coder, tag_of(case))])


def decoded(case, coder):
    """(int16 PCM, None) or (None, what the oracle's decoder raised)"""
    g, key = fixture(), "%s_%s" % (coder, tag_of(case))
    if "dec_" + key in g:
        return g["dec_" + key], None
    return None, str(g["raises_" + key])


def stream_arrays(case, coder):
    """what make_wide.py stores for one stream"""
    data = oracle_encode(case, coder)
    dec, raised = oracle_decode(coder, data)
    key = "%s_%s" % (coder, tag_of(case))
    out = {"pac_" + key: np.frombuffer(data, np.uint8)}
    if raised is None:
        assert dec.dtype == np.int16
        out["dec_" + key] = dec
    else:
        out["raises_" + key] = np.array(raised)
    return out


def case_arrays(case):
    pcm, _ = material(case)
    tag = tag_of(case)
    out = {"sha_" + tag: np.array(digest(pcm)), "tr_" + tag: np.array(transients(pcm), np.uint8)}
    for coder in CODERS:
        out.update(stream_arrays(case, coder))
    return out


# ------------------------------------------------------------------------------------------ the rate-control models
@functools.lru_cache(maxsize=None)
def rate_analysis(case):
    """rate_model.analysis of the case, block-switched: computed once, shared, never changed"""
    import rate_model as rm
    return rm.analysis(material(case)[0], case[0], True)


@functools.lru_cache(maxsize=None)
def vq_analysis(case):
    import rate_model as rm
    return rm.analysis(material(case)[0][:VQ_HOPS * HOP], case[0], True)


def rate_arrays(case):
    """the models' arrays of a rate-control case, as make_wide.py stores them (key -> array, without the tag)"""
    import abr_model as am
    import band_model as bm
    import rate_model as rm
    import vq_band_model as vm
    a = rate_analysis(case)
    c = am.curve(a, CAP_KBPS)
    b = bm.curve(a, CAP_KBPS)
    budget, capped, margin, live = rm.search(a, TARGETS[0], CAP_KBPS)
    v = vm.curve(vq_analysis(case), CAP_KBPS)
    return {"abr_worst": c["worst"], "abr_bits": c["bits"], "abr_steps": c["steps"], "band_nmr": b["nmr"],
            "band_cap": b["cap"], "band_cap_alloc": b["cap_alloc"], "search_budget": budget, "search_capped": capped,
            "search_margin": margin, "vq_nmr": v["nmr"], "vq_cap": v["cap"], "vq_cap_alloc": v["cap_alloc"],
            "vq_written": v["written"]}


def stored(case, name):
    return fixture()["%s_%s" % (name, tag_of(case))]


@functools.lru_cache(maxsize=None)
def band_curve(case):
    """band_model's curve of the case with the arrays of the fixture"""
    import band_model as bm
    c = bm.tables(rate_analysis(case)["p"])
    c["nmr"], c["cap"], c["cap_alloc"] = (stored(case, "band_" + k) for k in ("nmr", "cap", "cap_alloc"))
    return c


@functools.lru_cache(maxsize=None)
def vq_curve(case):
    import band_model as bm
    c = bm.tables(vq_analysis(case)["p"])
    c["nmr"], c["cap"], c["cap_alloc"], c["written"] = (stored(case, "vq_" + k) for k in
                                                         ("nmr", "cap", "cap_alloc", "written"))
    return c


@functools.lru_cache(maxsize=None)
def rate_curve(case):
    """abr_model's curve of the case with the arrays of the fixture"""
    import abr_model as am
    a = rate_analysis(case)
    row, sub = am.layout(a, CAP_KBPS)
    c = {"worst": stored(case, "abr_worst"), "bits": stored(case, "abr_bits"), "steps": stored(case, "abr_steps"),
         "row": row, "sub_stride": sub}
    c["evals"] = int((c["steps"][c["steps"] >= 0] + 1).sum())
    return c


# ------------------------------------------------------------------------------------------------- parsed streams
def scalar_units(data):
    """What a scalar stream holds, record by record: [(flags, [(overall, alloc [nBands], sf [nBands], mantissas of the
    coded lines in order)] per (sub-)block)], as oracle.encode_channel returns them"""
    import widths_cases
    data = bytes(data)
    p, pos = widths_cases.header(data)
    assert not p.useVQ
    out = []
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "little")
        br = po.BitReader(data[pos + 4:pos + 4 + n] + b'\0' * 8)
        pos += 4 + n
        flags = (br.get(1), br.get(1), br.get(1))
        cur = bool(flags[1])
        bands = p.sfBandsShort if cur else p.sfBands
        p.nMDCTLines = p.nSamplesPerBlock = SHORT if cur else HOP
        units = []
        try:
            for _ in range(SUB if cur else 1):
                sf, alloc, lines, overall = po.parse_block_body(br, p, cur)
                keep = np.repeat(np.asarray(alloc) != 0, bands.nLines)
                units.append((overall, np.asarray(alloc), np.asarray(sf), lines[:len(keep)][keep]))
        finally:
            p.nMDCTLines = p.nSamplesPerBlock = HOP
        out.append((flags, units))
    return out
