"""The cases of tests/golden/widths.part*.npz: one six-hop stream coded by the REFERENCE at field widths other than
nScaleBits = 4, nMantSizeBits = 12 (test helper; tests/golden/make_widths.py writes the fixture, this module names the
cases, reads it and states what makes every case worth having).

  stream   hops 24..30 of excerpt_castanet (stereo, 44.1 kHz), block switching on: blocks with the flag triples
           (0,0,1) (0,1,1) (1,1,1) (1,1,0) (1,0,0) (0,0,0): three short-coded hops, a start and a stop window
  case     (coder, nScaleBits, nMantSizeBits, kb/s per channel); coder 'sc' scalar mantissas, 'vq' gain-shape,
           'vqsbr' gain-shape with spectral band replication

  per case `tag`:  pac_bs_<tag> the reference's block-switched file, dec_bs_<tag> its decoder's int16 PCM of that file,
                   flags_<tag> the triples its driver passed;  scalar cases also pac_long_<tag>, the long-only file
  per (coder, kb/s):  base_<coder>_<kbps> the reference's block-switched file at 4 / 12
  vqcurve_*:       vq_band_model.curve of the first two hops at 4 / 3, cap 320 kb/s (nmr, cap, cap_alloc, written)
"""
import functools
import struct

import numpy as np

import golden_io
from oracle import pac_oracle as po

EXCERPT, HOP0, HOP1 = "castanet", 24, 30
FLAGS = [(0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 0, 0)]      # the six hops, the last again

SCALAR = [(3, 5, 128), (4, 3, 128), (4, 3, 320), (4, 1, 128), (1, 4, 128), (2, 2, 128), (4, 16, 128), (4, 16, 64),
          (4, 16, 32)]
VQ = [(3, 5, 128), (4, 3, 128), (2, 2, 128), (4, 1, 128)]
VQ_SBR = [(3, 5, 96), (4, 16, 96)]
CASES = [("sc",) + c for c in SCALAR] + [("vq",) + c for c in VQ] + [("vqsbr",) + c for c in VQ_SBR]
NOTHING_ALLOCATED = ("sc", 4, 16, 32)          # the budget is below zero in every block: the file is heads only
RATE_PAIRS = [(3, 5), (4, 3), (2, 16)]         # the width pairs of the rate-control tests
RATE_CASES = [(3, 5, 320), (4, 3, 320), (2, 16, 320), (4, 3, 48)]        # (widths, cap kb/s): at 48 the cap rule engages
NMR_TARGETS = (0.0, -6.0)                      # dB; tests/test_oracle_widths.py: no unit within the tie window of either
VQ_CURVE = {"widths": (4, 3), "hops": 2, "cap_kbps": 320}


def tag_of(case):
    return "%s_%d_%d_%d" % case


def case_id(case):
    return tag_of(case)


def is_vq(case):
    return case[0] != "sc"


def uses_sbr(case):
    return case[0] == "vqsbr"


def stream():
    """(pcm int16 [6144, 2], sample rate)"""
    ex = np.load(golden_io.GOLDEN + f"/excerpt_{EXCERPT}.npz")
    return np.ascontiguousarray(ex["pcm"][HOP0 * 1024:HOP1 * 1024]), int(ex["sr"])


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = golden_io.load_npz("widths")
    return _fixture


def header(data):
    """(oracle params with the stream's widths and coder, header length)"""
    data = bytes(data)
    fmt = '<LHLLHHHH'
    (sr, n_ch, _, n_lines, ns, nm, use_sbr, use_vq) = struct.unpack(fmt, data[4:4 + struct.calcsize(fmt)])
    pos = 4 + struct.calcsize(fmt)
    pos += 4 + 2 * struct.unpack('<L', data[pos:pos + 4])[0]
    p = po.make_params(sr, n_ch, 128, n_lines, ns, nm)
    p.useVQ, p.useSBR = bool(use_vq), bool(use_sbr)
    p.omittedBands = list(po.omitted_bands(p.sfBands)) if use_sbr else []
    return p, pos


def heads(data):
    """What the heads of a stream say, record by record: a list of (flags, [(overall, alloc [nBands], sf [nBands] or
    None for a gain-shape stream)] per (sub-)block).  The gain-shape reader stops after the allocations of the FIRST
    unit of a record: the fields that follow have data-dependent widths."""
    data = bytes(data)
    p, pos = header(data)
    out = []
    while pos < len(data):
        n = struct.unpack('<L', data[pos:pos + 4])[0]
        br = po.BitReader(data[pos + 4:pos + 4 + n] + b'\0' * 8)
        pos += 4 + n
        flags = (br.get(1), br.get(1), br.get(1))
        cur = bool(flags[1])
        units = []
        if p.useVQ:
            bands = p.sfBandsShort if cur else p.sfBands
            overall = br.get(p.nScaleBits)
            alloc = [a + 1 if a else 0 for a in (br.get(p.nMantSizeBits) for _ in range(bands.nBands))]
            units.append((overall, np.array(alloc), None))
        else:
            p.nMDCTLines = p.nSamplesPerBlock = po.SHORT_LINES if cur else 1024
            try:
                for _ in range(8 if cur else 1):
                    sf, alloc, _, overall = po.parse_block_body(br, p, cur)
                    units.append((overall, np.array(alloc), np.array(sf)))
            finally:
                p.nMDCTLines = p.nSamplesPerBlock = 1024
        out.append((flags, units))
    return out


def check_case(case, pac_bs, base_bs, flags):
    """The conditions that make a case worth having, with no exception: raises AssertionError where one fails."""
    coder, ns, nm, kbps = case
    flags = [tuple(int(v) for v in f) for f in flags]
    assert any(f[1] for f in flags), flags                                     # a short-coded hop
    assert any(not f[1] and f[2] and not f[0] for f in flags), flags           # a start window
    assert any(not f[1] and f[0] and not f[2] for f in flags), flags           # a stop window
    hs = heads(pac_bs)
    assert sorted({h[0] for h in hs}) == sorted(set(flags)), (sorted({h[0] for h in hs}), flags)
    units = [u for _, us in hs for u in us]
    allocs = set(int(v) for u in units for v in u[1])
    cap = min(1 << nm, 16)
    assert allocs <= {0} | set(range(2, cap + 1)), (case, allocs)
    if case == ("sc", 4, 3, 320):
        assert max(allocs) == 8, allocs                                        # some band sits at the cap 8, none above
    if nm == 1:
        assert allocs == {0, 2}, allocs
    if nm == 2:
        assert allocs <= {0, 2, 3, 4} and len(allocs) > 1, allocs
    if coder == "sc" and (ns, nm) in ((1, 4), (2, 2)):
        top = (1 << ns) - 1
        assert any(u[0] == top or (u[2] == top).any() for u in units), case     # a scale at the cap 2^nScaleBits - 1
        assert all(u[0] <= top and (u[2] <= top).all() for u in units), case
    if case == NOTHING_ALLOCATED:
        assert allocs == {0}, allocs
    else:
        assert allocs != {0}, case
    (_, at), (_, base_at) = header(pac_bs), header(base_bs)
    assert bytes(pac_bs)[at:] != bytes(base_bs)[base_at:], case                 # the widths change the body


# ------------------------------------------------------------------------------------------ the rate-control models
@functools.lru_cache(maxsize=None)
def rate_analysis(ns, nm):
    """rate_model.analysis of the stream at these widths: computed once, shared, never changed"""
    import rate_model as rm
    pcm, sr = stream()
    return rm.analysis(pcm, sr, True, ns, nm)


@functools.lru_cache(maxsize=None)
def band_curve(ns, nm, cap_kbps):
    import band_model as bm
    return bm.curve(rate_analysis(ns, nm), cap_kbps)


@functools.lru_cache(maxsize=None)
def rate_curve(ns, nm, cap_kbps):
    import abr_model as am
    return am.curve(rate_analysis(ns, nm), cap_kbps)


@functools.lru_cache(maxsize=None)
def rate_search(ns, nm, cap_kbps, target):
    """rate_model.search: (budget, capped, margin, live)"""
    import rate_model as rm
    return rm.search(rate_analysis(ns, nm), target, cap_kbps)
