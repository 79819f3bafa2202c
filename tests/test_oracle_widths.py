"""Field widths other than nScaleBits = 4 / nMantSizeBits = 12 on the CPU: the oracle against what the REFERENCE wrote
and decoded at those widths (tests/golden/widths.part*.npz, tests/golden/make_widths.py; cases in
tests/widths_cases.py), and the rate-control models at the three width pairs the GPU tests use them at.  No GPU, no
reference.

Everything is exact: bytes, int16 PCM, integers.  The one float check is the tie window of tests/test_gpu_rate.py and
tests/test_gpu_band.py (1e-4 dB): no unit of the stream may lie inside it at the targets of widths_cases.NMR_TARGETS,
so that the GPU tests leave no unit out.
"""
import numpy as np
import pytest

import band_model as bm
import nmr_model as nm
import profile_model as pm
import rate_model as rm
import widths_cases as wc
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv

WINDOW = 1e-4               # dB: tests/test_gpu_rate.py, tests/test_gpu_band.py
GRID = bm.GRID


def oracle_encode(case, pcm, sr, block_switching):
    coder, ns, nm_bits, kbps = case
    if wc.is_vq(case):
        assert wc.uses_sbr(case) == (kbps < 128)           # encode_stream_vq's own rule gives the case's setting
        return pv.encode_stream_vq(pcm, sr, kbps, block_switching=block_switching, n_scale_bits=ns,
                                   n_mant_size_bits=nm_bits)
    return po.encode_stream(pcm, sr, kbps, block_switching=block_switching, n_scale_bits=ns, n_mant_size_bits=nm_bits)


# ------------------------------------------------------------------ 1. the fixture itself
def test_fixture_holds_the_cases_and_the_stream():
    g = wc.fixture()
    pcm, sr = wc.stream()
    assert [str(c) for c in g["cases"]] == [wc.tag_of(c) for c in wc.CASES]
    assert np.array_equal(g["pcm"], pcm) and int(g["sr"]) == sr and pcm.shape == (6 * 1024, 2)
    assert len(wc.CASES) == len(set(wc.CASES)) == 15
    assert ("sc", 4, 16, 64) in wc.CASES and wc.NOTHING_ALLOCATED in wc.CASES


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_case_is_worth_having(case):
    """the conditions the generator asserted, from the committed file"""
    g = wc.fixture()
    tag = wc.tag_of(case)
    flags = [tuple(int(v) for v in f) for f in g["flags_" + tag]]
    assert flags == wc.FLAGS
    wc.check_case(case, bytes(g["pac_bs_" + tag]), bytes(g["base_%s_%d" % (case[0], case[3])]), flags)
    p, _ = wc.header(g["pac_bs_" + tag])
    assert (p.nScaleBits, p.nMantSizeBits, p.useVQ, p.useSBR) == (case[1], case[2], wc.is_vq(case), wc.uses_sbr(case))
    if not wc.is_vq(case):
        hs = wc.heads(g["pac_long_" + tag])
        assert len(hs) == 2 * 8 and not any(any(f) for f, _ in hs)


def test_nothing_allocated_is_the_floor_of_heads():
    g = wc.fixture()
    data = bytes(g["pac_bs_" + wc.tag_of(wc.NOTHING_ALLOCATED)])
    p, at = wc.header(data)
    nbl, nbs = p.sfBands.nBands, p.sfBandsShort.nBands
    long_bytes = (4 + nbl * 20 + 4 + 7) // 8               # overall scale, 16 + 4 bits a band; + 4 bits, rounded up
    short_bytes = (8 * (4 + nbs * 20) + 4 + 7) // 8
    n_short = sum(f[1] for f in wc.FLAGS)
    assert len(data) == at + 2 * ((8 - n_short) * (4 + long_bytes) + n_short * (4 + short_bytes)) == 1340


# ------------------------------------------------------------------ 2. the oracle against the reference
@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_oracle_writes_the_references_bytes(case):
    g = wc.fixture()
    pcm, sr = wc.stream()
    assert oracle_encode(case, pcm, sr, True) == bytes(g["pac_bs_" + wc.tag_of(case)])


@pytest.mark.parametrize("case", [c for c in wc.CASES if not wc.is_vq(c)], ids=wc.case_id)
def test_oracle_writes_the_references_bytes_long_only(case):
    g = wc.fixture()
    pcm, sr = wc.stream()
    assert oracle_encode(case, pcm, sr, False) == bytes(g["pac_long_" + wc.tag_of(case)])


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_oracle_decodes_to_the_references_pcm(case):
    g = wc.fixture()
    tag = wc.tag_of(case)
    data = bytes(g["pac_bs_" + tag])
    pcm = pv.decode_stream_vq(data) if wc.is_vq(case) else po.decode_stream(data)
    want = g["dec_bs_" + tag]
    assert want.dtype == np.int16 and pcm.shape == want.shape and np.array_equal(pcm, want)


def test_defaults_are_unchanged():
    pcm, sr = wc.stream()
    assert po.encode_stream(pcm, sr, 128, True) == po.encode_stream(pcm, sr, 128, True, n_scale_bits=4,
                                                                      n_mant_size_bits=12)
    p = pv.make_params_vq(sr, 2, 96)
    assert (p.nScaleBits, p.nMantSizeBits, p.useVQ, p.useSBR) == (4, 12, True, True)
    p = pv.make_params_vq(sr, 2, 128, 3, 5)
    assert (p.nScaleBits, p.nMantSizeBits, p.useVQ, p.useSBR) == (3, 5, True, False)
    a = rm.analysis(pcm[:1024], sr, False)
    assert rm.widths(a) == (4, 12) and (a["p"].nScaleBits, a["p"].nMantSizeBits) == (4, 12)


def test_nmr_model_reads_the_widths_from_the_stream():
    """nmr_model.model parses a stream with the widths its header declares"""
    g = wc.fixture()
    pcm, sr = wc.stream()
    m = nm.model(pcm, bytes(g["pac_bs_sc_3_5_128"]), True)
    live = ~np.isnan(m["nmr_db"])
    assert live.any() and np.isfinite(m["nmr_db"][live]).all() and m["flags"][:7] == [tuple(map(bool, f)) for f in wc.FLAGS]


# ------------------------------------------------------------------ 3. the rate-control models at the three pairs
def units_of(a):
    for row in a["units"]:
        if row is not None:
            for us in row:
                yield from us


@pytest.mark.parametrize("ns,nm_bits", wc.RATE_PAIRS)
def test_analysis_records_the_widths(ns, nm_bits):
    a = wc.rate_analysis(ns, nm_bits)
    assert (a["n_scale_bits"], a["n_mant_size_bits"]) == rm.widths(a) == (ns, nm_bits)
    assert (a["p"].nScaleBits, a["p"].nMantSizeBits) == (ns, nm_bits)
    assert [tuple(int(v) for v in f) for f in a["flags"]] == wc.FLAGS + [(0, 0, 0)] and not any(a["dropped"])
    top = (1 << ns) - 1
    assert all(0 <= u.overall <= top for u in units_of(a))
    # budgets that are the constant-rate rule's own reproduce the oracle's (= the reference's) constant-rate stream
    pcm, sr = wc.stream()
    p = po.make_params(sr, 2, 128, 1024, ns, nm_bits)
    cbr = np.zeros((len(a["flags"]), 2, rm.SUB))
    for f, row in enumerate(a["units"]):
        for ch, us in enumerate(row):
            for j, u in enumerate(us):
                p.nMDCTLines = rm.SHORT if u.short else rm.HOP
                cbr[f, ch, j] = po.bit_budget(p, *u.flags)
    assert rm.encode(a, cbr, len(pcm)) == po.encode_stream(pcm, sr, 128, True, n_scale_bits=ns, n_mant_size_bits=nm_bits)


@pytest.mark.parametrize("ns,nm_bits,cap", wc.RATE_CASES)
@pytest.mark.parametrize("target", wc.NMR_TARGETS)
def test_search_is_consistent_and_no_unit_is_inside_the_tie_window(ns, nm_bits, cap, target):
    """tests/test_rate_model.py's checks of the budget search; and the margin of every unit, so that the GPU test at
    these targets excludes none"""
    a = wc.rate_analysis(ns, nm_bits)
    budget, capped, margin, live = wc.rate_search(ns, nm_bits, cap, target)
    assert live.sum() == 10 + 6 * 8 and not budget[~live].any() and not capped[~live].any()
    print(f"{ns}/{nm_bits} cap {cap} at {target:+.0f} dB: smallest margin {margin[live].min():.3g} dB, "
          f"{int(capped.sum())} of {int(live.sum())} units capped")
    assert margin[live].min() >= WINDOW
    for f, row in enumerate(a["units"]):
        for ch, us in enumerate(row):
            for j, u in enumerate(us):
                J = rm.cap_steps(a, u, cap)
                b = int(budget[f, ch, j])
                assert b % rm.STEP == 0 and 0 <= b <= rm.STEP * J
                w = rm.worst_nmr(a["p"], u, b)
                if capped[f, ch, j]:
                    assert b == rm.STEP * J and w > target
                else:
                    assert w <= target
    if cap == 48:
        assert capped.any()


@pytest.mark.parametrize("ns,nm_bits,cap", wc.RATE_CASES)
def test_band_model_is_consistent(ns, nm_bits, cap):
    """tests/test_band_model.py / test_profile_model.py on this stream's curve: total == total_slow, frame by frame;
    profile == total at every target of +-30 dB; the solve on the profile is the solve on the curve; no pick above
    maxMantBits"""
    a = wc.rate_analysis(ns, nm_bits)
    c = wc.band_curve(ns, nm_bits, cap)
    top = bm.max_mant(a["p"])
    assert c["n_cand"] == top == min(1 << nm_bits, 16) and (c["n_scale_bits"], c["n_mant_size_bits"]) == (ns, nm_bits)
    unit, lines = bm.layout(c)
    live = unit >= 0
    assert live.sum() == 10 * len(c["lines_long"]) + 6 * 8 * len(c["lines_short"])
    assert np.isfinite(c["nmr"][live][:, :top]).all() and np.isposinf(c["nmr"][live][:, top:]).all()
    assert c["cap_alloc"].max() <= top and set(np.unique(c["cap_alloc"])) <= {0} | set(range(2, top + 1))
    t_lo, t_hi = -30 * GRID, 30 * GRID
    want = np.zeros(t_hi - t_lo + 1, np.int64)
    kinds = np.zeros(2, int)
    for t in range(t_lo, t_hi + 1):
        tot, alloc, n_bytes, capped, missed, over = bm.evaluate(c, t, detail=True)
        want[t - t_lo] = tot
        assert alloc.max() <= top and not alloc[~live].any()
        kinds += [int(missed.any()), int(over.any())]
        if t % 331 == 0:
            assert tot == bm.total_slow(c, t)
            for cf in range(len(c["cap"])):
                fa, n, fc = bm.frame(c, cf, t / GRID)
                assert np.array_equal(alloc[cf], fa) and n_bytes[cf] == n and capped[cf] == fc
    assert np.array_equal(pm.profile(c, t_lo, t_hi), want)
    if nm_bits == 3:
        assert kinds[0] > 0                                    # at -30 dB some band misses even with 8 bits a line
    if cap == 48:
        assert kinds[1] > 0                                    # the cap rule engages
    for limit in (int(want[-1]) - 1, int(want[-1]), int((want[0] + want[-1]) // 2), int(want.max()) + 1):
        s, q = bm.solve(c, limit, t_lo, t_hi), pm.solve(want, limit, t_lo, t_hi)
        assert (q["t"], q["met"], q["total"]) == (s["t"], s["met"], s["total"]), limit
        assert s["bit_alloc"].max() <= top
    for target in wc.NMR_TARGETS:
        m = bm.margins(c, target)
        print(f"{ns}/{nm_bits} cap {cap} at {target:+.0f} dB: smallest band margin {m[c['cap'] >= 0].min():.3g} dB")
        assert m[c["cap"] >= 0].min() >= WINDOW


def test_vq_curve_of_the_fixture_is_the_models():
    """two units of the committed gain-shape curve recomputed, as tests/test_vq_band_model.py does for its own"""
    import vq_band_model as vm
    g = wc.fixture()
    pcm, sr = wc.stream()
    a = rm.analysis(pcm[:wc.VQ_CURVE["hops"] * 1024], sr, True, *wc.VQ_CURVE["widths"])
    short_cf = next(f * 2 for f, fl in enumerate(a["flags"]) if fl[1])
    only = {(0, 0), (short_cf, 3)}
    c = vm.curve(a, wc.VQ_CURVE["cap_kbps"], only=only)
    assert c["n_cand"] == 8 and g["vqcurve_nmr"].shape == c["nmr"].shape
    whole = bm.with_arrays(c, g["vqcurve_nmr"], g["vqcurve_cap"], g["vqcurve_cap_alloc"])
    for target in wc.NMR_TARGETS:                              # no unit inside the tie window at the targets picked at
        assert bm.margins(whole, target)[whole["cap"] >= 0].min() >= WINDOW, target
    nbl, nbs = len(c["lines_long"]), len(c["lines_short"])
    for (cf, sb), nb in zip(sorted(only), (nbl, nbs)):
        at = slice(sb * nb, (sb + 1) * nb)
        assert np.array_equal(g["vqcurve_nmr"][cf, at], c["nmr"][cf, at])
        assert np.array_equal(g["vqcurve_written"][cf, at], c["written"][cf, at])
        assert np.array_equal(g["vqcurve_cap_alloc"][cf, at], c["cap_alloc"][cf, at])
        assert g["vqcurve_cap"][cf, sb] == c["cap"][cf, sb]
        assert np.isposinf(g["vqcurve_nmr"][cf, at, 8:]).all() and not np.isposinf(g["vqcurve_nmr"][cf, at, :8]).all()
