"""4 to 8 channels and sample rates above 96 kHz on the CPU: the fixture tests/golden/wide.part*.npz against the oracle that
wrote it, and the conditions that make every case of tests/wide_cases.py worth having.  No GPU.

Everything is exact: bytes, int16 PCM, integers.  The float checks are conditions on the material, not comparisons:
no scalar unit on a budget tie of BitAlloc (wide_cases.budget_ties), and no unit of the rate-control cases inside the
tie window of tests/test_gpu_rate.py and tests/test_gpu_band.py (1e-4 dB) at the targets the GPU tests use, so that
those tests leave no unit out.
"""
import numpy as np
import pytest

import band_model as bm
import wide_cases as wc
import widths_cases
from oracle import pac_oracle as po


def check_case(case):
    """The conditions of a case, with no exception, on the arrays of the fixture: raises AssertionError where one
    fails."""
    sr, n_ch, _ = case
    g, tag = wc.fixture(), wc.tag_of(case)
    pcm, planted = wc.material(case)
    assert pcm.shape == (wc.N_HOPS * wc.HOP, n_ch) and pcm.dtype == np.int16
    assert str(g["sha_" + tag]) == wc.digest(pcm), "the programme is not the one the fixture was made from"
    tr = [bool(v) for v in g["tr_" + tag]]
    assert tr == wc.transients(pcm) and any(tr), tr                            # a transient hop
    flags = wc.block_flags(tr)
    drop = wc.dropped_blocks(pcm, tr)
    assert any(chs - {0} for chs in drop.values()), drop                       # a dropped hop, not by channel 0 alone
    assert any(fl[1] and f not in drop for f, fl in enumerate(flags)), (flags, drop)       # a short-coded hop that stays
    assert any(not fl[1] for fl in flags[:-1]) or planted, flags
    # ---- the band layout
    nbl, lines_l, nbs, lines_s = wc.BANDS[sr]
    long_t, short_t = po.band_table(wc.HOP, sr), po.band_table(wc.SHORT, sr)
    assert (long_t.nBands, int(long_t.nLines.sum()), short_t.nBands, int(short_t.nLines.sum())) == wc.BANDS[sr]
    assert (long_t.nLines > 0).all() and (short_t.nLines > 0).all()
    if sr > 48000:
        assert wc.HOP - lines_l > 0 and wc.SHORT - lines_s > 0                 # lines of the dummy band
    else:
        assert lines_l == wc.HOP and lines_s == wc.SHORT
    # band_stride comes from the short layout (as at every rate the suite codes at: 8 x 6 against 17 at 48 kHz); at
    # 176.4 and 192 kHz that leaves a stride of 16 slots, the narrowest there is, of which a long block uses 9
    assert wc.SUB * nbs > nbl
    if sr in (176400, 192000):
        assert (wc.SUB * nbs, nbl) == (16, 9)
    # ---- the streams
    for coder, (kbps, bs, vq, sbr) in wc.CODERS.items():
        data = wc.reference(case, coder)
        p, at = widths_cases.header(data)
        assert (p.sampleRate, p.nChannels, bool(p.useVQ), bool(p.useSBR)) == (sr, n_ch, vq, sbr)
        assert (p.sfBands.nBands, p.sfBandsShort.nBands) == (nbl, nbs)
        want = [tuple(int(v) for v in fl) for f, fl in enumerate(flags) if f not in drop] if bs else \
            [(0, 0, 0)] * wc.N_BLOCKS
        hs = widths_cases.heads(data)
        assert [h[0] for h in hs] == [fl for fl in want for _ in range(n_ch)], (coder, [h[0] for h in hs])
        assert any(int(a) for _, us in hs for u in us for a in u[1]), coder    # bits are allocated
        dec, raised = wc.decoded(case, coder)
        if sbr and sr > 48000:
            assert dec is None and raised == "IndexError", (coder, raised)
        else:
            assert raised is None and dec.dtype == np.int16, (coder, raised)
            assert dec.shape == ((wc.N_BLOCKS + 1 - (len(drop) if bs else 0)) * wc.HOP, n_ch), (coder, dec.shape)
        if not vq:
            assert not wc.budget_ties(case, coder), (coder, wc.budget_ties(case, coder))


def check_rate_case(case):
    """no unit of a rate-control case inside the tie window at the targets used; the models' arrays have the shapes of
    the case's layout"""
    sr, n_ch, _ = case
    nbl, _, nbs, _ = wc.BANDS[sr]
    stride = max(nbl, wc.SUB * nbs)
    n_cf = wc.N_BLOCKS * n_ch
    c = wc.band_curve(case)
    assert c["band_stride"] == stride and c["nmr"].shape == (n_cf, stride, bm.CAND) and c["n_cand"] == 16
    unit, _ = bm.layout(c)
    live = c["cap"] >= 0
    n_long, n_short = int((live.sum(axis=1) == 1).sum()), int((live.sum(axis=1) == wc.SUB).sum())
    assert n_long and n_short and (~live.any(axis=1)).sum() >= n_ch            # long, short and dropped channel-frames
    assert (unit >= 0).sum() == n_long * nbl + n_short * wc.SUB * nbs
    assert np.isfinite(c["nmr"][unit >= 0]).all()
    for target in wc.TARGETS:
        m = bm.margins(c, target)
        print(f"{wc.tag_of(case)} at {target:+.0f} dB: smallest band margin {m[live].min():.3g} dB")
        assert m[live].min() >= wc.WINDOW, (case, target)
    budget, capped, margin, = (wc.stored(case, "search_" + k) for k in ("budget", "capped", "margin"))
    assert budget.shape == (wc.N_BLOCKS, n_ch, wc.SUB)
    assert np.array_equal(np.isfinite(margin).reshape(n_cf, wc.SUB), live)
    print(f"{wc.tag_of(case)} at {wc.TARGETS[0]:+.0f} dB: smallest search margin {margin.min():.3g} dB, "
          f"{int(capped.sum())} of {int(live.sum())} units capped")
    assert margin.min() >= wc.WINDOW, case
    r = wc.rate_curve(case)
    assert np.array_equal(r["steps"] >= 0, live) and r["worst"].shape == (n_cf, r["row"])
    v = wc.vq_curve(case)
    v_live = v["cap"] >= 0
    assert v_live.any() and v["nmr"].shape[1:] == (stride, bm.CAND)
    for target in wc.TARGETS:
        m = bm.margins(v, target)
        print(f"{wc.tag_of(case)} gain-shape at {target:+.0f} dB: smallest band margin {m[v_live].min():.3g} dB")
        assert m[v_live].min() >= wc.WINDOW, (case, target)


# ------------------------------------------------------------------ 1. the fixture and the cases
def test_fixture_holds_the_cases():
    g = wc.fixture()
    assert [str(c) for c in g["cases"]] == [wc.tag_of(c) for c in wc.CASES]
    assert len(wc.CASES) == len({wc.tag_of(c) for c in wc.CASES}) == 10 and len(wc.STREAMS) == 40
    assert sorted((c[0], c[1]) for c in wc.CHANNEL_CASES) == [(48000, n) for n in (4, 5, 6, 8)]
    assert sorted((c[0], c[1]) for c in wc.RATE_CASES) == [(r, 2) for r in (64000, 88200, 176400, 192000)]
    assert [(c[0], c[1]) for c in wc.BOTH_CASES] == [(192000, 8), (64000, 5)]
    assert set(wc.REGENERATED) <= set(wc.CASES) and set(wc.RATE_CONTROL) <= set(wc.CASES)
    want = {"cases"} | {f"{k}_{wc.tag_of(c)}" for c in wc.CASES for k in ("sha", "tr")}
    want |= {f"pac_{coder}_{wc.tag_of(c)}" for c, coder in wc.STREAMS}
    want |= {f"{k}_{wc.tag_of(c)}" for c in wc.RATE_CONTROL for k in wc.RATE_ARRAYS}
    have = {k for k in g if not k.startswith(("dec_", "raises_"))}
    assert have == want, have ^ want
    for c, coder in wc.STREAMS:
        key = f"{coder}_{wc.tag_of(c)}"
        assert ("dec_" + key in g) != ("raises_" + key in g), key


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_case_is_worth_having(case):
    check_case(case)


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_no_unit_is_inside_the_tie_window(case):
    check_rate_case(case)


def test_planting_gives_both_properties():
    """plant() on silence-free, click-free material: a steady low noise bed in every channel"""
    rng = np.random.default_rng(9)
    pcm = rng.integers(-300, 301, (wc.N_HOPS * wc.HOP, 3)).astype(np.int16)
    assert not any(wc.transients(pcm)) and not wc.dropped_blocks(pcm) and not wc.has_both(pcm)
    assert {f for f, _, _ in wc.zero_sub_blocks(pcm)} == {0, wc.N_BLOCKS - 1}      # the zeros before and after the stream
    planted = wc.plant(pcm)
    assert wc.transients(planted) == [False, True, False, False, False]
    assert wc.dropped_blocks(planted) == {2: {1}} and wc.has_both(planted)


# ------------------------------------------------------------------ 2. two cases made again from scratch
@pytest.mark.parametrize("case", wc.REGENERATED, ids=wc.case_id)
def test_oracle_gives_the_fixture_again(case):
    g = wc.fixture()
    made = wc.case_arrays(case)
    assert len(made) == 2 + 2 * len(wc.CODERS)
    for k, v in made.items():
        assert k in g and v.dtype == g[k].dtype and np.array_equal(v, g[k]), k


def test_models_give_the_fixture_again():
    """the band curve and the budget search of the 176.4 kHz case, three channel-frames of it: a long one, a short
    one, a dropped one"""
    import rate_model as rm
    case = (176400, 2, 42_180)
    assert case in wc.RATE_CONTROL
    a = wc.rate_analysis(case)
    c = wc.band_curve(case)
    live = c["cap"] >= 0
    kinds = {1: None, wc.SUB: None, 0: None}
    for cf in range(len(live)):
        if kinds.get(int(live[cf].sum()), 0) is None:
            kinds[int(live[cf].sum())] = cf
    assert None not in kinds.values(), kinds
    for cf in kinds.values():
        f, ch = divmod(cf, 2)
        if a["units"][f] is None:
            assert np.isnan(c["nmr"][cf]).all() and not c["cap_alloc"][cf].any()
            assert not wc.stored(case, "search_budget")[f, ch].any()
            continue
        for sb, u in enumerate(a["units"][f][ch]):
            nb = u.bands.nBands
            assert np.array_equal(c["nmr"][cf, sb * nb:(sb + 1) * nb], bm.unit_curve(a["p"], u)), (cf, sb)
            assert c["cap"][cf, sb] == rm.STEP * rm.cap_steps(a, u, wc.CAP_KBPS)
            budget, capped, margin = rm.search_unit(a, u, wc.TARGETS[0], wc.CAP_KBPS)
            assert budget == wc.stored(case, "search_budget")[f, ch, sb]
            assert capped == wc.stored(case, "search_capped")[f, ch, sb]
            assert margin == wc.stored(case, "search_margin")[f, ch, sb]
