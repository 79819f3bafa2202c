"""tests/mask_cases.py on the CPU: every constructed block is what it claims to be, from the oracle alone, with zero
exceptions (seeds and dither were chosen until that held), so that tests/test_gpu_mask_cases.py cannot pass by accident:

* every peak decision of every block is made by the signal, not by the rounding of an FFT;
* each family has the property it was built for (peak counts, the kept/dropped partition, delta, the crossing line);
* where a wrong skip is to be seen, the oracle's own threshold moves by far more than the 1e-9 dB bar when the masker
  in question is left out;
* an int16 rendering keeps the property it is listed with.
"""
import numpy as np
import pytest

import mask_cases as mc
from oracle import pac_oracle as po

CASES = mc.cases()
IDS = [c.name for c in CASES]
SIGNAL_DECIDED = 1e-10     # FFT rounding moves an intensity by ~5e-15 of sqrt(I * max I): four orders of magnitude


def renderings(case):
    return [("f64", case.x)] + ([("i16", mc.rendered(case))] if case.i16 else [])


def family(letter):
    sel = [c for c in CASES if c.family == letter]
    return pytest.mark.parametrize("case", sel, ids=[c.name for c in sel])


def test_the_families_are_all_there():
    names = set(IDS)
    assert {c.family for c in CASES} == set("abcdef")
    assert {"a_full_low", "a_full_high", "a_full_i16", "a_full_even"} <= names
    assert {f"b_kept_{n}" for n in (1, 63, 64, 65, 128, 129)} <= names
    for tag in ("below_adjacent", "above_adjacent", "below_far", "p_first", "p_last"):
        assert {f"c_{tag}_{d:+.0e}" for d in mc.DELTAS} <= names
    for tag in ("below_last", "below_first", "above_first", "short_above_first"):
        assert {f"d_{tag}_{s * e:+.0e}" for e in mc.EPSILONS for s in (1, -1)} <= names
    assert {c.sr for c in CASES if c.family == "c"} == {44100, 48000} == {c.sr for c in CASES if c.family == "d"}
    assert any(c.short for c in CASES if c.family == "d") and any(c.short for c in CASES if c.family == "f")
    for c in CASES:
        assert c.x.dtype == np.float64 and c.x.shape == (2048,)
        if c.i16:
            assert np.max(np.abs(c.x)) < 1.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_peak_is_decided_by_the_signal(case):
    for tag, x in renderings(case):
        for sb, blk in enumerate(mc.blocks_of(case, x)):
            inten = po.sidechain_intensity(blk)
            if not inten.any():
                continue                                   # digital silence: no peak, nothing to decide
            need = SIGNAL_DECIDED * np.sqrt(np.maximum(inten[1:], inten[:-1]) * np.max(inten))
            short_of = np.nonzero(np.abs(np.diff(inten)) < need)[0]
            assert len(short_of) == 0, (case.name, tag, sb, short_of[:5] + 1)


def test_threshold_helper_is_the_oracles():
    for name in ("b_kept_64", "c_below_far_+2e-04", "e_loud_in_batch"):
        c = mc.by_name(name)
        want = po.masked_threshold(c.x.copy(), 1024, c.sr)
        assert np.array_equal(mc.threshold(mc.analyse(c.x, c.sr), 1024, c.sr), want)


# ------------------------------------------------------------------ a
@family("a")
def test_full_peak_lists(case):
    an = mc.analyse(case.x, case.sr)
    if "n_peaks" in case.prop:
        assert len(an.bins) == case.prop["n_peaks"] == 512
        assert (an.bins[0], an.bins[-1]) == (case.prop["first_bin"], case.prop["last_bin"])
        if case.prop["all_below_40"]:
            assert np.all(an.spl + mc.SPL_BAND <= 40.0)                  # every one may be pruned ...
            dropped, kept = mc.pruning_partition(an, case.sr)
            assert dropped.sum() >= 64 and kept.sum() >= 64              # ... and many are, many are not
        else:
            assert np.all(an.spl - mc.SPL_BAND > 40.0)                   # none may: eight full batches for k_mask
            assert mc.pruning_partition(an, case.sr)[1].all()
    if case.i16:
        an16 = mc.analyse(mc.rendered(case), case.sr)
        assert len(an16.bins) >= case.prop["n_peaks_min"] >= 500
    # the comb's tones stand ~120 dB above its dither: a rendering cannot hold more peaks than the list does
    assert len(an.bins) <= 512


def test_peaks_at_the_ends_of_the_spectrum():
    assert mc.analyse(mc.by_name("a_full_low").x, mc.SR).bins[0] == 1          # compared with bin 0
    assert mc.analyse(mc.by_name("a_full_even").x, mc.SR).bins[-1] == 1024     # compared with its left neighbour only


# ------------------------------------------------------------------ b
@family("b")
def test_kept_maskers_are_certain(case):
    n = case.prop["n_kept"]
    for tag, x in renderings(case):
        an = mc.analyse(x, case.sr)
        dropped, kept = mc.pruning_partition(an, case.sr)
        assert np.array_equal(kept, an.spl > 40.0), (case.name, tag)      # the n tones and nothing else
        assert kept.sum() == n, (case.name, tag, kept.sum())
        assert np.array_equal(dropped, ~kept), (case.name, tag, np.nonzero(~dropped & ~kept)[0])
        if "n_peaks" in case.prop:
            assert len(an.bins) == case.prop["n_peaks"]
        else:
            assert len(an.bins) > n                                       # the pruning has something to drop


def test_pruning_partition_reads_the_bounds_both_ways():
    """two tones 27 dB/Bark apart to within the bounds' width are neither kept nor dropped for certain"""
    c = mc.by_name("c_below_adjacent_+2e-04")
    an = mc.analyse(c.x, c.sr)
    dropped, kept = mc.pruning_partition(an, c.sr)
    p = mc.ordinal(an, c.prop["p_bin"])
    assert not dropped[p] and not kept[p]
    assert kept[mc.ordinal(an, c.prop["q_bin"])]


# ------------------------------------------------------------------ c
@family("c")
def test_dominance_margin(case):
    assert not case.i16                                    # rounding to int16 moves an SPL by ~3e-3 dB
    an = mc.analyse(case.x, case.sr)
    p, q = mc.ordinal(an, case.prop["p_bin"]), mc.ordinal(an, case.prop["q_bin"])
    delta = case.prop["delta"]
    assert abs(mc.delta_of(an, p, q) - delta) <= 1e-9
    assert an.spl[p] + mc.SPL_BAND <= 40.0                 # p is open to pruning at all
    if p > q:
        assert an.spl[q] + mc.SPL_BAND <= 40.0             # upward, the rule is tight only with both slopes at -27
    assert abs(p - q) >= case.prop["apart"] and (case.prop["apart"] > 1 or abs(p - q) == 1)
    if case.prop["apart"] >= 64:
        assert p // 8 != q // 8                            # eight peaks a lane: the cross-lane scan decides
    if "p_ordinal" in case.prop:
        assert p == case.prop["p_ordinal"] % len(an.bins)
        assert len(an.bins) > 64                           # and the list runs over several lanes
    # no third masker decides the matter: without q, p is out of everyone's reach
    others = [i for i in range(len(an.bins)) if i not in (p, q)]
    assert np.max(an.spl[others] - 27.0 * np.abs(an.z[others] - an.z[p])) < an.spl[p] - 1.0
    full, without = mc.threshold(an, 1024, case.sr), mc.threshold(an, 1024, case.sr, without=(p,))
    dropped, _ = mc.pruning_partition(an, case.sr)
    slack = mc.bound_slack(an, case.sr, p)
    if delta > 0:
        # the bound rule may not drop p, and is at most 0.6 dB from doing so (p_first: 5.5 dB, a bin is 0.2 Bark there)
        assert not dropped[p]
        assert 0.0 < slack - delta < (6.0 if case.prop.get("p_ordinal") == 0 else 0.6)
        # sensitivity: a kernel that drops p is off by delta, 1e4 bars and more
        assert np.max(full - without) >= 1e-5
        assert np.max(full - without) >= 0.99 * delta
    else:
        assert np.array_equal(full, without)               # dominated: either decision gives the oracle's threshold


# ------------------------------------------------------------------ d
@family("d")
def test_chunk_screen_edge(case):
    assert not case.i16
    eps, line, j = case.prop["eps"], case.prop["line"], case.prop["chunk"]
    n_lines = 128 if case.short else 1024
    blk = mc.blocks_of(case)[case.prop["sub_block"]]
    an = mc.analyse(blk, case.sr)
    t = mc.ordinal(an, case.prop["tone_bin"])
    z, quiet = mc.line_tables(n_lines, case.sr)
    chunk = slice(64 * j, 64 * j + 64)
    assert line in (64 * j, 64 * j + 63)
    assert np.argmin(quiet[chunk]) + 64 * j == line        # the screen's `lowest quiet of the chunk` is this line's
    full = mc.threshold(an, n_lines, case.sr)
    curve = po.masker_curve_spl(an.f[t], an.spl[t], z)
    slope = -27.0 + 0.367 * max(an.spl[t] - 40.0, 0.0)
    assert slope <= 0.0                                    # the screen proper, not the loud-masker escape
    if eps > 0:
        over = np.nonzero(full[chunk] > quiet[chunk])[0] + 64 * j
        assert over.tolist() == [line]                     # only this line
        assert abs((full[line] - quiet[line]) - eps) <= 1e-6
        without = mc.threshold(an, n_lines, case.sr, without=(t,))
        assert full[line] - without[line] >= 0.5 * eps     # sensitivity: skipping the tone here shows
        assert np.array_equal(without[chunk], quiet[chunk])
    else:
        assert np.array_equal(full[chunk], quiet[chunk])   # the mirror: quiet everywhere in the chunk
        assert np.argmax((curve - quiet)[chunk]) + 64 * j == line
        assert abs((curve - quiet)[line] - eps) <= 1e-6
    # the tone is no masker for the chunk by a hair only: a few lines further (towards it) it is
    assert np.any(full > quiet + 1.0)


# ------------------------------------------------------------------ e
@family("e")
def test_loud_maskers(case):
    assert not case.i16 and np.max(np.abs(case.x)) > 1.0   # reachable through float64 views only
    an = mc.analyse(case.x, case.sr)
    loud = mc.ordinal(an, case.prop["loud_bin"])
    assert an.spl[loud] > case.prop["min_spl"] + 1.0
    assert -27.0 + 0.367 * (an.spl[loud] - 40.0) > 0.5     # its curve RISES above it
    assert np.sum(an.spl > case.prop["min_spl"]) == 1
    thr = mc.threshold(an, 1024, case.sr)
    assert thr[-1] > an.spl[loud] + 50.0                   # and goes on rising to the last line
    if "quiet_tones" in case.prop:
        dropped, kept = mc.pruning_partition(an, case.sr)
        first = np.nonzero(~dropped)[0][:64]               # the first batch holds at most these
        assert loud in first
        assert np.sum((an.spl[first] > 40.0) & (an.spl[first] < 100.0)) == case.prop["quiet_tones"]
        assert np.sum(~dropped) <= 64                      # one batch: b_slope > 0 for all that is kept


# ------------------------------------------------------------------ f
def test_short_frame_sub_blocks():
    case = mc.by_name("f_short_mixed")
    for tag, x in renderings(case):
        counts = [len(mc.analyse(blk, case.sr).bins) for blk in mc.blocks_of(case, x)]
        assert counts[case.prop["full_sub_block"]] == 64, (tag, counts)     # the short side chain's list is full
        for sb in case.prop["silent_sub_blocks"]:
            assert counts[sb] == 0 and not mc.blocks_of(case, x)[sb].any()
        an = mc.analyse(mc.blocks_of(case, x)[case.prop["tone_sub_block"]], case.sr)
        assert np.sum(an.spl > 40.0) == 1 and np.sort(an.spl)[-2] < 0.0     # one tone over dither
    silent = mc.by_name("f_long_silent")
    assert not silent.x.any() and not mc.as_int16(silent.x).any()
    assert np.array_equal(po.masked_threshold(silent.x.copy(), 1024, silent.sr), mc.line_tables(1024, silent.sr)[1])


def test_int16_renderings_are_exact_codes():
    for c in CASES:
        if c.i16:
            codes = mc.as_int16(c.x)
            assert np.max(np.abs(codes.astype(np.int64))) < 32768 and codes.min() > -32768
            assert np.array_equal(po.pcm16_to_fraction(codes), mc.rendered(c))
