"""The NMR model (tests/nmr_model.py) and the host arithmetic of quality.Report, without a GPU:
the hop-to-record map against what the oracle's writer wrote, the measure rising as the bit rate falls,
histogram / percentile / share against a NumPy sort."""
import numpy as np
import pytest

import nmr_model as nm
from conftest import EXCERPTS, load_excerpt
from oracle import pac_oracle as po


def padded(pcm):
    n = -len(pcm) % 1024
    return np.concatenate((pcm, np.zeros((n, pcm.shape[1]), pcm.dtype))) if n else pcm


def check_map(pcm, sr, block_switching):
    collect = []
    data = po.encode_stream(pcm, sr, 128, block_switching, collect=collect)
    flags, rec, n_rec = nm.record_map(pcm, block_switching)
    assert [tuple(map(bool, f)) for f in flags] == [tuple(map(bool, f)) for f, _ in collect]
    assert [r < 0 for r in rec] == [parts is None for _, parts in collect]
    recs, _ = nm.records(data)
    assert n_rec == len(recs)
    return rec


@pytest.mark.parametrize("name", EXCERPTS)
def test_record_map_on_excerpts(name):
    """flags and record counts of the golden .pac files (written by the reference) and of the oracle's writer"""
    ex = load_excerpt(name)
    pcm = padded(ex["pcm"])
    for variant, bs in (("long", False), ("bs", True)):
        flags, rec, n_rec = nm.record_map(pcm, bs)
        assert [list(map(int, f)) for f in flags[:-1]] == ex[f"flags_{variant}"].tolist()
        recs, _ = nm.records(bytes(ex[f"pac_{variant}"]))
        assert n_rec == len(recs)
    check_map(pcm[:8 * 1024], int(ex["sr"]), True)


def test_record_map_with_a_dropped_hop():
    """a click after silence: the short-coded hop behind it has all-zero sub-blocks and never reaches the file"""
    rng = np.random.default_rng(5)
    pcm = np.zeros((6 * 1024, 2), np.int16)
    pcm[1024:2048] = rng.integers(-3000, 3000, (1024, 2))
    pcm[3 * 1024 + 900:4 * 1024] = rng.integers(-30000, 30000, (124, 2))     # hop 3: a burst, zeros before it
    pcm[4 * 1024:] = rng.integers(-3000, 3000, (2 * 1024, 2))
    rec = check_map(pcm, 48000, True)
    assert any(r < 0 for r in rec)
    m = nm.model(pcm, po.encode_stream(pcm, 48000, 128, True), True)
    gone = [f for f, r in enumerate(rec) if r < 0]
    assert np.all(np.isnan(m["nmr_db"][gone])) and not np.all(np.isnan(m["nmr_db"][0]))


@pytest.mark.parametrize("name", EXCERPTS)
def test_model_rises_as_the_rate_falls(name):
    ex = load_excerpt(name)
    pcm = padded(ex["pcm"])
    hi = nm.model(pcm, bytes(ex["pac_long"]), False)["nmr_db"]
    lo = nm.model(pcm, bytes(ex["pac_long96"]), False)["nmr_db"]
    assert np.nanmedian(lo) > np.nanmedian(hi)
    assert np.mean(lo[~np.isnan(lo)] > 0) >= np.mean(hi[~np.isnan(hi)] > 0)


def test_report_arithmetic_against_a_sort():
    """Report from arrays alone: counts, bins, maxima, share and percentiles against NumPy on random values that
    reach both ends of the histogram"""
    import audio_codec_amd as A
    q = A.quality
    rng = np.random.default_rng(11)
    nbl, nbs, stride = 25, 6, 48
    hops, n_ch = 40, 2
    short = rng.random(hops) < 0.3
    nmr = np.full((hops, n_ch, stride), np.nan)
    for f in range(hops):
        n = 8 * nbs if short[f] else nbl
        nmr[f, :, :n] = rng.normal(-20, 18, (n_ch, n))
    nmr[0, 0, 0], nmr[1, 0, 1] = -500.0, 77.25                  # underflow and overflow bins
    nmr[2] = np.nan                                             # a block without a payload
    rep = q.Report(nmr, nmr, nmr, short, nbl, nbs)
    s = rep.summary
    for kind, sel, nb, per in ((0, ~short, nbl, 1), (1, short, nbs, 8)):
        for b in range(nb):
            v = nmr[sel][:, :, :per * nb].reshape(-1, per, nb)[:, :, b].ravel()
            v = np.sort(v[~np.isnan(v)])
            assert s.count[kind, b] == len(v) and s.audible[kind, b] == np.sum(v > 0) and s.max[kind, b] == v[-1]
            assert s.hist[kind, b].sum() == len(v)
            assert s.hist[kind, b, 0] == np.sum(v < -120) and s.hist[kind, b, -1] == np.sum(v >= 40)
            inner = v[(v >= -120) & (v < 40)]
            assert np.array_equal(s.hist[kind, b, 1:-1], np.histogram(inner, bins=320, range=(-120, 40))[0])
            for pct in (10, 50, 90):
                want = v[max(int(np.ceil(pct / 100 * len(v))), 1) - 1]
                if -120 <= want < 40:
                    assert abs(rep.percentile(pct, kind, b) - want) <= 0.5
    allv = np.sort(nmr[~np.isnan(nmr)])
    assert rep.share_audible() == np.sum(allv > 0) / len(allv)
    for pct in (1, 25, 50, 75, 99):
        assert abs(rep.percentile(pct) - allv[int(np.ceil(pct / 100 * len(allv))) - 1]) <= 0.5
    assert rep.percentile(0) == -120.0 and rep.percentile(100) == 77.25 and rep.maximum() == 77.25
    assert rep.median() == rep.percentile(50)
    # the library's words and back
    words = np.zeros((2, 32, A._lib.NMR_SUMMARY_WORDS), np.uint64)
    words[:, :, 0], words[:, :, 1], words[:, :, 3:] = s.count, s.audible, s.hist
    bits = np.where(np.isnan(s.max), 0.0, s.max).view(np.uint64)
    key = np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))
    words[:, :, 2] = np.where(np.isnan(s.max), np.uint64(0), key)
    assert q.Summary.from_words(words) == s
    assert q.Summary.from_words(words.view(np.int64)) == s


def test_quality_map_helpers_equal_the_model():
    """the host side of quality.nmr_of_file's hop-to-record map (flag shifting, dropped hops, record numbers)
    against the model's, given the detector's decisions"""
    import audio_codec_amd as A
    q = A.quality
    rng = np.random.default_rng(5)
    pcm = np.zeros((6 * 1024, 2), np.int16)
    pcm[1024:2048] = rng.integers(-3000, 3000, (1024, 2))
    pcm[3 * 1024 + 900:4 * 1024] = rng.integers(-30000, 30000, (124, 2))
    pcm[4 * 1024:] = rng.integers(-3000, 3000, (2 * 1024, 2))
    for p, drops in ((pcm, 1), (load_excerpt("castanet")["pcm"][:32 * 1024], 0)):
        flags, rec, n_rec = nm.record_map(p, True)
        packed = q.flags_from_transients([f[2] for f in flags[:len(p) // 1024]])
        assert packed.tolist() == [int(a) + 2 * int(b) + 4 * int(c) for a, b, c in flags]
        gone = q.dropped_blocks(q.padded_stream(p), packed)
        assert int(gone.sum()) == drops
        got, n_got = q.record_map(packed, gone, p.shape[1])
        assert got.tolist() == rec and n_got == n_rec
