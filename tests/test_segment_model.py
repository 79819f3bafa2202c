"""One target per stretch of a stream (tests/segment_model.py over band_model / abr_model): the invariants of a solve
whose constraint is local, on synthetic curves; the arithmetic of pacfile.segment_limits; and the library exports the
two entry points (include/pacx.h: pacx_rate_solve_segments, pacx_band_solve_segments).  No GPU: the library is looked
at, not called."""
import os
import re

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import segment_model as sm
from conftest import ROOT

NEW_EXPORTS = ("pacx_rate_solve_segments", "pacx_band_solve_segments")
KINDS = ("band", "rate")
N_CF = 3000


def plain(kind, c, limit, t_lo=-30 * 64, t_hi=30 * 64):
    return (bm.solve if kind == "band" else am.solve)(c, limit, t_lo, t_hi)


def same(kind, got, ref, a=0, b=None):
    """the per-cf outputs of `got` over [a, b) against a plain solve of that slice"""
    return all(np.array_equal(np.asarray(got[k])[a:b], np.asarray(ref[k])) for k in sm.PER_CF[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_one_segment_is_the_plain_solve(kind):
    c = sm.synthetic(kind, N_CF, 3)
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    for limit in ((small + big) // 2, small - 1, small, 10 ** 12):
        got, ref = sm.solve_segments(kind, c, [0, N_CF], [limit]), plain(kind, c, limit)
        assert (int(got["t"][0]), int(got["met"][0]), int(got["total"][0])) == (ref["t"], ref["met"], ref["total"])
        assert same(kind, got, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_the_shared_material(kind):
    """what the GPU tests compare against: met and unmet segments, many targets, both ends of the range; totals
    recomputed from n_bytes; empty segments; every limit kept or known to be out of reach"""
    c, first, limits = sm.material(kind)
    assert len(limits) == 57 and (np.diff(first) == 0).sum() >= 5
    got = sm.solve_segments(kind, c, first, limits)
    met = got["met"].astype(bool)
    assert 0.5 < met.mean() < 0.95 and len(set(got["t"].tolist())) >= 10
    assert got["t"].min() == -30 * 64 and got["t"].max() == 30 * 64
    for s, (a, b) in enumerate(zip(first, first[1:])):
        n = got["n_bytes"][a:b].astype(np.int64)
        assert int(np.sum(n[n > 0] + 4)) == got["total"][s], s
        if a == b:
            assert (got["t"][s], got["met"][s], got["total"][s]) == (-30 * 64, 1, 0), s
        assert (got["total"][s] <= limits[s]) == bool(met[s]), s
        if not met[s]:
            assert got["t"][s] == 30 * 64, s
    if kind == "band":                                    # the issue's figures for this curve
        assert abs(met.mean() - 0.75) < 0.01 and len(set(got["t"].tolist())) == 17


@pytest.mark.parametrize("kind", KINDS)
def test_other_ranges(kind):
    c, first, _ = sm.material(kind)
    for t_lo, t_hi in ((-2 * 64, 352), (5, 5)):
        limits = sm.limits_for(kind, c, first, t_lo, t_hi)
        got = sm.solve_segments(kind, c, first, limits, t_lo, t_hi)
        assert got["t"].min() >= t_lo and got["t"].max() <= t_hi
        empty = np.diff(first) == 0
        assert (got["t"][empty] == t_lo).all() and (got["met"][empty] == 1).all() and (got["total"][empty] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_refining_a_partition_changes_no_segment_that_is_kept(kind):
    c, first, limits = sm.material(kind, seed=11)
    got = sm.solve_segments(kind, c, first, limits)
    # cut every third segment of two or more frames in two; the halves get limits of their own
    fine_first, fine_limits, kept = [0], [], []
    for s, (a, b) in enumerate(zip(first, first[1:])):
        if s % 3 == 0 and b - a >= 2:
            mid = int(a + (b - a) // 2)
            fine_first += [mid, int(b)]
            fine_limits += [int(limits[s]) // 2, int(limits[s]) - int(limits[s]) // 2]
        else:
            kept.append((s, len(fine_limits)))
            fine_first.append(int(b))
            fine_limits.append(int(limits[s]))
    assert len(fine_limits) > len(limits) and len(kept) > 30
    fine = sm.solve_segments(kind, c, fine_first, fine_limits)
    for s, f in kept:
        assert (got["t"][s], got["met"][s], got["total"][s]) == (fine["t"][f], fine["met"][f], fine["total"][f]), s
        a, b = int(first[s]), int(first[s + 1])
        for k in sm.PER_CF[kind]:
            assert np.array_equal(got[k][a:b], fine[k][a:b]), (s, k)


def test_segment_limits():
    """pacfile.segment_limits: the whole-stream convention per segment"""
    import audio_codec_amd as a
    fn = a.pacfile.segment_limits
    whole = lambda kbps, n_ch, sr, blocks: int(np.floor(kbps * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))   # noqa: E731
    for kbps, n_ch, sr, blocks, hops in ((96, 2, 44100, 26, 8), (128, 1, 48000, 26, 5), (96.5, 3, 96000, 7, 1),
                                         (64, 2, 44100, 26, 13), (96, 2, 44100, 26, 26), (96, 2, 44100, 26, 1000)):
        first, count, limit = fn(kbps, n_ch, sr, blocks, hops)
        assert first.tolist() == list(range(0, blocks, hops)) and count.sum() == blocks
        assert (count[:-1] == hops).all() and 1 <= count[-1] <= hops
        assert [int(v) for v in limit] == [whole(kbps, n_ch, sr, int(c)) for c in count]
        assert limit.sum() <= whole(kbps, n_ch, sr, blocks)
        assert limit.sum() > whole(kbps, n_ch, sr, blocks) - len(limit)              # each floor loses less than a byte
        if hops >= blocks:
            assert len(limit) == 1 and limit[0] == whole(kbps, n_ch, sr, blocks)
    first, count, limit = fn(96, 2, 44100, 26, 8)                                    # a last short segment
    assert count.tolist() == [8, 8, 8, 2] and limit[3] < limit[0]
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="segment_hops"):
            fn(96, 2, 44100, 26, bad)
    with pytest.raises(ValueError, match="kbps_per_channel"):
        fn(0, 2, 44100, 26, 8)


def test_library_exports_the_entry_points():
    """fails on a tree without the feature"""
    import audio_codec_amd as a
    lib = a.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pacx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in pacx.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in a._lib.SIGNATURES, name
    assert lib.pacx_abi_version() == 7                 # additive: no caller breaks
    for name in ("rate_solve_segments", "band_solve_segments"):
        assert callable(getattr(a.engine.Encoder, name))


def test_segment_kernels_use_no_scratch():
    """the compiler's resource report of the solve's kernels: no scratch, no spilled registers"""
    import importlib
    res = importlib.import_module("audio_codec_amd.build").resources()
    want = {"k_solve_pick", "k_solve_init", "k_solve_step", "k_band_pick_seg"}
    mine = {k: v for k, v in res.items() if any(n in k for n in want)}
    assert {n for n in want if any(n in k for k in mine)} == want
    for name, r in mine.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
