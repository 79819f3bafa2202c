"""An average for the stream, a peak per segment (tests/peak_model.py over segment_model and the plain models): what the
definition of include/pacx.h (pacx_rate_solve_peak / pacx_band_solve_peak) implies, on synthetic curves; the library
exports the two entry points; and what pacfile.encode_stream_abr refuses before any GPU work.  No GPU: the library is
looked at, not called."""
import os
import re

import numpy as np
import pytest

import peak_model as pm
import segment_model as sm
from conftest import ROOT

NEW_EXPORTS = ("pacx_rate_solve_peak", "pacx_band_solve_peak")
KINDS = ("band", "rate")
T_LO, T_HI = -30 * 64, 30 * 64
HUGE = 10 ** 12


def plain(kind, c, limit, t_lo=T_LO, t_hi=T_HI):
    return sm.solve_segments(kind, c, [0, sm.n_cf_of(kind, c)], [limit], t_lo, t_hi)


@pytest.mark.parametrize("kind", KINDS)
def test_peaks_that_never_bind_give_the_plain_solve(kind):
    c, first, _ = sm.material(kind)
    small, big = sm.total(kind, c, T_HI), sm.total(kind, c, T_LO)
    for limit in ((small + big) // 2, small - 1, small, HUGE):
        got, ref = pm.solve_peak(kind, c, first, [HUGE] * (len(first) - 1), limit), plain(kind, c, limit)
        assert (got["floor"] == T_LO).all() and got["met"].all()
        assert (got["t_stream"], got["met_stream"], got["total_stream"]) == (ref["t"][0], ref["met"][0], ref["total"][0])
        assert (got["t"] == ref["t"][0]).all() and got["total"].sum() == ref["total"][0]
        for k in sm.PER_CF[kind]:
            assert np.array_equal(got[k], ref[k]), (limit, k)


@pytest.mark.parametrize("kind", KINDS)
def test_a_limit_that_never_binds_gives_the_segmented_solve(kind):
    c, first, peaks = sm.material(kind)
    got, ref = pm.solve_peak(kind, c, first, peaks, HUGE), sm.solve_segments(kind, c, first, peaks)
    assert (got["t_stream"], got["met_stream"]) == (T_LO, 1) and got["total_stream"] == ref["total"].sum()
    for k in ("t", "met", "total") + sm.PER_CF[kind]:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["floor"], ref["t"])


@pytest.mark.parametrize("kind", KINDS)
def test_the_shared_material(kind):
    """what the GPU tests compare against: at the four stream limits T_s = max(t*, u_s), pinned and unpinned segments,
    totals recomputed from n_bytes, met measured at the final target"""
    c, first, peaks = sm.material(kind)
    u = pm.floors(kind, c, first, peaks)
    limits = pm.stream_limits(kind, c, first, peaks)
    assert limits[0] > limits[2] == limits[1] + 1
    seen = []
    for i, limit in enumerate(limits):
        got = pm.solve_peak(kind, c, first, peaks, limit)
        assert np.array_equal(got["floor"], u)
        assert np.array_equal(got["t"], np.maximum(got["t_stream"], u))
        assert got["met_stream"] == (0 if i == 1 else 1) and got["total_stream"] == got["total"].sum()
        assert (got["total_stream"] <= limit) == bool(got["met_stream"])
        if i in (1, 2):
            assert got["t_stream"] == T_HI and (got["t"] == T_HI).all()
        if i == 3:
            assert got["t_stream"] == T_LO
        for s, (a, b) in enumerate(zip(first, first[1:])):
            n = got["n_bytes"][a:b].astype(np.int64)
            assert int(np.sum(n[n > 0] + 4)) == got["total"][s], s
            assert got["met"][s] == (got["total"][s] <= peaks[s]), s
            if a == b:
                assert (got["floor"][s], got["t"][s], got["met"][s], got["total"][s]) == (T_LO, got["t_stream"], 1, 0), s
        seen.append(got)
    mid = seen[0]
    pinned = mid["t"] > mid["t_stream"]
    print(f"{kind}: t* {mid['t_stream']}, {int(pinned.sum())} of {len(pinned)} segments pinned, "
          f"{int((mid['met'] == 0).sum())} beyond their peak")
    assert T_LO < mid["t_stream"] < T_HI and 0 < pinned.sum() < len(pinned)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_cases(kind):
    c = sm.synthetic(kind, 40, 3)
    c0 = sm.slice_curve(kind, c, 0, 0)
    got = pm.solve_peak(kind, c0, [0, 0, 0, 0], [0, 5, HUGE], 0, -2 * 64, 352)
    assert (got["t_stream"], got["met_stream"], got["total_stream"]) == (-2 * 64, 1, 0)
    assert (got["floor"] == -2 * 64).all() and (got["t"] == -2 * 64).all() and got["met"].all() and not got["total"].any()
    first = [0, 0, 20, 20, 40]                                  # empty segments beside full ones
    peaks = sm.limits_for(kind, c, first)
    got = pm.solve_peak(kind, c, first, peaks, pm.stream_limits(kind, c, first, peaks)[0])
    for s in (0, 2):
        assert (got["floor"][s], got["t"][s], got["met"][s], got["total"][s]) == (T_LO, got["t_stream"], 1, 0)


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
    for name in ("rate_solve_peak", "band_solve_peak"):
        assert callable(getattr(a.engine.Encoder, name))


def test_peak_kernels_use_no_scratch():
    """the compiler's resource report of both instances of the pick kernels and of the second level's own"""
    import importlib
    res = importlib.import_module("audio_codec_amd.build").resources()
    want = {"k_solve_pick<false>", "k_solve_pick<true>", "k_band_pick_seg<false>", "k_band_pick_seg<true>", "k_peak_init",
            "k_peak_step", "k_peak_finish"}
    mine = {k: v for k, v in res.items() if any(n in k for n in want)}
    assert {n for n in want if any(n in k for k in mine)} == want
    for name, r in mine.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_what_encode_stream_abr_refuses_before_any_gpu_work():
    """no GPU here: anything that got past these checks would fail otherwise, at the handle"""
    import audio_codec_amd as a
    pcm = np.zeros((4096, 2), np.int16)
    abr = a.pacfile.encode_stream_abr
    with pytest.raises(ValueError, match="peak_kbps_per_channel goes with segment_hops"):
        abr(pcm, 44100, kbps_per_channel=96, peak_kbps_per_channel=128)
    with pytest.raises(ValueError, match="peak_kbps_per_channel goes with segment_hops"):
        a.quality.encode_stream_to_rate(pcm, 44100, max_bytes=50000, peak_kbps_per_channel=128)
    for bad in (0, -128, float("nan")):
        with pytest.raises(ValueError, match="peak_kbps_per_channel must be positive"):
            abr(pcm, 44100, kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=bad)
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match="segment_hops"):
            abr(pcm, 44100, kbps_per_channel=96, segment_hops=bad, peak_kbps_per_channel=128)
