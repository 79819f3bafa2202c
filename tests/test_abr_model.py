"""The NumPy statement of coding to an average bit rate (tests/abr_model.py) holds its own invariants on synthetic
curves, and the library exports the entry points it states (include/pacx.h: pacx_rate_curve_layout,
pacx_rate_curve_batch, pacx_rate_solve).  No GPU: the library is looked at, not called."""
import os
import re

import numpy as np
import pytest

import abr_model as am
from conftest import ROOT

NEW_EXPORTS = ("pacx_rate_curve_layout", "pacx_rate_curve_batch", "pacx_rate_solve")


@pytest.fixture(scope="module")
def C():
    return am.synthetic(300, 40, 6, seed=1)


def test_vectorised_total_is_the_unit_by_unit_one(C):
    for t in (-30 * 64, -641, -1, 0, 7, 500, 30 * 64):
        tot, budget, n_bytes, capped = am.evaluate(C, t)
        assert tot == am.total_slow(C, t)
        for cf in (0, 1, 17, 150, 299):
            b, n, cap = am.frame(C, cf, t / 64)
            assert np.array_equal(budget[cf], b) and n_bytes[cf] == n and capped[cf] == cap
    dropped = (C["steps"] < 0).all(axis=1)
    assert dropped.any() and not am.evaluate(C, 0)[2][dropped].any()
    assert (am.evaluate(C, 0)[2][~dropped] > 0).all()


def test_the_synthetic_totals_are_not_monotone_in_the_unit_curves(C):
    """what the solve's header says: worst[j] is not monotone in j, so pick() is the bisection's answer only"""
    cf = int(np.argmax(C["steps"][:, 0] > 10))
    w = C["worst"][cf, :C["steps"][cf, 0] + 1]
    assert (np.diff(w) > 0).any() and (np.diff(w) < 0).any()


@pytest.mark.parametrize("share", [0.1, 0.35, 0.5, 0.8, 0.97])
def test_the_answer_fits_and_the_probe_below_it_failed(C, share):
    lo_t, hi_t = -30 * 64, 30 * 64
    small, big = am.total(C, hi_t), am.total(C, lo_t)
    assert small < big
    limit = int(small + share * (big - small))
    s = am.solve(C, limit, lo_t, hi_t)
    assert s["met"] == 1 and lo_t <= s["t"] <= hi_t
    assert s["total"] == am.total(C, s["t"]) <= limit
    assert s["total"] == int(np.sum(s["n_bytes"][s["n_bytes"] > 0] + 4))
    below = [(t, tot) for t, tot in s["path"] if t < s["t"]]
    assert below and max(below)[1] > limit                   # the largest t tried below the answer did not fit
    assert all(tot <= limit for t, tot in s["path"] if t == s["t"])
    assert len(s["path"]) + 1 <= am.pairs(lo_t, hi_t)         # the probes and the writing pick fit the fixed launches


def test_edges(C):
    lo_t, hi_t = -20 * 64, 20 * 64
    small, big = am.total(C, hi_t), am.total(C, lo_t)
    # unreachable: not even the highest target fits
    s = am.solve(C, small - 1, lo_t, hi_t)
    assert (s["met"], s["t"], s["total"]) == (0, hi_t, small) and len(s["path"]) == 1
    # the limit is exactly the smallest total
    s = am.solve(C, small, lo_t, hi_t)
    assert s["met"] == 1 and s["total"] <= small
    # everything fits at the lowest target (total is not monotone: take a limit above every total on the path)
    s = am.solve(C, 10 * big, lo_t, hi_t)
    assert (s["met"], s["t"], s["total"]) == (1, lo_t, big)
    # limit == total(t) exactly, at a t the bisection reaches
    ref = am.solve(C, (small + big) // 2, lo_t, hi_t)
    s = am.solve(C, ref["total"], lo_t, hi_t)
    assert s["met"] == 1 and s["total"] <= ref["total"]
    if s["t"] == ref["t"]:
        assert s["total"] == ref["total"]
    # one point on the grid
    s = am.solve(C, 10 * big, 5, 5)
    assert (s["met"], s["t"]) == (1, 5) and len(s["path"]) == 1
    # no channel-frames
    empty = {"worst": np.zeros((0, C["row"])), "bits": np.zeros((0, C["row"]), np.int32),
             "steps": np.zeros((0, 8), np.int32), "row": C["row"], "sub_stride": C["sub_stride"]}
    s = am.solve(empty, 0, lo_t, hi_t)
    assert (s["met"], s["t"], s["total"]) == (1, lo_t, 0)


def test_pairs():
    assert am.pairs(5, 5) == 3 and am.pairs(0, 2) == 4 and am.pairs(-1920, 1920) == 2 + 12


def test_pick():
    w = np.array([9.0, 1.0, 8.0, 7.0, 2.0, 1.5, 0.5])
    assert am.pick(w, 6, 0.0) == (6, True)                   # the cap misses the target
    assert am.pick(w, 6, 0.5) == (6, False)
    assert am.pick(w, 6, 2.0) == (4, False)                  # the bisection's answer, not the global one (j = 1)
    assert am.pick(w, 6, 100.0) == (0, False)
    assert am.pick(np.array([np.nan]), 0, 0.0) == (0, True)
    assert am.pick(np.array([3.0]), 0, 3.0) == (0, False)    # J = 0: one budget, 0 bits


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
    assert "PACX_RATE_TARGET_GRID" in header and a._lib.RATE_TARGET_GRID == am.GRID == 64
    assert lib.pacx_abi_version() == 7                 # additive: no caller breaks
