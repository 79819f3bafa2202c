"""The NumPy statement of the band-by-band allocation (tests/band_model.py) holds its own invariants on synthetic
curves -- non-monotone band rows and NaN included -- and the library exports the entry points it states
(include/pacx.h: pacx_band_curve_batch, pacx_band_pick, pacx_band_solve, pacx_encode_pack_alloc_batch).  No GPU: the
library is looked at, not called."""
import os
import re

import numpy as np
import pytest

import band_model as bm
from conftest import ROOT

NEW_EXPORTS = ("pacx_band_curve_batch", "pacx_band_pick", "pacx_band_solve", "pacx_encode_pack_alloc_batch")


@pytest.fixture(scope="module")
def C():
    """caps so wide that no unit exceeds them, no NaN: nothing is capped above the rows' worst values"""
    return bm.synthetic(120, seed=1, p_nan=0.0, p_dead=0.0, cap_scale=4.0)


@pytest.fixture(scope="module")
def K():
    """ordinary caps and a few NaN: all three kinds of capped unit occur"""
    return bm.synthetic(120, seed=2)


def row(*v):
    r = np.full(bm.CAND, 50.0)
    r[:len(v)] = v
    return r[None, :]


# ------------------------------------------------------------------ the pick
def test_pick_is_the_ascending_scans_first_pass():
    one = np.array([10])
    # NMR rises again at 4 bits: a bisection between 0 and 16 bits would look at the middle and never see 3 bits
    r = row(9.0, 5.0, 1.0, 6.0, 7.0, 8.0, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0, -1.0, -2.0, -3.0, -4.0)
    a, capped, missed, over = bm.pick(r, one, 10_000, np.array([0]), 2.0, 16)
    assert (list(a), capped, missed, over) == ([3], False, False, False)
    assert list(bm.pick(r, one, 10_000, np.array([0]), 100.0, 16)[0]) == [0]             # candidate 0: no bits
    assert list(bm.pick(r, one, 10_000, np.array([0]), 5.0, 16)[0]) == [2]               # equality passes
    assert list(bm.pick(r, one, 10_000, np.array([0]), 0.45, 16)[0]) == [8]
    # n_cand = 4: the sizes are 0, 2, 3, 4 and entries beyond are not looked at
    a, capped, missed, over = bm.pick(r, one, 10_000, np.array([0]), 0.45, 4)
    assert (list(a), capped, missed, over) == ([4], True, True, False)


def test_the_three_kinds_of_capped_unit():
    lines = np.array([10, 20])
    rows = np.concatenate((row(9.0, 5.0, 1.0), row(9.0, 8.0, 7.0, 1.0)))
    # nothing capped: 3 x 10 + 4 x 20 = 110 bits
    a, capped, missed, over = bm.pick(rows, lines, 110, np.array([2, 2]), 2.0, 16)
    assert (list(a), capped, missed, over) == ([3, 4], False, False, False)
    # a band missed at every size (NaN at the only passing one): 16 bits for it, the sum still fits, a_b kept
    nan_rows = rows.copy()
    nan_rows[1, 3] = np.nan
    a, capped, missed, over = bm.pick(nan_rows, lines, 10_000, np.array([2, 2]), 2.0, 16)
    assert (list(a), capped, missed, over) == ([3, 16], True, True, False)
    # the sum exceeds the cap: coded with cap_alloc
    a, capped, missed, over = bm.pick(rows, lines, 109, np.array([2, 3]), 2.0, 16)
    assert (list(a), capped, missed, over) == ([2, 3], True, False, True)
    # ... and a cap_alloc of zeros is taken as it is
    a, capped, missed, over = bm.pick(rows, lines, 0, np.array([0, 0]), 2.0, 16)
    assert (list(a), capped, missed, over) == ([0, 0], True, False, True)
    # a miss whose 16 bits exceed the cap: cap_alloc as well
    a, capped, missed, over = bm.pick(nan_rows, lines, 200, np.array([2, 3]), 2.0, 16)
    assert (list(a), capped, missed, over) == ([2, 3], True, True, True)


def test_vectorised_total_is_the_unit_by_unit_one(K):
    kinds = np.zeros(3, int)
    for t in (-75 * 64, -30 * 64, -641, -1, 0, 7, 500, 30 * 64):
        tot, alloc, n_bytes, capped, missed, over = bm.evaluate(K, t, detail=True)
        assert tot == bm.total_slow(K, t)
        for cf in range(0, 120, 7):
            a, n, cap = bm.frame(K, cf, t / 64)
            assert np.array_equal(alloc[cf], a) and n_bytes[cf] == n and capped[cf] == cap
        kinds += [int((missed & ~over).any()), int((over & ~missed).any()), int((over & missed).any())]
    assert kinds.all()                                         # every kind of capped unit somewhere on the way
    dropped = (K["cap"] < 0).all(axis=1)
    assert dropped.any() and not bm.evaluate(K, 0)[2][dropped].any() and not bm.evaluate(K, 0)[1][dropped].any()
    assert (bm.evaluate(K, 0)[2][~dropped] > 0).all()
    unit, lines = bm.layout(K)
    assert not bm.evaluate(K, 0)[1][unit < 0].any()            # no unit, no bits


def test_rows_are_not_monotone(C):
    unit, _ = bm.layout(C)
    r = C["nmr"][unit >= 0]
    assert (np.diff(r, axis=1) > 0).any() and (np.diff(r, axis=1) < 0).any()


def test_allocation_and_total_fall_as_the_target_rises_when_nothing_is_capped(C):
    ts = list(range(-20 * 64, 31 * 64, 37))
    ev = [bm.evaluate(C, t) for t in ts]
    assert (~ev[0][3]).mean() > 0.5                             # most channel-frames uncapped from the start
    for (_, a0, n0, c0), (_, a1, n1, c1) in zip(ev, ev[1:]):
        both = ~c0 & ~c1
        assert (a1[both] <= a0[both]).all() and (n1[both] <= n0[both]).all()
    # from the first target at which nothing at all is capped, the total itself falls
    first = next(i for i, e in enumerate(ev) if not e[3].any())
    tot = [e[0] for e in ev[first:]]
    assert len(tot) > 10 and all(b <= a for a, b in zip(tot, tot[1:])) and tot[-1] < tot[0]


def test_the_solve_is_the_brute_force_minimum_when_nothing_is_capped(C):
    t_lo = next(t for t in range(-20 * 64, 30 * 64) if not bm.evaluate(C, t)[3].any())
    t_hi = 30 * 64
    totals = {t: bm.total(C, t) for t in range(t_lo, t_hi + 1, 1)}
    for share in (0.05, 0.3, 0.5, 0.8, 0.99):
        limit = int(totals[t_hi] + share * (totals[t_lo] - totals[t_hi]))
        s = bm.solve(C, limit, t_lo, t_hi)
        assert s["met"] == 1 and not s["capped"].any()
        assert s["t"] == min(t for t, tot in totals.items() if tot <= limit)
        assert s["total"] == totals[s["t"]] == int(np.sum(s["n_bytes"][s["n_bytes"] > 0] + 4))
        assert len(s["path"]) + 1 <= 2 + int(np.ceil(np.log2(t_hi - t_lo + 2)))


def test_edges(K):
    lo_t, hi_t = -20 * 64, 20 * 64
    small, big = bm.total(K, hi_t), bm.total(K, lo_t)
    # unreachable: not even the highest target fits
    s = bm.solve(K, small - 1, lo_t, hi_t)
    assert (s["met"], s["t"], s["total"]) == (0, hi_t, small) and len(s["path"]) == 1
    # the limit is exactly the smallest total
    s = bm.solve(K, small, lo_t, hi_t)
    assert s["met"] == 1 and s["total"] <= small
    # everything fits at the lowest target (capped units: take a limit above every total on the path)
    s = bm.solve(K, 10 * max(big, small), lo_t, hi_t)
    assert (s["met"], s["t"], s["total"]) == (1, lo_t, big)
    # limit == total(t) exactly, at a t the bisection reaches
    ref = bm.solve(K, (small + big) // 2, lo_t, hi_t)
    s = bm.solve(K, ref["total"], lo_t, hi_t)
    assert s["met"] == 1 and s["total"] <= ref["total"]
    if s["t"] == ref["t"]:
        assert s["total"] == ref["total"]
    # one point on the grid
    s = bm.solve(K, 10 * big, 5, 5)
    assert (s["met"], s["t"]) == (1, 5) and len(s["path"]) == 1
    # no channel-frames
    empty = bm.with_arrays(K, np.zeros((0, K["band_stride"], bm.CAND)), np.zeros((0, 8), np.int32),
                           np.zeros((0, K["band_stride"]), np.int32))
    s = bm.solve(empty, 0, lo_t, hi_t)
    assert (s["met"], s["t"], s["total"]) == (1, lo_t, 0)


def test_margins_and_sanitise(K):
    m = bm.margins(K, 0.0)
    assert np.array_equal(np.isinf(m), K["cap"] < 0)
    unit, _ = bm.layout(K)
    cf = int(np.argmax((K["cap"] >= 0).all(axis=1)))            # a short-coded frame
    d = np.abs(K["nmr"][cf][unit[cf] == 3])
    assert m[cf, 3] == np.nanmin(d)
    assert list(bm.sanitise(K, [-3, 0, 1, 2, 7, 16, 17, 99])) == [0, 0, 0, 2, 7, 16, 16, 16]
    assert [bm.bits_of(i) for i in range(4)] == [0, 2, 3, 4] and bm.bits_of(15) == 16


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
    assert re.search(r"#define\s+PACX_BAND_CAND\s+16\b", header) and a._lib.BAND_CAND == bm.CAND == 16
    assert lib.pacx_abi_version() == 7                 # additive: no caller breaks


def test_band_kernels_use_no_scratch():
    """the compiler's resource report of the new kernels: no scratch, no spilled registers"""
    import importlib
    res = importlib.import_module("audio_codec_amd.build").resources()
    mine = {k: v for k, v in res.items() if v["source"] == "k_band.hip"}
    assert {n for n in ("k_band_curve<1024>", "k_band_curve<128>", "k_band_pick", "k_band_sanitize")
            if any(n in k for k in mine)} == {"k_band_curve<1024>", "k_band_curve<128>", "k_band_pick", "k_band_sanitize"}
    for name, r in mine.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
