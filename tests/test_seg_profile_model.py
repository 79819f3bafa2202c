"""CPU checks of the per-segment rate profile (include/pacx.h, pacx_band_profile_segments / pacx_profile_solve_segments /
pacx_profile_clamp_add / pacx_band_pick_segments): tests/seg_profile_model.py -- rows, a solve per row, the clamped sum
-- gives what segment_model.solve_segments and peak_model.solve_peak give on the whole curve; rows are additive over
any cut of the frames; the exports; and what the chunked encode refuses of the new keywords before it touches a GPU."""
import functools
import os
import re

import numpy as np
import pytest

import band_model as bm
import peak_model as pk
import seg_profile_model as sp
import segment_model as sm

GRID = bm.GRID
T_LO, T_HI = -2 * GRID, 2 * GRID
MATERIAL = [(300, 7, 1.0), (300, 9, 0.2), (41, 3, 0.2)]
NAMES = ("pacx_band_profile_segments", "pacx_profile_solve_segments", "pacx_profile_clamp_add",
         "pacx_band_pick_segments")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


@functools.lru_cache(maxsize=None)
def material(n_cf, seed, cap_scale):
    """(curve, boundaries, peaks, rows, floors of the reference), taken once and left unchanged"""
    c = bm.synthetic(n_cf, seed, cap_scale=cap_scale)
    first = sm.boundaries(n_cf)
    peaks = sm.limits_for("band", c, first, T_LO, T_HI)
    rows = sp.rows(c, first, T_LO, T_HI)
    rows.setflags(write=False)
    return c, first, peaks, rows, pk.floors("band", c, first, peaks, T_LO, T_HI)


@pytest.mark.parametrize("n_cf,seed,cap_scale", MATERIAL)
def test_solve_per_row_is_the_segmented_solve(n_cf, seed, cap_scale):
    c, first, limits, rows, _ = material(n_cf, seed, cap_scale)
    want = sm.solve_segments("band", c, first, limits, T_LO, T_HI)
    got = sp.solve_rows(rows, limits, T_LO, T_HI)
    for k in ("t", "met", "total"):
        assert np.array_equal(got[k], want[k]), k
    assert 0 < got["met"].sum() < len(limits)               # both decisions are taken
    for s, row in enumerate(rows):                          # worst_above against its definition, target by target
        a, b = int(first[s]), int(first[s + 1])
        part = sp.piece(c, a, b)
        assert got["worst_above"][s] == max(bm.total(part, t) for t in range(int(got["t"][s]), T_HI + 1))
    empty = np.flatnonzero(np.diff(first) == 0)
    assert len(empty) and (got["t"][empty] == T_LO).all() and (got["met"][empty] == 1).all() and \
        (got["total"][empty] == 0).all()


@pytest.mark.parametrize("n_cf,seed,cap_scale", MATERIAL)
def test_peak_solve_on_rows_is_the_peak_solve(n_cf, seed, cap_scale):
    c, first, peaks, rows, u = material(n_cf, seed, cap_scale)
    limits = pk.stream_limits("band", c, first, peaks, T_LO, T_HI, u=u)
    met = []
    for limit in limits:
        want = pk.solve_peak("band", c, first, peaks, limit, T_LO, T_HI, u=u)
        got = sp.solve_peak(rows, peaks, limit, T_LO, T_HI)
        assert np.array_equal(got["floor"], want["floor"])
        assert (got["t_stream"], got["met_stream"], got["total_stream"]) == \
            (want["t_stream"], want["met_stream"], want["total_stream"]), limit
        for k in ("t", "met", "total"):
            assert np.array_equal(got[k], want[k]), (k, limit)
        met.append(got["met_stream"])
    assert met == [1, 0, 1, 1]


def test_material_holds_a_doubtful_and_an_unreachable_segment():
    """(300, 7): a segment the peaks can reach whose size above its floor exceeds its peak somewhere -- the case the
    chunked encode can only decide in its second pass -- and one that cannot be reached"""
    _, _, peaks, rows, _ = material(300, 7, 1.0)
    a = sp.solve_rows(rows, peaks, T_LO, T_HI)
    assert ((a["met"] == 1) & (a["worst_above"] > peaks)).any()
    assert (a["met"] == 0).any()
    assert (a["worst_above"] >= a["total"]).all()


def test_negative_limit_is_never_met():
    _, _, peaks, rows, _ = material(41, 3, 0.2)
    got = sp.solve_rows(rows, np.full(len(rows), -1), T_LO, T_HI)
    assert (got["met"] == 0).all() and (got["t"] == T_HI).all() and np.array_equal(got["total"], rows[:, -1])


def test_clamp_add_adds():
    _, _, peaks, rows, u = material(41, 3, 0.2)
    out = np.full(rows.shape[1], 5, np.int64)
    sp.clamp_add(rows, u, T_LO, out=out)
    assert np.array_equal(out, sp.clamp_add(rows, u, T_LO) + 5)
    # floors at t_lo: nothing is clamped, the sum is the stream's profile
    assert np.array_equal(sp.clamp_add(rows, np.full(len(rows), T_LO), T_LO), rows.sum(axis=0))


@pytest.mark.parametrize("seg_cf,first_off", [(1, 0), (7, 0), (7, 6), (64, 63), (1000, 999), (1000, 0)])
def test_rows_are_additive_over_cuts(seg_cf, first_off):
    """uniform segments as the C API takes them; the frames cut at arbitrary places, inside segments too: every piece
    adds its share to the rows of the segments it touches"""
    c = material(300, 7, 1.0)[0]
    n_cf = 300
    whole = sp.rows(c, sp.uniform_first(n_cf, seg_cf, first_off), T_LO, T_HI)
    assert np.array_equal(whole.sum(axis=0), sp.pm.profile(c, T_LO, T_HI))
    got = np.zeros((len(whole) + 2, whole.shape[1]), np.int64)
    for a, b in ((0, 1), (1, 1), (1, 10), (10, 77), (77, 78), (78, 299), (299, 300)):
        off = (first_off + a) % seg_cf
        s0 = (first_off + a) // seg_cf
        local = sp.uniform_first(b - a, seg_cf, off)
        sp.rows(sp.piece(c, a, b), local, T_LO, T_HI, out=got[s0:])
    assert np.array_equal(got[:len(whole)], whole) and not got[len(whole):].any()


def test_library_exports_the_segment_profile_calls(A):
    lib = A.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pacx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert hasattr(lib, name) and name in A._lib.SIGNATURES and name in declared, name
    assert set(A._lib.SIGNATURES) == declared
    # argument counts of the four against the header's declarations
    for name in NAMES:
        args = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(A._lib.SIGNATURES[name][1]) == len(args.split(",")), name
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7


def test_chunked_abr_refuses_the_new_keywords_before_gpu_work(A, monkeypatch):
    """every refusal is a ValueError raised before an encoder is asked for"""
    from audio_codec_amd import context, pacfile

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    bad = [
        dict(peak_kbps_per_channel=128),                                    # a peak without segments
        dict(segment_hops=8, peak_kbps_per_channel=0), dict(segment_hops=8, peak_kbps_per_channel=-5),
        dict(segment_hops=8, kbps_per_channel=None, max_bytes=100000),      # a file size without a peak
        dict(segment_hops=8, kbps_per_channel=None),
        dict(segment_hops=0), dict(segment_hops=-2), dict(segment_hops=2.5),
        dict(segment_hops=0, peak_kbps_per_channel=128), dict(segment_hops=1.5, peak_kbps_per_channel=128),
        dict(segment_hops=8, kbps_per_channel=0), dict(segment_hops=8, kbps_per_channel=-1),
        dict(segment_hops=8, peak_kbps_per_channel=128, kbps_per_channel=None),
        dict(segment_hops=8, peak_kbps_per_channel=128, max_bytes=100000),  # two sizes
        dict(segment_hops=8, peak_kbps_per_channel=128, kbps_per_channel=None, max_bytes=3),
        dict(segment_hops=8, chunk_hops=0), dict(segment_hops=8, nmr_range_db=(-70, 70)),
    ]
    for kw in bad:
        args = dict(kbps_per_channel=96, chunk_hops=2)
        args.update(kw)
        with pytest.raises(ValueError):
            pacfile.encode_stream_abr_chunked(pcm, 44100, **args)
        with pytest.raises(ValueError):
            pacfile.iter_encode_abr_chunked(pcm, 44100, **args)
    # valid calls get as far as the encoder
    for kw in (dict(segment_hops=8), dict(segment_hops=3, peak_kbps_per_channel=128),
               dict(segment_hops=np.int64(3), peak_kbps_per_channel=128, kbps_per_channel=None, max_bytes=100000)):
        args = dict(kbps_per_channel=96, chunk_hops=2)
        args.update(kw)
        with pytest.raises(AssertionError, match="an encoder was asked for"):
            pacfile.encode_stream_abr_chunked(pcm, 44100, **args)
