"""CPU checks of the whole-grid profile of a rate curve (include/pacx.h, pacx_rate_profile / pacx_rate_profile_segments /
pacx_rate_pick / pacx_rate_pick_segments): tests/rate_profile_model.py's threshold route -- the way the kernel goes --
against the definition, abr_model.total target by target, on synthetic curves with everything planted that the route
can get wrong; rows per segment solved by seg_profile_model against segment_model and peak_model on the whole curve;
rows additive over cuts; the pick against abr_model.evaluate; the exports; and what the chunked encode refuses of the
new keyword before it touches a GPU."""
import functools
import os
import re

import numpy as np
import pytest

import abr_model as am
import peak_model as pk
import rate_profile_model as rp
import seg_profile_model as sp
import segment_model as sm

GRID = am.GRID
NARROW, WIDE = (-2 * GRID, 2 * GRID), (-30 * GRID, 30 * GRID)
NAMES = ("pacx_rate_profile", "pacx_rate_profile_segments", "pacx_rate_pick", "pacx_rate_pick_segments")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


@pytest.mark.parametrize("t_lo,t_hi", [NARROW, WIDE])
@pytest.mark.parametrize("n_cf,seed", [(60, 3), (41, 11)])
def test_threshold_route_is_the_definition_on_synthetic_curves(n_cf, seed, t_lo, t_hi):
    c = am.synthetic(n_cf, 40, 12, seed)
    want = rp.profile(c, t_lo, t_hi)
    assert np.array_equal(rp.profile_steps(c, t_lo, t_hi), want)
    assert want[0] > want[-1] > 0                           # the range is not a trivial one


@pytest.mark.parametrize("t_lo,t_hi", [NARROW, WIDE, (0, 0), (-7, -6), (5 * GRID, 9 * GRID)])
def test_threshold_route_is_the_definition_on_planted_entries(t_lo, t_hi):
    c = rp.planted(120, 5, t_lo, t_hi)
    assert np.array_equal(rp.profile_steps(c, t_lo, t_hi), rp.profile(c, t_lo, t_hi))


def test_planted_entries_are_what_they_claim():
    """the grid points, their neighbours, the infinities, NaN at J and inside, 1e300 and denormals are all among the
    entries the units read"""
    t_lo, t_hi = NARROW
    c = rp.planted(120, 5, t_lo, t_hi)
    used, at_J = [], []
    for cf, sb in zip(*np.nonzero(c["steps"] >= 0)):
        J, at = int(c["steps"][cf, sb]), sb * c["sub_stride"]
        used.append(c["worst"][cf, at:at + J + 1])
        at_J.append(c["worst"][cf, at + J])
    used, at_J = np.concatenate(used), np.array(at_J)
    x = used * GRID
    with np.errstate(invalid="ignore", over="ignore"):
        on_grid = np.isfinite(x) & (x == np.round(x)) & (x >= t_lo) & (x <= t_hi)
        ulp = np.isfinite(x) & (x != np.round(x)) & (np.abs(x - np.round(x)) < 1e-9) & (np.abs(used) > 1e-3)
    assert on_grid.sum() > 10 and ulp.sum() > 20
    assert np.isposinf(used).any() and np.isneginf(used).any() and np.isnan(used).any() and np.isnan(at_J).any()
    assert (used == 1e300).any() and (np.abs(used) == 5e-324).any()
    e = rp.thresholds(used, t_lo, t_hi)
    G = t_hi - t_lo + 1
    assert (e[np.isnan(used) | np.isposinf(used) | (used == 1e300)] == G).all() and (e[np.isneginf(used)] == 0).all()
    assert (e[used == 5e-324] == 1 - t_lo).all() and (e[used == -5e-324] == 0 - t_lo).all()


@pytest.mark.parametrize("J", [0, 1])
def test_units_of_one_and_two_entries(J):
    """J = 0: the cap test is the whole pick; J = 1: one halving"""
    t_lo, t_hi = NARROW
    rng = np.random.default_rng(J)
    n_cf, sub = 24, 2
    c = {"worst": rng.uniform(-3, 3, (n_cf, 8 * sub)), "bits": rng.integers(50, 900, (n_cf, 8 * sub)).astype(np.int32),
         "steps": np.full((n_cf, am.SUB), -1, np.int32), "row": 8 * sub, "sub_stride": sub}
    c["steps"][: n_cf // 2, 0] = J                          # long frames
    c["steps"][n_cf // 2:, :] = J                           # short-coded frames
    c["steps"][-1, :] = -1                                  # and a dropped hop
    c["worst"][3, :] = np.nan
    want = rp.profile(c, t_lo, t_hi)
    assert np.array_equal(rp.profile_steps(c, t_lo, t_hi), want)
    # one entry: whatever the target, the unit takes it (capped or not); two: the sizes move with the target
    assert len(set(want.tolist())) == 1 if J == 0 else len(set(want.tolist())) > 5


def test_a_row_that_cuts_a_units_J():
    t_lo, t_hi = NARROW
    full = am.synthetic(80, 40, 4, 9, p_short=0.5)          # row 41, sub_stride 5
    c = rp.narrowed(full, 7 * full["sub_stride"] + 1)       # row 36: long units above 35 and the last sub-block are cut
    steps, cutted = np.asarray(c["steps"]), rp.cut(c)["steps"]
    assert (cutted[:, 0] < steps[:, 0]).any() and (cutted[:, 7] < steps[:, 7]).any() and (cutted[:, 7][steps[:, 7] >= 0] == 0).all()
    want = rp.profile(c, t_lo, t_hi)
    assert np.array_equal(rp.profile_steps(c, t_lo, t_hi), want)
    assert not np.array_equal(want, rp.profile(full, t_lo, t_hi))      # the cut changes the sizes
    got = rp.pick(c, 0)
    assert (got["budget"] <= am.STEP * (c["row"] - 1)).all()


def test_dropped_hops_add_nothing():
    t_lo, t_hi = NARROW
    c = am.synthetic(50, 40, 12, 21, p_drop=0.5)
    dropped = (c["steps"] < 0).all(axis=1)
    assert 10 < dropped.sum() < 40
    want = rp.profile(c, t_lo, t_hi)
    assert np.array_equal(rp.profile_steps(c, t_lo, t_hi), want)
    kept = np.flatnonzero(~dropped)
    only = {"worst": c["worst"][kept], "bits": c["bits"][kept], "steps": c["steps"][kept], "row": c["row"],
            "sub_stride": c["sub_stride"]}
    assert np.array_equal(rp.profile_steps(only, t_lo, t_hi), want)
    assert not rp.profile_steps(rp.piece(c, 0, 0), t_lo, t_hi).any()


@functools.lru_cache(maxsize=None)
def material(n_cf, seed):
    """(curve, boundaries, peaks, rows, floors of the reference), taken once and left unchanged"""
    t_lo, t_hi = NARROW
    c = am.synthetic(n_cf, 40, 12, seed)
    first = sm.boundaries(n_cf)
    peaks = sm.limits_for("rate", c, first, t_lo, t_hi)
    rows = rp.rows(c, first, t_lo, t_hi)
    rows.setflags(write=False)
    return c, first, peaks, rows, pk.floors("rate", c, first, peaks, t_lo, t_hi)


@pytest.mark.parametrize("n_cf,seed", [(300, 7), (41, 3)])
def test_solve_per_row_is_the_segmented_solve(n_cf, seed):
    t_lo, t_hi = NARROW
    c, first, limits, rows, _ = material(n_cf, seed)
    want = sm.solve_segments("rate", c, first, limits, t_lo, t_hi)
    got = sp.solve_rows(rows, limits, t_lo, t_hi)
    for k in ("t", "met", "total"):
        assert np.array_equal(got[k], want[k]), k
    assert 0 < got["met"].sum() < len(limits)               # both decisions are taken
    picked = rp.pick_segments(c, first, got["t"])
    for k in sm.PER_CF["rate"]:
        assert np.array_equal(picked[k], want[k]), k
    whole = sp.pm.solve(rows.sum(axis=0), int(limits.sum() // 2), t_lo, t_hi)      # one segment: the plain solve
    plain = am.solve(c, int(limits.sum() // 2), t_lo, t_hi)
    assert (whole["t"], whole["met"], whole["total"]) == (plain["t"], plain["met"], plain["total"])


@pytest.mark.parametrize("n_cf,seed", [(300, 7), (41, 3)])
def test_peak_solve_on_rows_is_the_peak_solve(n_cf, seed):
    t_lo, t_hi = NARROW
    c, first, peaks, rows, u = material(n_cf, seed)
    met = []
    for limit in pk.stream_limits("rate", c, first, peaks, t_lo, t_hi, u=u):
        want = pk.solve_peak("rate", c, first, peaks, limit, t_lo, t_hi, u=u)
        got = sp.solve_peak(rows, peaks, limit, t_lo, t_hi)
        assert np.array_equal(got["floor"], want["floor"])
        assert (got["t_stream"], got["met_stream"], got["total_stream"]) == \
            (want["t_stream"], want["met_stream"], want["total_stream"]), limit
        for k in ("t", "met", "total"):
            assert np.array_equal(got[k], want[k]), (k, limit)
        met.append(got["met_stream"])
    assert met == [1, 0, 1, 1]


@pytest.mark.parametrize("seg_cf,first_off", [(1, 0), (7, 0), (7, 6), (64, 63), (1000, 999), (1000, 0)])
def test_rows_are_additive_over_cuts(seg_cf, first_off):
    """uniform segments as the C API takes them; the frames cut at arbitrary places, inside segments too"""
    t_lo, t_hi = NARROW
    c, n_cf = material(300, 7)[0], 300
    whole = rp.rows(c, sp.uniform_first(n_cf, seg_cf, first_off), t_lo, t_hi)
    assert np.array_equal(whole.sum(axis=0), rp.profile_steps(c, t_lo, t_hi))
    got = np.zeros((len(whole) + 2, whole.shape[1]), np.int64)
    for a, b in ((0, 1), (1, 1), (1, 10), (10, 77), (77, 78), (78, 299), (299, 300)):
        off, s0 = (first_off + a) % seg_cf, (first_off + a) // seg_cf
        rp.rows(rp.piece(c, a, b), sp.uniform_first(b - a, seg_cf, off), t_lo, t_hi, out=got[s0:])
    assert np.array_equal(got[:len(whole)], whole) and not got[len(whole):].any()


def test_rows_by_the_definition_are_the_threshold_routes():
    t_lo, t_hi = NARROW
    c = rp.planted(64, 13, t_lo, t_hi)
    first = sp.uniform_first(64, 9, 4)
    assert np.array_equal(rp.rows(c, first, t_lo, t_hi), rp.rows(c, first, t_lo, t_hi, route=rp.profile))


@pytest.mark.parametrize("t", [-2 * GRID, -17, 0, 1, 2 * GRID])
def test_pick_is_the_models_evaluation(t):
    c = rp.planted(90, 17, *NARROW)
    total, budget, n_bytes, capped = am.evaluate(c, t)
    got = rp.pick(c, t)
    assert np.array_equal(got["budget"], budget) and np.array_equal(got["n_bytes"], n_bytes) and \
        np.array_equal(got["capped"], capped)
    assert int(np.sum(n_bytes[n_bytes > 0] + 4)) == total == rp.profile_steps(c, t, t)[0]
    for cf in (0, 17, 89):                                  # and unit by unit
        b, n, cap = am.frame(c, cf, t / GRID)
        assert np.array_equal(b, budget[cf]) and n == n_bytes[cf] and cap == capped[cf]


def test_library_exports_the_rate_profile_calls(A):
    lib = A.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pacx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert hasattr(lib, name) and name in A._lib.SIGNATURES and name in declared, name
    assert set(A._lib.SIGNATURES) == declared
    for name in NAMES:                                      # argument counts against the header's declarations
        args = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(A._lib.SIGNATURES[name][1]) == len(args.split(",")), name
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7
    for name in ("rate_profile", "rate_profile_segments", "rate_pick", "rate_pick_segments"):
        assert callable(getattr(A.engine.Encoder, name))


def test_chunked_abr_refuses_before_gpu_work(A, monkeypatch):
    """a bad allocation is a ValueError and gain-shape with "budget" the one-batch call's NotImplementedError, both
    raised before an encoder is asked for; valid calls with the keyword get as far as the encoder"""
    import inspect
    from audio_codec_amd import context, pacfile, quality, streaming

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    for call in (pacfile.encode_stream_abr_chunked, pacfile.iter_encode_abr_chunked):
        for bad in ("bands", "", None, 1):
            with pytest.raises(ValueError, match="allocation"):
                call(pcm, 44100, kbps_per_channel=96, chunk_hops=2, allocation=bad)
        with pytest.raises(NotImplementedError, match="^gain-shape streams: allocation 'band' only$"):
            call(pcm, 44100, kbps_per_channel=96, chunk_hops=2, allocation="budget", use_vq=True)
        with pytest.raises(ValueError):                     # the other refusals come first with the keyword too
            call(pcm, 44100, kbps_per_channel=96, chunk_hops=0, allocation="budget")
        for kw in (dict(), dict(segment_hops=3), dict(segment_hops=3, peak_kbps_per_channel=128)):
            for allocation in ("budget", "band"):
                with pytest.raises(AssertionError, match="an encoder was asked for"):
                    call(pcm, 44100, kbps_per_channel=96, chunk_hops=2, allocation=allocation, **kw)
        assert list(inspect.signature(call).parameters)[-1] == "allocation"        # the LAST keyword; default: today's
        assert inspect.signature(call).parameters["allocation"].default == "band"
    with pytest.raises(ValueError, match="allocation"):
        quality.stream_rate_profile(pcm, 44100, chunk_hops=2, allocation="both")
    with pytest.raises(NotImplementedError):
        quality.stream_rate_profile(pcm, 44100, chunk_hops=2, allocation="budget", use_vq=True)
    assert inspect.signature(quality.stream_rate_profile).parameters["allocation"].default == "band"
    ctor = inspect.signature(streaming.HostStreamRateEncoder.__init__).parameters
    assert list(ctor)[-1] == "allocation" and ctor["allocation"].default == "band"
