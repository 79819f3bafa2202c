"""CPU checks of the whole-grid rate profile (include/pacx.h, pacx_band_profile / pacx_profile_solve): the step-function
route of tests/profile_model.py -- the kernel's route -- against band_model.total at every target of the range, the
solve on a profile against band_model.solve, the exports, and what encode_stream_abr_chunked refuses before it touches
a GPU."""
import os

import numpy as np
import pytest

import band_model as bm
import profile_model as pm

GRID = bm.GRID
NARROW, WIDE = (-2 * GRID, 2 * GRID), (-30 * GRID, 30 * GRID)


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


def totals(c, t_lo, t_hi):
    return np.array([bm.total(c, t) for t in range(t_lo, t_hi + 1)], np.int64)


@pytest.fixture(scope="module")
def wide():
    """one synthetic curve of a few hundred frames with its totals over +-30 dB, taken once"""
    c = bm.synthetic(200, 11)
    return c, totals(c, *WIDE)


def test_profile_equals_total_at_every_target_wide(wide):
    c, want = wide
    assert np.array_equal(pm.profile(c, *WIDE), want)
    assert len(set(want.tolist())) > 1000                   # the curve moves over the range: the steps are exercised


@pytest.mark.parametrize("n_cf,seed,cap_scale", [(300, 3, 1.0), (240, 4, 0.25), (1, 5, 1.0), (0, 6, 1.0)])
def test_profile_equals_total_at_every_target_narrow(n_cf, seed, cap_scale):
    c = bm.synthetic(n_cf, seed, cap_scale=cap_scale)
    assert np.array_equal(pm.profile(c, *NARROW), totals(c, *NARROW))


@pytest.mark.parametrize("cap_scale", [1.0, 0.2])
def test_planted_entries(cap_scale):
    """grid points and their neighbours one ulp away, +-inf, NaN, rows outside the range, huge and denormal values"""
    c = pm.planted(160, 21, *NARROW, cap_scale=cap_scale)
    want = totals(c, *NARROW)
    assert np.array_equal(pm.profile(c, *NARROW), want)
    if cap_scale < 1.0:                                     # many units take cap_alloc somewhere on the range
        over = bm.evaluate(c, NARROW[0], detail=True)[5]
        assert over.sum() > 50


def test_planted_entries_one_target():
    """G = 1 and G = 2: everything is a clamp"""
    c = pm.planted(40, 22, 0, 1)
    assert np.array_equal(pm.profile(c, 0, 0), totals(c, 0, 0))
    assert np.array_equal(pm.profile(c, 0, 1), totals(c, 0, 1))


def test_profile_is_additive(wide):
    c, want = wide
    out = np.full(len(want), 7, np.int64)
    for a, b in ((0, 77), (77, 200)):
        pm.profile(bm.with_arrays(c, c["nmr"][a:b], c["cap"][a:b], c["cap_alloc"][a:b]), *WIDE, out=out)
    assert np.array_equal(out, want + 7)


def test_solve_on_profile_equals_band_solve(wide):
    c, prof = wide
    t_lo, t_hi = WIDE
    top = int(prof[-1])
    ref = bm.solve(c, int(prof[len(prof) // 2]), t_lo, t_hi)
    on_path = [tot for _, tot in ref["path"]]
    limits = [0, top - 1, top // 2, top, top + 1, int(prof[0]), int(prof[0]) + 5, int(prof.max()) + 1] + \
        on_path + [v - 1 for v in on_path] + [v + 1 for v in on_path]
    for limit in limits:
        want, got = bm.solve(c, limit, t_lo, t_hi), pm.solve(prof, limit, t_lo, t_hi)
        assert (got["t"], got["met"], got["total"]) == (want["t"], want["met"], want["total"]), limit
    assert pm.solve(prof, top - 1, t_lo, t_hi)["met"] == 0 and pm.solve(prof, 0, t_lo, t_hi)["met"] == 0


def test_solve_on_profile_narrow_and_single():
    c = bm.synthetic(50, 8)
    for t_lo, t_hi in (NARROW, (5, 5), (5, 6)):
        prof = pm.profile(c, t_lo, t_hi)
        for limit in (0, int(prof.min()) - 1, int(prof.min()), int(prof[-1]), int(prof[0]), int(prof.max()) + 1):
            want, got = bm.solve(c, limit, t_lo, t_hi), pm.solve(prof, limit, t_lo, t_hi)
            assert (got["t"], got["met"], got["total"]) == (want["t"], want["met"], want["total"]), (t_lo, t_hi, limit)


def test_library_exports_the_profile_calls(A):
    lib = A.load()
    for name in ("pacx_band_profile", "pacx_profile_solve"):
        assert hasattr(lib, name) and name in A._lib.SIGNATURES
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7
    assert A._lib.PROFILE_MAX == pm.PROFILE_MAX
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pacx.h")).read()
    assert f"#define PACX_PROFILE_MAX {pm.PROFILE_MAX}" in header


def test_chunked_abr_refuses_before_gpu_work(A, monkeypatch):
    """every refusal is a ValueError raised before an encoder is asked for"""
    from audio_codec_amd import context, pacfile

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    bad = [
        dict(chunk_hops=0), dict(chunk_hops=-3), dict(chunk_hops=2.5), dict(chunk_hops="many"), dict(chunk_hops=None),
        dict(chunk_hops=True),
        dict(kbps_per_channel=None), dict(max_bytes=100000), dict(kbps_per_channel=0), dict(kbps_per_channel=-1),
        dict(kbps_per_channel=None, max_bytes=3),
        dict(max_kbps_per_channel=0), dict(max_kbps_per_channel=1000),
        dict(nmr_range_db=(3, -3)), dict(nmr_range_db=(0.01, 3)), dict(nmr_range_db=(-70, 70)), dict(nmr_range_db=5),
        dict(nmr_range_db=(float("nan"), 3)),
    ]
    for kw in bad:
        args = dict(kbps_per_channel=96, chunk_hops=2)
        args.update(kw)
        with pytest.raises(ValueError):
            pacfile.encode_stream_abr_chunked(pcm, 44100, **args)
        with pytest.raises(ValueError):
            pacfile.iter_encode_abr_chunked(pcm, 44100, **args)
    for wrong in (pcm[:1000], pcm.astype(np.int32), pcm[:, 0], pcm[:0]):
        with pytest.raises(ValueError):
            pacfile.encode_stream_abr_chunked(wrong, 44100, kbps_per_channel=96, chunk_hops=2)
    # a valid call gets as far as the encoder
    with pytest.raises(AssertionError, match="an encoder was asked for"):
        pacfile.encode_stream_abr_chunked(pcm, 44100, kbps_per_channel=96, chunk_hops=2)
    with pytest.raises(AssertionError, match="an encoder was asked for"):
        pacfile.encode_stream_abr_chunked(pcm, 44100, kbps_per_channel=96, chunk_hops=np.int64(7), use_vq=True)
