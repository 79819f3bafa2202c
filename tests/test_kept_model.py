"""CPU checks of the curves kept as thresholds (include/pacx.h, pacx_band_thresholds / pacx_rate_thresholds and the picks
on them): tests/kept_model.py's picks on the 16-bit form against the models on the curve itself -- band_model.evaluate,
rate_profile_model.pick -- at every grid target of a narrow range and at drawn targets of a wide one, on curves with
everything planted that the form can get wrong; the segment forms slice by slice; the layout rules of the kept arrays;
the exports; the store's arithmetic; what encode_stream_abr_kept and keep_curves refuse before an encoder exists; and
the three signatures that stay as they are."""
import inspect
import os
import re

import numpy as np
import pytest

import band_model as bm
import kept_model as km
import profile_model as pm
import rate_profile_model as rp

GRID = bm.GRID
NARROW, WIDE = (-2 * GRID, 2 * GRID), (-30 * GRID, 30 * GRID)
NAMES = ("pacx_band_thresholds", "pacx_band_pick_thresholds", "pacx_band_pick_thresholds_segments",
         "pacx_rate_thresholds", "pacx_rate_pick_thresholds", "pacx_rate_pick_thresholds_segments")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


def same(got, want, keys):
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def band_want(c, t):
    _, alloc, n_bytes, capped = bm.evaluate(c, t)
    return {"bit_alloc": alloc, "n_bytes": n_bytes, "capped": capped}


BAND_KEYS, RATE_KEYS = ("bit_alloc", "n_bytes", "capped"), ("budget", "n_bytes", "capped")


@pytest.mark.parametrize("n_cf,seed,cap_scale", [(40, 7, 1.0), (40, 9, 0.4), (300, 21, 0.6)])
def test_band_pick_on_thresholds_is_the_models_at_every_target_of_a_narrow_range(n_cf, seed, cap_scale):
    t_lo, t_hi = NARROW
    c = pm.planted(n_cf, seed, t_lo, t_hi, cap_scale=cap_scale)
    kept = km.band_thresholds(c, t_lo, t_hi)
    some_capped = False
    for t in range(t_lo, t_hi + 1):
        want = band_want(c, t)
        same(km.band_pick(kept, t), want, BAND_KEYS)
        some_capped |= bool(want["capped"].any())
    assert some_capped                                      # the cap rule was taken


@pytest.mark.parametrize("n_cf,seed,cap_scale", [(40, 7, 0.5), (300, 21, 1.0)])
def test_band_pick_on_thresholds_is_the_models_at_drawn_targets_of_a_wide_range(n_cf, seed, cap_scale):
    t_lo, t_hi = WIDE
    c = pm.planted(n_cf, seed, t_lo, t_hi, cap_scale=cap_scale)
    kept = km.band_thresholds(c, t_lo, t_hi)
    rng = np.random.default_rng(seed)
    for t in [t_lo, t_hi] + [int(t) for t in rng.integers(t_lo, t_hi + 1, 200)]:
        same(km.band_pick(kept, t), band_want(c, t), BAND_KEYS)


def test_band_thresholds_write_every_entry_and_depend_on_defined_entries_only():
    t_lo, t_hi = NARROW
    G = t_hi - t_lo + 1
    c = pm.planted(60, 3, t_lo, t_hi)
    kept = km.band_thresholds(c, t_lo, t_hi)
    unit, _ = bm.layout(c)
    assert kept["e"].dtype == np.uint16 and kept["cap_alloc"].dtype == np.uint8 and kept["cap"].dtype == np.int32
    assert (kept["e"][unit < 0] == G).all() and (kept["e"][:, :, c["n_cand"]:] == G).all()
    assert (kept["cap_alloc"][unit < 0] == 0).all() and np.array_equal(kept["cap"], c["cap"])
    assert (kept["e"] <= G).all() and (kept["e"][unit >= 0][:, :c["n_cand"]] < G).any()
    junk = bm.with_arrays(c, c["nmr"].copy(), c["cap"], c["cap_alloc"].copy())     # what no band uses, overwritten
    junk["nmr"][unit < 0] = -123.0
    junk["nmr"][:, :, c["n_cand"]:] = -5.0
    junk["cap_alloc"][unit < 0] = 9
    again = km.band_thresholds(junk, t_lo, t_hi)
    same(again, kept, ("e", "cap", "cap_alloc"))
    wide = bm.with_arrays(c, c["nmr"], c["cap"], np.where(unit >= 0, c["cap_alloc"] + 300, c["cap_alloc"]))
    assert (km.band_thresholds(wide, t_lo, t_hi)["cap_alloc"][unit >= 0] == 255).all()      # saturates
    assert kept["e"].nbytes + kept["cap"].nbytes + kept["cap_alloc"].nbytes == 60 * km.band_bytes_per_cf(c["band_stride"])


@pytest.mark.parametrize("t_lo,t_hi", [NARROW, (0, 0), (-7, -6), (5 * GRID, 9 * GRID)])
def test_rate_pick_on_thresholds_is_the_models_at_every_target(t_lo, t_hi):
    c = rp.planted(120, 5, t_lo, t_hi)
    kept = km.rate_thresholds(c, t_lo, t_hi)
    for t in range(t_lo, t_hi + 1):
        same(km.rate_pick(kept, t), rp.pick(c, t), RATE_KEYS)


def test_rate_pick_on_thresholds_at_drawn_targets_with_a_row_that_cuts_J():
    t_lo, t_hi = WIDE
    full = rp.planted(90, 17, t_lo, t_hi, j_long=200, j_short=12)
    c = rp.narrowed(full, 7 * full["sub_stride"] + 1)       # long blocks' J leave the row: cut by the rule
    assert (c["steps"][:, 0] > c["row"] - 1).any()
    kept = km.rate_thresholds(c, t_lo, t_hi)
    assert (kept["steps"][:, 0] <= c["row"] - 1).all()
    lengths = c["steps"][c["steps"] >= 0]
    assert (lengths == 0).any() and (lengths == 1).any()    # units of one and of two entries
    assert (c["steps"] < 0).all(axis=1).any()               # dropped hops
    rng = np.random.default_rng(4)
    for t in [t_lo, t_hi] + [int(t) for t in rng.integers(t_lo, t_hi + 1, 200)]:
        same(km.rate_pick(kept, t), rp.pick(c, t), RATE_KEYS)


def test_rate_thresholds_write_every_entry():
    t_lo, t_hi = NARROW
    G = t_hi - t_lo + 1
    c = rp.planted(80, 2, t_lo, t_hi)
    kept = km.rate_thresholds(c, t_lo, t_hi)
    used = np.zeros(c["worst"].shape, bool)
    for cf, sb in zip(*np.nonzero(c["steps"] >= 0)):
        at = sb * c["sub_stride"]
        used[cf, at:at + int(c["steps"][cf, sb]) + 1] = True
    assert (kept["e"][~used] == G).all() and (kept["bits"][~used] == 0).all()
    assert np.array_equal(kept["bits"][used], c["bits"][used])
    assert np.array_equal(kept["e"][used], rp.thresholds(c["worst"], t_lo, t_hi)[used])
    assert kept["e"].nbytes + kept["bits"].nbytes + kept["steps"].nbytes == 80 * km.rate_bytes_per_cf(c["row"])


@pytest.mark.parametrize("seg_cf,first_off", [(1, 0), (2, 1), (3, 0), (3, 2), (64, 0), (64, 63), (10 ** 6, 0)])
def test_segment_forms_are_the_plain_models_slice_by_slice(seg_cf, first_off):
    t_lo, t_hi = NARROW
    n_cf = 150
    rng = np.random.default_rng(seg_cf + first_off)
    n_seg = -(-(first_off + n_cf) // seg_cf)
    targets = rng.integers(t_lo, t_hi + 1, n_seg)
    edges = np.clip(np.arange(n_seg + 1) * seg_cf - first_off, 0, n_cf)
    cb = pm.planted(n_cf, 31, t_lo, t_hi, cap_scale=0.6)
    got = km.band_pick_segments(km.band_thresholds(cb, t_lo, t_hi), seg_cf, first_off, targets)
    for a, b, t in zip(edges, edges[1:], targets):
        want = band_want(bm.with_arrays(cb, cb["nmr"][a:b], cb["cap"][a:b], cb["cap_alloc"][a:b]), int(t))
        same({k: got[k][a:b] for k in BAND_KEYS}, want, BAND_KEYS)
    cr = rp.planted(n_cf, 32, t_lo, t_hi)
    got = km.rate_pick_segments(km.rate_thresholds(cr, t_lo, t_hi), seg_cf, first_off, targets)
    same(got, rp.pick_segments(cr, edges, targets), RATE_KEYS)


def test_library_exports_the_kept_calls(A):
    lib = A.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pacx.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in A._lib.SIGNATURES, name
        args = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(A._lib.SIGNATURES[name][1]) == len(args.split(",")), name
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7
    for name in NAMES:
        assert callable(getattr(A.engine.Encoder, name[len("pacx_"):]))
    from audio_codec_amd import pacfile
    for path in (pacfile._BandPath, pacfile._BudgetPath):
        for name in ("thresholds", "pick_kept", "pick_kept_segments", "kept_bytes_per_cf"):
            assert callable(getattr(path, name))


def test_kept_bytes_arithmetic(A):
    """the store's size: (n_hops + 2) nCh kept_bytes_per_cf, per_cf = 33 band_stride + 32 or 6 row + 32; the host-only
    mirror the kept call refuses a short store with agrees with the models' tables"""
    from audio_codec_amd import pacfile, streaming

    class Path:
        def kept_bytes_per_cf(self, max_bits_per_sample):
            return 33 * 200 + 32

    hr = streaming.HostStreamRateEncoder.__new__(streaming.HostStreamRateEncoder)
    hr.n_ch, hr.path, hr.max_bps = 2, Path(), 7.0
    assert hr.kept_bytes(10) == 12 * 2 * (33 * 200 + 32)
    import abr_model as am
    import rate_model as rm
    from oracle import pac_oracle as po
    for sample_rate, kbps in ((44100, 320), (44100, 128), (48000, 96)):
        pcm = np.zeros((2048, 2), np.int16)
        cp = pacfile._rate_coding_params(pcm, sample_rate, kbps, None)
        pacfile.header_bytes(cp)
        c = bm.tables(po.make_params(sample_rate, 2, kbps))
        assert pacfile._kept_bytes_per_cf(cp, "band") == km.band_bytes_per_cf(c["band_stride"])
        a = {"sample_rate": sample_rate, "n_ch": 2, "p": po.make_params(sample_rate, 2, kbps, rm.HOP)}
        row, _ = am.layout(a, kbps)
        assert pacfile._kept_bytes_per_cf(cp, "budget") == km.rate_bytes_per_cf(row)


def test_kept_abr_refuses_before_an_encoder_is_asked_for(A, monkeypatch):
    """a store one byte short, read-only or not uint8, and every refusal of the chunked call, are raised before an
    encoder is asked for; valid calls get as far as the encoder"""
    from audio_codec_amd import context, pacfile, streaming

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    cp = pacfile._rate_coding_params(pcm, 44100, 320, None)
    pacfile.header_bytes(cp)
    for call in (pacfile.encode_stream_abr_kept, pacfile.iter_encode_abr_kept):
        for allocation in ("band", "budget"):
            need = 6 * 2 * pacfile._kept_bytes_per_cf(cp, allocation)
            kw = dict(kbps_per_channel=96, chunk_hops=2, allocation=allocation)
            with pytest.raises(ValueError, match="curve_store.*it holds %d" % (need - 1)):
                call(pcm, 44100, curve_store=np.zeros(need - 1, np.uint8), **kw)
            frozen = np.zeros(need, np.uint8)
            frozen.setflags(write=False)
            with pytest.raises(ValueError, match="curve_store.*read-only"):
                call(pcm, 44100, curve_store=frozen, **kw)
            with pytest.raises(ValueError, match="curve_store.*not uint8"):
                call(pcm, 44100, curve_store=np.zeros(need, np.int8), **kw)
            with pytest.raises(ValueError, match="curve_store.*not C-contiguous"):
                call(pcm, 44100, curve_store=np.zeros(2 * need, np.uint8)[::2], **kw)
            with pytest.raises(ValueError, match="curve_store"):
                call(pcm, 44100, curve_store=7, **kw)
            for store in (None, np.zeros(need, np.uint8), bytearray(need)):
                for more in (dict(), dict(segment_hops=3), dict(segment_hops=3, peak_kbps_per_channel=128)):
                    with pytest.raises(AssertionError, match="an encoder was asked for"):
                        call(pcm, 44100, curve_store=store, **kw, **more)
        # the chunked call's own refusals, with its messages
        for bad in ("bands", "", None, 1):
            with pytest.raises(ValueError, match="allocation"):
                call(pcm, 44100, kbps_per_channel=96, chunk_hops=2, allocation=bad)
        with pytest.raises(NotImplementedError, match="^gain-shape streams: allocation 'band' only$"):
            call(pcm, 44100, kbps_per_channel=96, chunk_hops=2, allocation="budget", use_vq=True)
        for kw in (dict(chunk_hops=0), dict(chunk_hops=2.5), dict(nmr_range_db=(-100, 100)), dict(segment_hops=0),
                   dict(peak_kbps_per_channel=128), dict(max_bytes=10 ** 6)):
            kw = {"kbps_per_channel": 96, "chunk_hops": 2, **kw}
            with pytest.raises(ValueError) as kept:
                call(pcm, 44100, **kw)
            with pytest.raises(ValueError) as chunked:
                pacfile.encode_stream_abr_chunked(pcm, 44100, **kw)
            assert str(kept.value) == str(chunked.value)
        with pytest.raises(ValueError, match="at least one block"):
            call(np.zeros((0, 2), np.int16), 44100, kbps_per_channel=96)
        names = list(inspect.signature(call).parameters)
        assert names[:-1] == list(inspect.signature(pacfile.encode_stream_abr_chunked).parameters)
        assert names[-1] == "curve_store" and inspect.signature(call).parameters["curve_store"].default is None
    # keep_curves on the object: the same three refusals from analyse(), before it queues anything
    hr = streaming.HostStreamRateEncoder.__new__(streaming.HostStreamRateEncoder)

    class Path:
        solver = None

        def kept_bytes_per_cf(self, max_bits_per_sample):
            return 100
    hr.n_ch, hr.path, hr.max_bps, hr.keep, hr.kept = 2, Path(), 7.0, None, None
    need = hr.kept_bytes(4)
    frozen = np.zeros(need, np.uint8)
    frozen.setflags(write=False)
    for store, why in ((np.zeros(need - 1, np.uint8), "it holds"), (frozen, "read-only"),
                       (np.zeros(need, np.uint16), "not uint8")):
        assert hr.keep_curves(store) is hr
        with pytest.raises(ValueError, match="store.*" + why):
            hr.analyse(pcm)


def test_the_three_pinned_signatures_are_unchanged(A):
    from audio_codec_amd import pacfile, streaming
    want = ["pcm", "sample_rate", "kbps_per_channel", "max_bytes", "chunk_hops", "max_kbps_per_channel",
            "block_switching", "header_samples", "nmr_range_db", "use_vq", "segment_hops", "peak_kbps_per_channel",
            "allocation"]
    for call in (pacfile.encode_stream_abr_chunked, pacfile.iter_encode_abr_chunked):
        assert list(inspect.signature(call).parameters) == want
        assert inspect.signature(call).parameters["allocation"].default == "band"
    assert list(inspect.signature(streaming.HostStreamRateEncoder.__init__).parameters) == \
        ["self", "enc", "n_channels", "hops_per_chunk", "max_bits_per_sample", "block_switching", "nmr_lo_db",
         "nmr_hi_db", "depth", "allocation"]
    assert "use_kept" in inspect.signature(streaming.HostStreamRateEncoder.encode).parameters
    assert callable(streaming.HostStreamRateEncoder.keep_curves) and callable(streaming.HostStreamRateEncoder.kept_bytes)
