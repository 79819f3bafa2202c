"""Curves kept as thresholds on the GPU (pacx_band_thresholds / pacx_rate_thresholds and the four picks on them, the
Encoder methods of those names, streaming.HostStreamRateEncoder.keep_curves, pacfile.encode_stream_abr_kept /
iter_encode_abr_kept).

Everything here is integers and bytes: every check is for equality, there is no tolerance.
  Thresholds.  On planted curves (profile_model.planted, rate_profile_model.planted) the kept arrays are the model's
  (tests/kept_model.py) in EVERY entry, starting from outputs filled with 0xFF: 0 - 5 frames, the frames either side of
  the kernels' 256 threads (the band pick holds four frames per workgroup), grids of 1 to PACX_PROFILE_MAX targets, a
  handle with fewer than 16 sizes, rate rows at and above the layout's.
  Picks.  On those curves the picks from thresholds are the existing picks of the same handle, array for array, at every
  target of a narrow range (which holds every planted grid point and its neighbours), at the ends and drawn targets of
  a wide one, and per segment.  The same on the GPU's own curves of the widths tests' stream.
  Streams.  encode_stream_abr_kept gives encode_stream_abr_chunked's bytes and messages, and takes every chunk's curve
  once where that call takes it twice.  Nothing existing moves.
"""
import functools

import numpy as np
import pytest

import band_model as bm
import kept_model as km
import profile_model as pm
import rate_profile_model as rp
import vq_band_model as vm
import widths_cases as wc
from conftest import load_excerpt

pytestmark = pytest.mark.gpu

GRID = bm.GRID
NARROW, WIDE = (-2 * GRID, 2 * GRID), (-30 * GRID, 30 * GRID)
GRIDS = [(-3 * GRID, -3 * GRID), (17, 18), NARROW, WIDE, (-64 * GRID, 64 * GRID)]      # G = 1, 2, 257, 3841, 8193
THREADS = 256               # k_kept.hip: threads of every workgroup; k_rate_pick_kept holds a frame per thread
FRAMES = [0, 1, 2, 3, 4, 5, THREADS - 1, THREADS, THREADS + 1]
BAND_OUT, RATE_OUT = ("bit_alloc", "n_bytes", "capped"), ("budget", "n_bytes", "capped")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def solver(A, nm_bits=12):
    """a scalar encoder on the band tables of band_model.synthetic"""
    return A.context.encoder(44100, 128 / 44.1, 4, nm_bits)


def band_dev(enc, c):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(c[k]), device=enc.device) for k in ("nmr", "cap", "cap_alloc")}


def rate_dev(enc, c):
    import torch
    d = {k: torch.as_tensor(np.ascontiguousarray(c[k]), device=enc.device) for k in ("worst", "bits", "steps")}
    d["row"], d["sub_stride"] = c["row"], c["sub_stride"]
    return d


def poisoned(enc, shapes):
    """outputs filled with 0xFF bytes: an entry the kernel leaves out shows"""
    import torch
    return {k: torch.as_tensor(np.full(shape, -1, np.int64).astype(dtype), device=enc.device)
            for k, (shape, dtype) in shapes.items()}


@functools.lru_cache(maxsize=None)
def band_curve(n_cf, seed, t_lo, t_hi, cap_scale=0.6, n_cand=16):
    c = pm.planted(n_cf, seed, t_lo, t_hi, cap_scale=cap_scale)
    if n_cand != 16:                                        # a handle with fewer sizes: the entries beyond hold anything
        bits = {8: 3}[n_cand]
        rng = np.random.default_rng(seed)
        c["nmr"][:, :, n_cand:] = rng.uniform(-40, 40, c["nmr"][:, :, n_cand:].shape)
        c["n_cand"], c["n_mant_size_bits"] = n_cand, bits
        c["cap_alloc"] = np.minimum(c["cap_alloc"], n_cand)
    return c


@functools.lru_cache(maxsize=None)
def rate_curve(n_cf, seed, t_lo, t_hi, extra=0):
    c = rp.planted(n_cf, seed, t_lo, t_hi)
    if extra:                                               # a row above the layout's: the tail belongs to no unit
        rng = np.random.default_rng(seed)
        c["worst"] = np.concatenate((c["worst"], rng.uniform(-40, 40, (n_cf, extra))), axis=1)
        c["bits"] = np.concatenate((c["bits"], rng.integers(1, 999, (n_cf, extra)).astype(np.int32)), axis=1)
        c["row"] += extra
    return c


def same(got, want, keys, what=None):
    for k in keys:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = want[k].cpu().numpy() if hasattr(want[k], "cpu") else np.asarray(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), (k, what)


def check_band_thresholds(enc, c, t_lo, t_hi):
    n_cf, bs = len(c["cap"]), c["band_stride"]
    assert bs == enc.band_stride
    out = poisoned(enc, {"e": ((n_cf, bs, 16), np.uint16), "cap": ((n_cf, 8), np.int32), "cap_alloc": ((n_cf, bs), np.uint8)})
    kept = enc.band_thresholds(band_dev(enc, c), t_lo / GRID, t_hi / GRID, out=out)
    assert all(kept[k] is out[k] for k in out) and (kept["nmr_lo_db"], kept["nmr_hi_db"]) == (t_lo / GRID, t_hi / GRID)
    same(kept, km.band_thresholds(c, t_lo, t_hi), ("e", "cap", "cap_alloc"), (n_cf, t_lo, t_hi))
    return kept


def check_rate_thresholds(enc, c, t_lo, t_hi):
    n_cf, row = len(c["steps"]), c["row"]
    out = poisoned(enc, {"e": ((n_cf, row), np.uint16), "bits": ((n_cf, row), np.int32), "steps": ((n_cf, 8), np.int32)})
    kept = enc.rate_thresholds(rate_dev(enc, c), t_lo / GRID, t_hi / GRID, out=out)
    assert all(kept[k] is out[k] for k in out) and (kept["row"], kept["sub_stride"]) == (row, c["sub_stride"])
    same(kept, km.rate_thresholds(c, t_lo, t_hi), ("e", "bits", "steps"), (n_cf, t_lo, t_hi))
    return kept


# ------------------------------------------------------------------------------------------------ 1. thresholds
@pytest.mark.parametrize("n_cf", FRAMES)
def test_thresholds_frame_counts(A, n_cf):
    enc = solver(A)
    t_lo, t_hi = NARROW
    kept = check_band_thresholds(enc, band_curve(n_cf, 40 + n_cf, t_lo, t_hi), t_lo, t_hi)
    assert kept["e"].dtype.itemsize == 2 and kept["cap_alloc"].dtype.itemsize == 1
    assert sum(kept[k].numel() * kept[k].element_size() for k in ("e", "cap", "cap_alloc")) == \
        n_cf * km.band_bytes_per_cf(enc.band_stride) == n_cf * A.pacfile._BandPath(enc).kept_bytes_per_cf(0.0)
    kept = check_rate_thresholds(enc, rate_curve(n_cf, 60 + n_cf, t_lo, t_hi), t_lo, t_hi)
    assert sum(kept[k].numel() * kept[k].element_size() for k in ("e", "bits", "steps")) == \
        n_cf * km.rate_bytes_per_cf(kept["row"])
    # made by the call: the same arrays
    c = band_curve(n_cf, 40 + n_cf, t_lo, t_hi)
    same(enc.band_thresholds(band_dev(enc, c), t_lo / GRID, t_hi / GRID), km.band_thresholds(c, t_lo, t_hi),
         ("e", "cap", "cap_alloc"))


@pytest.mark.parametrize("t_lo,t_hi", GRIDS)
def test_thresholds_grids(A, t_lo, t_hi):
    enc = solver(A)
    assert t_hi - t_lo + 1 in (1, 2, 257, 3841, rp.PROFILE_MAX)
    check_band_thresholds(enc, band_curve(40, 7, t_lo, t_hi), t_lo, t_hi)
    check_rate_thresholds(enc, rate_curve(40, 8, t_lo, t_hi), t_lo, t_hi)
    check_rate_thresholds(enc, rate_curve(40, 8, t_lo, t_hi, extra=5), t_lo, t_hi)       # a row above the layout's, odd


def test_thresholds_with_fewer_sizes_and_cut_rows(A):
    """a handle of eight sizes: the entries beyond them hold G whatever the curve holds there, and the pick agrees; a
    rate row that cuts J; units of one and two entries"""
    enc = solver(A, nm_bits=3)
    t_lo, t_hi = NARROW
    c = band_curve(70, 5, t_lo, t_hi, n_cand=8)
    kept = check_band_thresholds(enc, c, t_lo, t_hi)
    assert bool((kept["e"][:, :, 8:] == t_hi - t_lo + 1).all())
    dev = band_dev(enc, c)
    for t in (t_lo, -31, 0, 17, t_hi):
        same(enc.band_pick_thresholds(kept, t / GRID), enc.band_pick(dev, t / GRID), BAND_OUT, t)
    enc = solver(A)
    full = rp.planted(80, 9, t_lo, t_hi, j_long=200, j_short=4)
    c = rp.narrowed(full, 7 * full["sub_stride"] + 1)
    assert (rp.cut(c)["steps"] < c["steps"]).any()
    kept = check_rate_thresholds(enc, c, t_lo, t_hi)
    dev = rate_dev(enc, c)
    for t in (t_lo, -31, 0, 17, t_hi):
        same(enc.rate_pick_thresholds(kept, t / GRID), enc.rate_pick(dev, t / GRID), RATE_OUT, t)
        same(enc.rate_pick_thresholds(kept, t / GRID), rp.pick(c, t), RATE_OUT, t)


# ------------------------------------------------------------------------------------------------ 2. picks
@pytest.mark.parametrize("n_cf", [5, THREADS + 1])
def test_picks_at_every_target_of_a_narrow_range(A, n_cf):
    """every planted grid point and its neighbours lie in the range or are cut to its ends: all 257 targets are tried"""
    enc = solver(A)
    t_lo, t_hi = NARROW
    cb, cr = band_curve(n_cf, 90, t_lo, t_hi), rate_curve(n_cf, 91, t_lo, t_hi)
    bdev, rdev = band_dev(enc, cb), rate_dev(enc, cr)
    bkept, rkept = check_band_thresholds(enc, cb, t_lo, t_hi), check_rate_thresholds(enc, cr, t_lo, t_hi)
    capped = 0
    for t in range(t_lo, t_hi + 1):
        want = enc.band_pick(bdev, t / GRID)
        same(enc.band_pick_thresholds(bkept, t / GRID), want, BAND_OUT, t)
        same(enc.rate_pick_thresholds(rkept, t / GRID), enc.rate_pick(rdev, t / GRID), RATE_OUT, t)
        capped += int(want["capped"].sum().item())
    assert capped                                           # the cap rule ran
    for t in (t_lo, 3, t_hi):                               # and the models', once
        same(enc.band_pick_thresholds(bkept, t / GRID), km.band_pick(km.band_thresholds(cb, t_lo, t_hi), t), BAND_OUT, t)


@pytest.mark.parametrize("n_cf", FRAMES)
def test_picks_frame_counts_and_drawn_targets_of_a_wide_range(A, n_cf):
    enc = solver(A)
    t_lo, t_hi = WIDE
    cb, cr = band_curve(n_cf, 70 + n_cf, t_lo, t_hi), rate_curve(n_cf, 80 + n_cf, t_lo, t_hi)
    bdev, rdev = band_dev(enc, cb), rate_dev(enc, cr)
    bkept = enc.band_thresholds(bdev, t_lo / GRID, t_hi / GRID)
    rkept = enc.rate_thresholds(rdev, t_lo / GRID, t_hi / GRID)
    rng = np.random.default_rng(n_cf)
    for t in [t_lo, t_hi] + [int(t) for t in rng.integers(t_lo, t_hi + 1, 16)]:
        same(enc.band_pick_thresholds(bkept, t / GRID), enc.band_pick(bdev, t / GRID), BAND_OUT, t)
        same(enc.rate_pick_thresholds(rkept, t / GRID), enc.rate_pick(rdev, t / GRID), RATE_OUT, t)


@pytest.mark.parametrize("n_cf", [5, 300])
def test_segment_picks(A, n_cf):
    enc = solver(A)
    t_lo, t_hi = NARROW
    cb, cr = band_curve(n_cf, 33, t_lo, t_hi), rate_curve(n_cf, 34, t_lo, t_hi)
    bdev, rdev = band_dev(enc, cb), rate_dev(enc, cr)
    bkept = enc.band_thresholds(bdev, t_lo / GRID, t_hi / GRID)
    rkept = enc.rate_thresholds(rdev, t_lo / GRID, t_hi / GRID)
    rng = np.random.default_rng(n_cf)
    for seg_cf in (1, 2, 3, 64, n_cf):
        for first_off in sorted({0, seg_cf - 1}):
            t = rng.integers(t_lo, t_hi + 1, -(-(first_off + n_cf) // seg_cf))
            what = (seg_cf, first_off)
            same(enc.band_pick_thresholds_segments(bkept, seg_cf, first_off, t),
                 enc.band_pick_segments(bdev, seg_cf, first_off, t), BAND_OUT, what)
            same(enc.rate_pick_thresholds_segments(rkept, seg_cf, first_off, t),
                 enc.rate_pick_segments(rdev, seg_cf, first_off, t), RATE_OUT, what)
    t = rng.integers(t_lo, t_hi + 1, -(-(2 + n_cf) // 3))
    same(enc.band_pick_thresholds_segments(bkept, 3, 2, t), km.band_pick_segments(km.band_thresholds(cb, t_lo, t_hi), 3, 2, t),
         BAND_OUT)
    same(enc.rate_pick_thresholds_segments(rkept, 3, 2, t), km.rate_pick_segments(km.rate_thresholds(cr, t_lo, t_hi), 3, 2, t),
         RATE_OUT)
    # all targets equal: the plain pick, bit for bit
    t = np.full(-(-n_cf // 64), 37)
    same(enc.band_pick_thresholds_segments(bkept, 64, 0, t), enc.band_pick_thresholds(bkept, 37 / GRID), BAND_OUT)
    same(enc.rate_pick_thresholds_segments(rkept, 64, 0, t), enc.rate_pick_thresholds(rkept, 37 / GRID), RATE_OUT)


def test_arguments_and_refusals(A):
    import torch
    enc = solver(A)
    t_lo, t_hi = NARROW
    cb, cr = band_curve(5, 33, t_lo, t_hi), rate_curve(5, 34, t_lo, t_hi)
    bkept = enc.band_thresholds(band_dev(enc, cb), -2, 2)
    rkept = enc.rate_thresholds(rate_dev(enc, cr), -2, 2)
    for call in (enc.band_pick_thresholds, enc.rate_pick_thresholds):
        kept = bkept if call == enc.band_pick_thresholds else rkept
        for bad in (0.01, 2 + 1 / 64, -2 - 1 / 64, float("nan"), float("inf")):       # off the grid, outside the range
            with pytest.raises(A._lib.PacxError):
                call(kept, bad)
    for bad in (dict(nmr_lo_db=3, nmr_hi_db=-3), dict(nmr_lo_db=-70, nmr_hi_db=70), dict(nmr_lo_db=0.01, nmr_hi_db=1)):
        with pytest.raises(ValueError):
            enc.band_thresholds(band_dev(enc, cb), **bad)
        with pytest.raises(ValueError):
            enc.rate_thresholds(rate_dev(enc, cr), **bad)
    with pytest.raises(ValueError):
        enc.band_thresholds(band_dev(enc, cb), -2, 2, out={**bkept, "e": bkept["e"].view(torch.int16)})
    with pytest.raises(ValueError):
        enc.band_pick_thresholds({**bkept, "cap_alloc": bkept["cap_alloc"].int()}, 0.0)
    with pytest.raises(ValueError):
        enc.rate_pick_thresholds_segments(rkept, 2, 0, [0, 0])          # three segments, two targets
    with pytest.raises(ValueError):
        enc.band_pick_thresholds_segments(bkept, 2, 2, [0, 0, 0])
    # a device target outside the range is clamped into it
    far = torch.as_tensor(np.array([10 ** 6, -10 ** 6, 0], np.int32), device=enc.device)
    ends = [t_hi, t_lo, 0]
    same(enc.band_pick_thresholds_segments(bkept, 2, 0, far), enc.band_pick_thresholds_segments(bkept, 2, 0, ends), BAND_OUT)
    same(enc.rate_pick_thresholds_segments(rkept, 2, 0, far), enc.rate_pick_thresholds_segments(rkept, 2, 0, ends), RATE_OUT)
    # n_cf = 0 is a valid call
    none = enc.band_thresholds(band_dev(enc, band_curve(0, 1, t_lo, t_hi)), -2, 2)
    assert enc.band_pick_thresholds(none, 0.0)["n_bytes"].numel() == 0
    # handles that are not scalar answer NotImplementedError
    for other in (A.context.encoder(44100, 96 / 44.1, use_vq=True), A.context.encoder(44100, 96 / 44.1, use_vq=True, use_sbr=True)):
        for call in (lambda: other.band_thresholds(band_dev(other, cb), -2, 2),
                     lambda: other.rate_thresholds(rate_dev(other, cr), -2, 2),
                     lambda: other.band_pick_thresholds({k: v.to(other.device) if hasattr(v, "to") else v
                                                         for k, v in bkept.items()}, 0.0),
                     lambda: other.rate_pick_thresholds_segments(rkept, 2, 0, [0, 0, 0])):
            with pytest.raises(NotImplementedError):
                call()


# ------------------------------------------------------------------------------------------------ 3. the GPU's own curves
def test_picks_on_the_gpus_own_curves(A):
    """the block-switched six-hop stereo castanet excerpt of the widths tests: band curve, rate curve at a 320 kb/s cap,
    gain-shape band curve; at the solved target and at both ends of the range"""
    pcm, sr = wc.stream()
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    bps = cp.targetBitsPerSample
    band, rate = enc.band_curve(view, flags, bps), enc.rate_curve(view, flags, bps)
    assert bool((band["cap"][:, 1] >= 0).any()) and bool((band["cap"][:, 1] < 0).any())        # short and long frames
    _, vq, vview, vflags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None, use_vq=True)
    sib = A.context.scalar_sibling(vq)
    gain = vq.vq_band_curve(vview, vflags, bps)
    for who, curve in ((enc, band), (sib, gain)):
        prof = who.band_profile(curve)
        limit = int((prof[0].item() + prof[-1].item()) // 2)
        sol = who.band_solve(curve, limit)
        assert sol["met"] and -30 < sol["target_nmr_db"] < 30
        kept = who.band_thresholds(curve)
        host = {k: curve[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")}
        same(kept, km.band_thresholds({**bm.tables(_params(cp)), **host}, *WIDE), ("e", "cap", "cap_alloc"))
        same(who.band_pick_thresholds(kept, sol["target_nmr_db"]), sol, BAND_OUT)
        for t in (-30.0, 30.0):
            same(who.band_pick_thresholds(kept, t), who.band_pick(curve, t), BAND_OUT, t)
    prof = enc.rate_profile(rate)
    sol = enc.rate_solve(rate, flags, int((prof[0].item() + prof[-1].item()) // 2))
    assert sol["met"]
    kept = enc.rate_thresholds(rate)
    same(enc.rate_pick_thresholds(kept, sol["target_nmr_db"]), sol, RATE_OUT)
    for t in (-30.0, 30.0):
        same(enc.rate_pick_thresholds(kept, t), enc.rate_pick(rate, t), RATE_OUT, t)


def _params(cp):
    from oracle import pac_oracle as po
    return po.make_params(cp.sampleRate, cp.nChannels, 320)


# ------------------------------------------------------------------------------------------------ 4. streams
@functools.lru_cache(maxsize=None)
def castanet():
    ex = load_excerpt("castanet")
    return np.ascontiguousarray(ex["pcm"][:len(ex["pcm"]) // 1024 * 1024]), int(ex["sr"])


def stream_of(name):
    return castanet() if name == "castanet" else vm.fixture_stream()


def frozen(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def chunked(name, kw):
    import audio_codec_amd as A
    pcm, sr = stream_of(name)
    return A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, **dict(kw))


SEGMENTS = [dict(), dict(segment_hops=3), dict(segment_hops=8), dict(segment_hops=8, peak_kbps_per_channel=128)]


@pytest.mark.parametrize("allocation", ["band", "budget"])
@pytest.mark.parametrize("chunk_hops", [1, 5, "all", 4096])
def test_kept_equals_chunked_on_castanet(A, chunk_hops, allocation):
    pcm, sr = castanet()
    hops = len(pcm) // 1024 if chunk_hops == "all" else chunk_hops
    for more in SEGMENTS:
        kw = dict(kbps_per_channel=96, allocation=allocation, **more)
        got = A.pacfile.encode_stream_abr_kept(pcm, sr, chunk_hops=hops, block_switching=True, **kw)
        assert got == chunked("castanet", frozen(kw)), more
    if chunk_hops == 5:
        plain, one = chunked("castanet", frozen(dict(kbps_per_channel=96, allocation=allocation))), None
        for more in SEGMENTS[1:]:
            assert chunked("castanet", frozen(dict(kbps_per_channel=96, allocation=allocation, **more))) != plain
        one = A.pacfile.encode_stream_abr(pcm, sr, 96, block_switching=True, allocation=allocation)
        assert plain == one                                 # and so the one-batch call


def test_a_peak_pins_some_of_castanets_segments(A):
    pcm, sr = castanet()
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    n_ch, blocks = cp.nChannels, view.n_frames
    first, count, peaks = A.pacfile.segment_limits(128, n_ch, sr, blocks, 8)
    limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    hr = A.streaming.HostStreamRateEncoder(enc, n_ch, 5, 320 / (sr / 1000), block_switching=True)
    assert hr.keep_curves() is hr
    hr.analyse(pcm, segment_hops=8, segment_limits=peaks, peak=True)
    sol = hr.solve_peak(limit)
    assert sol["pinned"].any() and not sol["pinned"].all()
    assert hr.kept is not None and len(hr.kept["store"]) == hr.kept_bytes(len(pcm) // 1024)
    kept = b"".join(bytes(b) for b in hr.encode(pcm, sol["target_nmr_db"], segment_hops=8, segment_limits=peaks))
    again = b"".join(bytes(b) for b in hr.encode(pcm, sol["target_nmr_db"], segment_hops=8, segment_limits=peaks,
                                                use_kept=False))
    want = chunked("castanet", frozen(dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=128)))
    assert kept == again and A.pacfile.header_bytes(cp) + kept == want
    # with a store, targets off the grid or outside the object's range are refused
    for bad in (0.01, 31.0, -30.5):
        with pytest.raises(ValueError, match="kept curves"):
            list(hr.encode(pcm, bad))
    assert b"".join(bytes(b) for b in hr.encode(pcm, 31.0, use_kept=False))           # today's route takes it
    # a stream of another length: the store is not used
    short = pcm[:7 * 1024]
    assert b"".join(bytes(b) for b in hr.encode(short, 0.0)) == b"".join(bytes(b) for b in hr.encode(short, 0.0, use_kept=False))


@pytest.mark.parametrize("chunk_hops", [1, 3, 4096])
def test_kept_equals_chunked_for_gain_shape(A, chunk_hops):
    pcm, sr = vm.fixture_stream()
    for more in (dict(), dict(segment_hops=3)):
        kw = dict(kbps_per_channel=96, max_kbps_per_channel=vm.CAP_KBPS, use_vq=True, **more)
        got = A.pacfile.encode_stream_abr_kept(pcm, sr, chunk_hops=chunk_hops, block_switching=True, **kw)
        assert got == chunked("fixture", frozen(kw)), more
    assert chunked("fixture", frozen(dict(kbps_per_channel=96, max_kbps_per_channel=vm.CAP_KBPS, use_vq=True))) == \
        A.pacfile.encode_stream_vq_abr(pcm, sr, 96, max_kbps_per_channel=vm.CAP_KBPS, block_switching=True)


@pytest.mark.parametrize("allocation", ["band", "budget"])
def test_a_memmap_store_and_the_iterators_pieces(A, tmp_path, allocation):
    pcm, sr = castanet()
    hops = len(pcm) // 1024
    cp, enc, _, _ = A.pacfile._rate_stream_setup(pcm[:1024], sr, 320, True, None)
    hr = A.streaming.HostStreamRateEncoder(enc, cp.nChannels, 12, cp.targetBitsPerSample, allocation=allocation)
    need = hr.kept_bytes(hops)
    cp2 = A.pacfile._rate_coding_params(pcm, sr, 320, None)
    A.pacfile.header_bytes(cp2)
    assert need == (hops + 2) * cp.nChannels * A.pacfile._kept_bytes_per_cf(cp2, allocation)
    store = np.memmap(tmp_path / "curves.u8", dtype=np.uint8, mode="w+", shape=(need + 3,))
    store[:] = 0xFF
    kw = dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=128, allocation=allocation)
    parts = list(A.pacfile.iter_encode_abr_kept(pcm, sr, chunk_hops=12, block_switching=True, curve_store=store, **kw))
    assert len(parts) == 1 + -(-hops // 12) + 1 and all(isinstance(p, bytes) for p in parts)
    assert parts[0] == A.pacfile.header_bytes(A.pacfile._rate_coding_params(pcm, sr, 320, None))
    assert b"".join(parts) == chunked("castanet", frozen(kw))
    assert (store[need:] == 0xFF).all() and not (store[:need] == 0xFF).all()          # written, and not past its size
    with pytest.raises(ValueError, match="curve_store"):
        A.pacfile.encode_stream_abr_kept(pcm, sr, chunk_hops=12, curve_store=store[:need - 1], **kw)


def test_error_messages_are_the_chunked_calls(A):
    pcm, sr = castanet()
    for kw, part in ((dict(kbps_per_channel=8, segment_hops=8), "cannot be reached: its limit is"),
                     (dict(kbps_per_channel=1), "cannot be reached: at the highest target"),
                     (dict(kbps_per_channel=1, segment_hops=8, peak_kbps_per_channel=128),
                      "cannot be reached: at the highest target")):
        for allocation in ("band", "budget"):
            with pytest.raises(ValueError) as want:
                A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, allocation=allocation, **kw)
            with pytest.raises(ValueError) as got:
                A.pacfile.encode_stream_abr_kept(pcm, sr, chunk_hops=5, block_switching=True, allocation=allocation, **kw)
            with pytest.raises(ValueError) as pieces:
                list(A.pacfile.iter_encode_abr_kept(pcm, sr, chunk_hops=5, block_switching=True, allocation=allocation, **kw))
            assert str(got.value) == str(want.value) == str(pieces.value) and part in str(want.value)
    with pytest.raises(NotImplementedError, match="^gain-shape streams: allocation 'band' only$"):
        A.pacfile.encode_stream_abr_kept(pcm, sr, 96, allocation="budget", use_vq=True)


@pytest.mark.parametrize("allocation,use_vq", [("band", False), ("budget", False), ("band", True)])
def test_every_curve_is_taken_once(A, monkeypatch, allocation, use_vq):
    """the point of the feature: a stream in k chunks and the tail takes k + 1 curves kept, 2 (k + 1) chunked"""
    pcm, sr = vm.fixture_stream() if use_vq else castanet()
    pcm = pcm[:12 * 1024]
    path = A.pacfile._BandPath if allocation == "band" else A.pacfile._BudgetPath
    real, calls = path.curve, []

    def counted(self, view, flags, max_bits_per_sample):
        calls.append(view.n_frames)
        return real(self, view, flags, max_bits_per_sample)
    monkeypatch.setattr(path, "curve", counted)
    hops = len(pcm) // 1024
    for chunk_hops in (1, 5):
        k = -(-hops // chunk_hops)
        kw = dict(kbps_per_channel=96, chunk_hops=chunk_hops, block_switching=True, allocation=allocation, use_vq=use_vq,
                  max_kbps_per_channel=vm.CAP_KBPS if use_vq else 320)
        del calls[:]
        kept = A.pacfile.encode_stream_abr_kept(pcm, sr, **kw)
        assert len(calls) == k + 1 and sum(calls) == hops + 2, (calls, k)
        del calls[:]
        assert A.pacfile.encode_stream_abr_chunked(pcm, sr, **kw) == kept
        assert len(calls) == 2 * (k + 1), (calls, k)


# ------------------------------------------------------------------------------------------------ 5. nothing existing moves
def test_without_keep_curves_nothing_is_kept_and_existing_calls_are_unchanged(A):
    pcm, sr = castanet()
    pcm = pcm[:12 * 1024]
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    curve = enc.band_curve(view, flags, cp.targetBitsPerSample)

    def snapshot():
        out = enc.encode_pack(view, flags)
        pick = enc.band_pick(curve, -1.5)
        hr = A.streaming.HostStreamRateEncoder(enc, cp.nChannels, 5, cp.targetBitsPerSample, block_switching=True)
        hr.analyse(pcm)
        sol = hr.solve(30000)
        body = b"".join(bytes(b) for b in hr.encode(pcm, sol["target_nmr_db"]))
        assert hr.keep is None and hr.kept is None and not hasattr(hr, "dev_kept") and not hasattr(hr, "host_kept")
        return ([out[k].cpu().numpy().copy() for k in ("n_bytes", "bit_alloc", "overall", "status")] +
                [out["payload"].cpu().numpy()[:, :64].copy()] + [pick[k].cpu().numpy().copy() for k in BAND_OUT] +
                [np.frombuffer(body, np.uint8), np.array([sol["target_nmr_db"], sol["met"], sol["total_bytes"]])] +
                [np.frombuffer(A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=5,
                                                                   block_switching=True), np.uint8)])
    before = snapshot()
    kept = enc.band_thresholds(curve)
    enc.band_pick_thresholds(kept, -1.5)
    enc.band_pick_thresholds_segments(kept, 4, 0, np.zeros(-(-view.n_cf // 4), np.int64))
    rate = enc.rate_curve(view, flags, cp.targetBitsPerSample)
    rkept = enc.rate_thresholds(rate)
    enc.rate_pick_thresholds(rkept, 2.0)
    enc.rate_pick_thresholds_segments(rkept, 4, 0, np.zeros(-(-view.n_cf // 4), np.int64))
    assert A.pacfile.encode_stream_abr_kept(pcm, sr, kbps_per_channel=96, chunk_hops=5, block_switching=True) == \
        bytes(before[-1])
    after = snapshot()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
