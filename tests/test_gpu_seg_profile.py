"""The per-segment rate profile and the chunked average-bit-rate encode with segments and peaks on the GPU
(pacx_band_profile_segments / pacx_profile_solve_segments / pacx_profile_clamp_add / pacx_band_pick_segments, the
Encoder methods of those names, streaming.HostStreamRateEncoder with segments, the segment_hops= and
peak_kbps_per_channel= keywords of pacfile.encode_stream_abr_chunked / iter_encode_abr_chunked).

Everything here is integers, comparisons and bytes: every check is for equality, there is no tolerance.
  Rows.  On synthetic curves (band_model.synthetic, profile_model.planted) the GPU's rows are the model's
  (tests/seg_profile_model.py: profile_model.profile per slice) for 0 - 5 and 511 - 513 frames, segments of 1, 2, 3, 64
  and all frames starting at a segment's first and last frame, grids of 1 to PACX_PROFILE_MAX targets; they add up.
  Solve and clamped sum equal the model's, which tests/test_seg_profile_model.py holds to segment_model and peak_model.
  The pick per segment is band_pick per slice.  End to end the chunked calls give the one-batch calls' bytes and
  messages.  Nothing existing moves.
"""
import ctypes
import functools

import numpy as np
import pytest

import band_model as bm
import peak_model as pk
import profile_model as pm
import seg_profile_model as sp
import segment_model as sm
import vq_band_model as vm
from conftest import load_excerpt

pytestmark = pytest.mark.gpu

GRID = bm.GRID
NARROW = (-2 * GRID, 2 * GRID)


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def solver(A):
    """a scalar encoder on the band tables of band_model.synthetic (the handle of tests/test_gpu_profile.py)"""
    return A.context.encoder(44100, 128 / 44.1)


def on_device(enc, c, a=0, b=None):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(c[k][a:b]), device=enc.device) for k in ("nmr", "cap", "cap_alloc")}


@functools.lru_cache(maxsize=None)
def synthetic(n_cf, seed, cap_scale=1.0):
    return bm.synthetic(n_cf, seed, cap_scale=cap_scale)


@functools.lru_cache(maxsize=None)
def frame_rows(n_cf, seed, t_lo, t_hi):
    """the model's profile of every single frame, [n_cf, G]: the rows of any segmentation are sums of these"""
    c = synthetic(n_cf, seed)
    out = sp.rows(c, np.arange(n_cf + 1), t_lo, t_hi)
    out.setflags(write=False)
    return out


def rows_from_frames(per_frame, seg_cf, first_off):
    n_cf = len(per_frame)
    n_seg = -(-(first_off + n_cf) // seg_cf)
    out = np.zeros((n_seg, per_frame.shape[1]), np.int64)
    np.add.at(out, (first_off + np.arange(n_cf)) // seg_cf, per_frame)
    return out


# ------------------------------------------------------------------------------------------------ 1. the rows
@pytest.mark.parametrize("n_cf,seed", [(0, 40), (1, 40), (3, 41), (5, 40), (511, 50), (512, 51), (513, 52)])
def test_rows_frame_counts_and_segment_lengths(A, n_cf, seed):
    import torch
    enc = solver(A)
    t_lo, t_hi = NARROW
    G = t_hi - t_lo + 1
    dev = on_device(enc, synthetic(n_cf, seed))
    per_frame = frame_rows(n_cf, seed, t_lo, t_hi)
    whole = enc.band_profile(dev, t_lo / GRID, t_hi / GRID).cpu().numpy()
    for seg_cf in (1, 2, 3, 64, n_cf + 3):
        for first_off in sorted({0, seg_cf - 1}):
            want = rows_from_frames(per_frame, seg_cf, first_off)
            got = enc.band_profile_segments(dev, seg_cf, first_off, t_lo / GRID, t_hi / GRID)
            assert got.dtype == torch.int64 and tuple(got.shape) == want.shape == (-(-(first_off + n_cf) // seg_cf), G)
            assert np.array_equal(got.cpu().numpy(), want), (seg_cf, first_off)
            assert np.array_equal(want.sum(axis=0), whole)              # the rows add up to band_profile of the curve
            # a larger buffer: a second call adds to the rows, the rows beyond n_seg are left alone
            buf = torch.full((len(want) + 2, G), 7, dtype=torch.int64, device=enc.device)
            buf[:len(want)] = got
            back = enc.band_profile_segments(dev, seg_cf, first_off, t_lo / GRID, t_hi / GRID, out=buf)
            assert back is buf
            assert np.array_equal(buf[:len(want)].cpu().numpy(), 2 * want) and bool((buf[len(want):] == 7).all())
    if n_cf:                                                            # one segment is band_profile
        one = enc.band_profile_segments(dev, n_cf, 0, t_lo / GRID, t_hi / GRID).cpu().numpy()
        assert one.shape == (1, G) and np.array_equal(one[0], whole)


@pytest.mark.parametrize("t_lo,t_hi", [(-3 * GRID, -3 * GRID), (17, 18), NARROW, (-30 * GRID, 30 * GRID),
                                       (-64 * GRID, 64 * GRID)])
def test_rows_grids(A, t_lo, t_hi):
    """G = 1, 2, 257, 3841 and PACX_PROFILE_MAX on 300 frames, a segment boundary inside most workgroups' runs"""
    enc = solver(A)
    assert t_hi - t_lo + 1 in (1, 2, 257, 3841, pm.PROFILE_MAX)
    c = synthetic(300, 7)
    seg_cf, first_off = 64, 5
    want = sp.rows(c, sp.uniform_first(300, seg_cf, first_off), t_lo, t_hi)
    got = enc.band_profile_segments(on_device(enc, c), seg_cf, first_off, t_lo / GRID, t_hi / GRID).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("cap_scale", [1.0, 0.2])
def test_rows_planted_entries(A, cap_scale):
    """grid points and their neighbours one ulp away, +-inf, NaN, rows outside the range, huge and denormal values;
    cap_scale 0.2: many units take cap_alloc"""
    enc = solver(A)
    for t_lo, t_hi in (NARROW, (0, 1), (5, 5)):
        c = pm.planted(160, 21, t_lo, t_hi, cap_scale=cap_scale)
        for seg_cf, first_off in ((7, 3), (1, 0), (200, 199)):
            want = sp.rows(c, sp.uniform_first(160, seg_cf, first_off), t_lo, t_hi)
            got = enc.band_profile_segments(on_device(enc, c), seg_cf, first_off, t_lo / GRID, t_hi / GRID)
            assert np.array_equal(got.cpu().numpy(), want), (t_lo, t_hi, seg_cf)


def test_rows_are_additive_over_pieces(A):
    """a stream cut inside segments: every piece adds its share, through `out`, at the rows of the segments it touches"""
    import torch
    enc = solver(A)
    c = synthetic(300, 7)
    t_lo, t_hi = NARROW
    seg_cf = 7
    want = rows_from_frames(frame_rows(300, 7, t_lo, t_hi), seg_cf, 0)
    buf = torch.zeros(want.shape, dtype=torch.int64, device=enc.device)
    for a, b in ((0, 1), (1, 10), (10, 150), (150, 150), (150, 299), (299, 300)):
        s0, off = a // seg_cf, a % seg_cf
        enc.band_profile_segments(on_device(enc, c, a, b), seg_cf, off, t_lo / GRID, t_hi / GRID, out=buf[s0:])
    assert np.array_equal(buf.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 2. solve and clamped sum
@functools.lru_cache(maxsize=None)
def solve_material(n_cf, seed, cap_scale):
    c = synthetic(n_cf, seed, cap_scale)
    first = sm.boundaries(n_cf)
    peaks = sm.limits_for("band", c, first, *NARROW)
    rows = sp.rows(c, first, *NARROW)
    return c, first, peaks, rows


@pytest.mark.parametrize("n_cf,seed,cap_scale", [(300, 7, 1.0), (300, 9, 0.2), (41, 3, 0.2)])
def test_solve_segments_and_clamp_add(A, n_cf, seed, cap_scale):
    import torch
    enc = solver(A)
    t_lo, t_hi = NARROW
    lo, hi = t_lo / GRID, t_hi / GRID
    c, first, peaks, rows = solve_material(n_cf, seed, cap_scale)
    rows_dev = torch.as_tensor(rows, device=enc.device)
    assert (rows.sum(axis=1) == 0).any()                                # empty segments: rows of zeros
    top = rows[:, -1]
    for limits in (peaks, np.zeros(len(rows), np.int64), np.maximum(top - 1, 0), top):
        want = sp.solve_rows(rows, limits, t_lo, t_hi)
        got = enc.profile_solve_segments(rows_dev, limits, lo, hi)
        assert np.array_equal(got["target_nmr_db"] * GRID, want["t"]) and np.array_equal(got["met"], want["met"] != 0)
        assert np.array_equal(got["total_bytes"], want["total"])
        assert np.array_equal(got["worst_above"], want["worst_above"])
        empty = rows.sum(axis=1) == 0
        assert (want["t"][empty] == t_lo).all() and (want["met"][empty] == 1).all() and (want["total"][empty] == 0).all()
        prof = torch.full((rows.shape[1],), 3, dtype=torch.int64, device=enc.device)
        assert enc.profile_clamp_add(rows_dev, got["result"], lo, hi, out=prof) is prof
        assert np.array_equal(prof.cpu().numpy(), sp.clamp_add(rows, want["t"], t_lo) + 3)
    # the peak solve on rows alone against the model on the whole curve
    u = pk.floors("band", c, first, peaks, t_lo, t_hi)
    floors = enc.profile_solve_segments(rows_dev, peaks, lo, hi)
    star = enc.profile_clamp_add(rows_dev, floors["result"], lo, hi)
    for limit in pk.stream_limits("band", c, first, peaks, t_lo, t_hi, u=u):
        want = pk.solve_peak("band", c, first, peaks, limit, t_lo, t_hi, u=u)
        got = enc.profile_solve(star, limit, lo, hi)
        assert (got["target_nmr_db"] * GRID, got["met"], got["total_bytes"]) == \
            (want["t_stream"], bool(want["met_stream"]), want["total_stream"]), limit
        assert np.array_equal(np.maximum(floors["target_nmr_db"] * GRID, want["t_stream"]), want["t"])
    # a negative limit, which only the C call takes (a device array): never met
    neg = torch.full((len(rows),), -1, dtype=torch.int64, device=enc.device)
    got = enc.profile_solve_segments(rows_dev, neg, lo, hi)
    assert not got["met"].any() and (got["target_nmr_db"] == hi).all() and np.array_equal(got["total_bytes"], top)
    with pytest.raises(ValueError):
        enc.profile_solve_segments(rows_dev, np.where(np.arange(len(rows)) == 2, -1, peaks), lo, hi)


def test_clamp_add_many_rows(A):
    """more rows than one trip of the clamp kernel's workgroups takes (4096 x 32): G = 2, every row its own words"""
    import torch
    enc = solver(A)
    n = 2 * 4096 * 32 + 5
    rng = np.random.default_rng(9)
    rows = rng.integers(0, 1000, (n, 2))
    t = rng.integers(17, 19, n)                                         # the range is [17, 18] in grid units
    res = np.zeros((n, 4), np.int32)
    res[:, 0] = t
    got = enc.profile_clamp_add(torch.as_tensor(rows, device=enc.device), torch.as_tensor(res, device=enc.device),
                                17 / GRID, 18 / GRID).cpu().numpy()
    assert got.tolist() == [int(np.where(t == 17, rows[:, 0], rows[:, 1]).sum()), int(rows[:, 1].sum())]


# ------------------------------------------------------------------------------------------------ 3. the pick per segment
@pytest.mark.parametrize("n_cf,seg_cf,first_off", [(300, 7, 3), (5, 1, 0), (513, 64, 63), (41, 100, 99)])
def test_pick_segments_is_band_pick_per_slice(A, n_cf, seg_cf, first_off):
    enc = solver(A)
    c = synthetic(n_cf, 7, 0.2)
    dev = on_device(enc, c)
    first = sp.uniform_first(n_cf, seg_cf, first_off)
    rng = np.random.default_rng(5)
    t = rng.integers(-2 * GRID, 2 * GRID + 1, len(first) - 1)
    got = enc.band_pick_segments(dev, seg_cf, first_off, t)
    for s, (a, b) in enumerate(zip(first, first[1:])):
        if b > a:
            want = enc.band_pick(on_device(enc, c, int(a), int(b)), t[s] / GRID)
            for k in ("bit_alloc", "n_bytes", "capped"):
                assert np.array_equal(got[k][a:b].cpu().numpy(), want[k].cpu().numpy()), (s, k)
    same = enc.band_pick_segments(dev, seg_cf, first_off, np.full(len(t), 37))
    plain = enc.band_pick(dev, 37 / GRID)
    for k in ("bit_alloc", "n_bytes", "capped"):
        assert np.array_equal(same[k].cpu().numpy(), plain[k].cpu().numpy()), k
    if n_cf == 300:
        assert got["capped"].any() and not got["capped"].all()


def test_arguments(A):
    import torch
    enc = solver(A)
    dev = on_device(enc, synthetic(5, 40))
    ptr = A.engine._ptr
    G = 257
    rows = torch.zeros((8, G), dtype=torch.int64, device=enc.device)
    res = torch.zeros((8, 4), dtype=torch.int32, device=enc.device)
    lim = torch.zeros(8, dtype=torch.int64, device=enc.device)
    t = torch.zeros(8, dtype=torch.int32, device=enc.device)
    alloc = torch.zeros((5, enc.band_stride), dtype=torch.int32, device=enc.device)
    nby, cpd = torch.zeros(5, dtype=torch.int32, device=enc.device), torch.zeros(5, dtype=torch.uint8, device=enc.device)
    i64, f64 = ctypes.c_int64, ctypes.c_double
    curve = [ptr(dev[k]) for k in ("nmr", "cap", "cap_alloc")]

    def profile(n_cf=5, seg_cf=2, off=0, lo=-2.0, hi=2.0, out=rows, arrays=curve):
        return enc.lib.pacx_band_profile_segments(enc.h, i64(n_cf), *arrays, i64(seg_cf), i64(off), f64(lo), f64(hi),
                                                  ptr(out) if out is not None else None, None)

    def pick(n_cf=5, seg_cf=2, off=0, targets=t, arrays=curve):
        return enc.lib.pacx_band_pick_segments(enc.h, i64(n_cf), *arrays, i64(seg_cf), i64(off),
                                               ptr(targets) if targets is not None else None, ptr(alloc), ptr(nby),
                                               ptr(cpd), None)

    def solve(n_seg=8, lo=-2.0, hi=2.0, rows=rows, limits=lim, result=res):
        return enc.lib.pacx_profile_solve_segments(enc.h, i64(n_seg), *(ptr(x) if x is not None else None
                                                                       for x in (rows, limits)), f64(lo), f64(hi),
                                                   ptr(result) if result is not None else None, None, None)

    prof = torch.zeros(G, dtype=torch.int64, device=enc.device)

    def clamp(n_seg=8, lo=-2.0, hi=2.0, rows=rows, result=res, out=prof):
        return enc.lib.pacx_profile_clamp_add(enc.h, i64(n_seg), *(ptr(x) if x is not None else None
                                                                  for x in (rows, result)), f64(lo), f64(hi),
                                              ptr(out) if out is not None else None, None)
    E_ARG = A._lib.E_ARG
    assert profile() == 0 and pick() == 0 and solve() == 0 and clamp() == 0          # worst_above may be null
    rows.zero_()
    no_curve = [None, curve[1], curve[2]]
    for rc in (profile(seg_cf=0), profile(seg_cf=-1), profile(off=2), profile(off=-1), profile(n_cf=-1), profile(out=None),
               profile(arrays=no_curve), profile(lo=3, hi=-3), profile(lo=0.01), profile(lo=-64, hi=64 + 1 / 64),
               profile(lo=float("nan")), profile(seg_cf=2 ** 40 + 1), profile(seg_cf=2 ** 62, off=2 ** 62 - 1),
               pick(seg_cf=2 ** 40 + 1), pick(seg_cf=2 ** 63 - 1, off=2 ** 63 - 2), pick(seg_cf=0), pick(off=2), pick(off=-1), pick(n_cf=-1), pick(targets=None),
               pick(arrays=no_curve), solve(n_seg=0), solve(n_seg=-1), solve(rows=None), solve(limits=None),
               solve(result=None), solve(lo=3, hi=-3), solve(lo=-64, hi=64 + 1 / 64), clamp(n_seg=0), clamp(rows=None),
               clamp(result=None), clamp(out=None), clamp(hi=0.01)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert not rows.any()
    assert profile(n_cf=0, arrays=[None, None, None]) == 0 and pick(n_cf=0, arrays=[None, None, None], targets=None) == 0
    # the Python side: its own checks, and the refusal of handles that are not scalar
    assert profile(seg_cf=2 ** 40, off=2 ** 40 - 1, out=rows) == 0 and pick(seg_cf=2 ** 40, off=2 ** 40 - 1) == 0
    rows.zero_()
    for bad in (dict(seg_cf=0), dict(seg_cf=2.5), dict(seg_cf=2 ** 40 + 1), dict(seg_cf=2, first_off=2), dict(seg_cf=2, first_off=-1),
                dict(seg_cf=2, nmr_lo_db=3, nmr_hi_db=-3), dict(seg_cf=2, out=rows[:2]), dict(seg_cf=2, out=rows.int())):
        with pytest.raises(ValueError):
            enc.band_profile_segments(dev, **{"nmr_lo_db": -2, "nmr_hi_db": 2, **bad})
    with pytest.raises(ValueError):
        enc.band_pick_segments(dev, 2, 0, [0, 0])                       # three segments, two targets
    with pytest.raises(ValueError):
        enc.band_pick_segments(dev, 2, 0, [0, 0.5, 0])
    with pytest.raises(ValueError):
        enc.profile_solve_segments(rows, [1] * 7, -2, 2)
    with pytest.raises(ValueError):
        enc.profile_clamp_add(rows, res[:7], -2, 2)
    pcm, sr = vm.fixture_stream()
    _, vq, _, _ = A.pacfile._rate_stream_setup(pcm, sr, vm.CAP_KBPS, True, None, use_vq=True)
    vdev = on_device(vq, synthetic(5, 40))
    with pytest.raises(NotImplementedError):
        vq.band_profile_segments(vdev, 2, 0, -2, 2)
    with pytest.raises(NotImplementedError):
        vq.band_pick_segments(vdev, 2, 0, [0, 0, 0])
    with pytest.raises(NotImplementedError):
        vq.profile_solve_segments(torch.zeros((2, G), dtype=torch.int64, device=vq.device), [1, 1], -2, 2)
    with pytest.raises(NotImplementedError):
        vq.profile_clamp_add(torch.zeros((2, G), dtype=torch.int64, device=vq.device),
                             torch.zeros((2, 4), dtype=torch.int32, device=vq.device), -2, 2)


# ------------------------------------------------------------------------------------------------ 4. end to end
@functools.lru_cache(maxsize=None)
def castanet():
    ex = load_excerpt("castanet")
    return np.ascontiguousarray(ex["pcm"][:len(ex["pcm"]) // 1024 * 1024]), int(ex["sr"])


@functools.lru_cache(maxsize=None)
def one_batch(**kw):
    import audio_codec_amd as A
    pcm, sr = castanet()
    return A.pacfile.encode_stream_abr(pcm, sr, block_switching=True, allocation="band", **kw)


CHUNKS = [1, 5, 12, 4096]


@pytest.mark.parametrize("chunk_hops", CHUNKS)
def test_chunked_segments_equal_one_batch(A, chunk_hops):
    pcm, sr = castanet()
    want = one_batch(kbps_per_channel=96, segment_hops=8)
    got = A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=chunk_hops, block_switching=True,
                                              segment_hops=8)
    assert got == want and want != one_batch(kbps_per_channel=96)


@pytest.mark.parametrize("segment_hops", [3, 8, 32])
@pytest.mark.parametrize("chunk_hops", CHUNKS)
def test_chunked_peak_equals_one_batch(A, chunk_hops, segment_hops):
    pcm, sr = castanet()
    kw = dict(kbps_per_channel=96, segment_hops=segment_hops, peak_kbps_per_channel=128)
    want = one_batch(**kw)
    got = A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=chunk_hops, block_switching=True, **kw)
    assert got == want
    if segment_hops == 8 and chunk_hops == 5:                           # a file size as the stream's size
        kw = dict(max_bytes=len(want) - 1500, segment_hops=8, peak_kbps_per_channel=128)
        want = one_batch(**kw)
        assert len(want) <= kw["max_bytes"]
        assert A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=chunk_hops, block_switching=True, **kw) == want


def test_peak_solve_in_chunks_pins_segments(A):
    """the first pass on its own: floors, stream result and targets are the one-batch peak solve's, and the peak binds"""
    pcm, sr = castanet()
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    n_ch, blocks = cp.nChannels, view.n_frames
    first, count, peaks = A.pacfile.segment_limits(128, n_ch, sr, blocks, 8)
    limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    want = enc.band_solve_peak(enc.band_curve(view, flags, cp.targetBitsPerSample), np.append(first, blocks) * n_ch, peaks,
                               limit)
    hr = A.streaming.HostStreamRateEncoder(enc, n_ch, 5, cp.targetBitsPerSample, block_switching=True)
    hr.analyse(pcm, segment_hops=8, segment_limits=peaks, peak=True)
    assert hr.rows.shape[0] == -(-5 * n_ch // (8 * n_ch)) + 1
    got = hr.solve_peak(limit)
    assert (got["stream_target_nmr_db"], got["stream_met"], got["stream_total_bytes"]) == \
        (want["stream_target_nmr_db"], want["stream_met"], want["stream_total_bytes"])
    for k in ("floor_nmr_db", "target_nmr_db", "pinned"):
        assert np.array_equal(got[k], want[k]), k
    assert got["pinned"].any() and not got["pinned"].all()
    print(f"pinned {int(got['pinned'].sum())} of {len(peaks)} segments")
    # and the segmented first pass
    hr.analyse(pcm, segment_hops=8, segment_limits=peaks)
    seg = hr.solve_segments()
    assert np.array_equal(seg["target_nmr_db"], want["floor_nmr_db"])


def test_chunked_long_only_gain_shape_and_pieces(A, tmp_path):
    ex = load_excerpt("harpsichord")
    pcm, sr = np.ascontiguousarray(ex["pcm"][:14 * 1024]), int(ex["sr"])
    kw = dict(kbps_per_channel=96, segment_hops=3, peak_kbps_per_channel=110)
    want = A.pacfile.encode_stream_abr(pcm, sr, allocation="band", **kw)
    assert A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=4, **kw) == want
    # gain-shape, against encode_stream_vq_abr
    vpcm, vsr = vm.fixture_stream()                         # 4 hops, 6 blocks
    for kw in (dict(segment_hops=2), dict(segment_hops=2, peak_kbps_per_channel=110)):
        want = A.pacfile.encode_stream_vq_abr(vpcm, vsr, kbps_per_channel=96, max_kbps_per_channel=vm.CAP_KBPS,
                                              block_switching=True, **kw)
        got = A.pacfile.encode_stream_abr_chunked(vpcm, vsr, kbps_per_channel=96, chunk_hops=3,
                                                  max_kbps_per_channel=vm.CAP_KBPS, block_switching=True, use_vq=True, **kw)
        assert got == want
    # piece by piece, from an np.memmap
    pcm, sr = castanet()
    path = tmp_path / "pcm.i16"
    pcm.tofile(path)
    mm = np.memmap(path, dtype=np.int16, mode="r", shape=pcm.shape)
    kw = dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=128)
    parts = list(A.pacfile.iter_encode_abr_chunked(mm, sr, chunk_hops=12, block_switching=True, **kw))
    assert len(parts) == 1 + -(-(len(pcm) // 1024) // 12) + 1 and all(isinstance(p, bytes) for p in parts)
    assert parts[0] == A.pacfile.header_bytes(A.pacfile._rate_coding_params(pcm, sr, 320, None))
    assert b"".join(parts) == one_batch(**kw)


def both_messages(A, up_front, **kw):
    """up_front: the iterator form raises when it is called, before the header is given"""
    pcm, sr = castanet()
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, block_switching=True, allocation="band", **kw)
    with pytest.raises(ValueError) as chunked:
        A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, **kw)
    with pytest.raises(ValueError) as pieces:
        it = A.pacfile.iter_encode_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, **kw)
        assert not up_front
        list(it)
    assert str(chunked.value) == str(one.value) == str(pieces.value)
    return str(one.value)


_PEAK = []


def peak_that_a_segment_exceeds(A):
    """the highest peak rate, from 48 kb/s down in steps of 0.5, at which the one-batch peak solve for 96 kb/s reaches the
    stream's size and leaves a segment of 8 blocks beyond its peak -> (kb/s, that solve)"""
    if not _PEAK:
        pcm, sr = castanet()
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
        curve = enc.band_curve(view, flags, cp.targetBitsPerSample)
        n_ch, blocks = cp.nChannels, view.n_frames
        limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
        for kbps in np.arange(48.0, 0.0, -0.5):
            fb, count, peaks = A.pacfile.segment_limits(kbps, n_ch, sr, blocks, 8)
            ref = enc.band_solve_peak(curve, np.append(fb, blocks) * n_ch, peaks, limit)
            if not ref["met"].all():
                assert ref["stream_met"]
                _PEAK.append((float(kbps), {k: ref[k] for k in ("met", "floor_nmr_db", "total_bytes")}))
                break
    assert _PEAK
    return _PEAK[0]


def test_error_messages_are_the_one_batch_call_s(A):
    # a segment that cannot be reached, the stream that cannot be reached
    msg = both_messages(A, True, kbps_per_channel=8, segment_hops=8)
    assert "cannot be reached: its limit is" in msg
    msg = both_messages(A, True, kbps_per_channel=1, segment_hops=8, peak_kbps_per_channel=128)
    assert "cannot be reached: at the highest target" in msg
    found, ref = peak_that_a_segment_exceeds(A)
    s = int(np.argmin(ref["met"]))
    print(f"peak {found} kb/s: met {ref['met'].tolist()}, floors {ref['floor_nmr_db'].tolist()}, first segment {s}")
    # nothing before that segment is in doubt (no reachable segment whose size above its floor exceeds its peak), so it
    # is certain after the first pass and the iterator form raises when it is called, before the header
    pcm, sr = castanet()
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    n_ch = cp.nChannels
    peaks = A.pacfile.segment_limits(found, n_ch, sr, view.n_frames, 8)[2]
    rows = enc.band_profile_segments(enc.band_curve(view, flags, cp.targetBitsPerSample), 8 * n_ch, 0)
    a = enc.profile_solve_segments(rows, peaks)
    assert not a["met"][s] and a["met"][:s].all() and not (a["worst_above"][:s] > peaks[:s]).any()
    msg = both_messages(A, True, kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=found)
    assert "it cannot be reached at all" in msg
    assert f"segment {s} " in msg and "exceeds its peak" in msg


def test_a_segment_that_fits_at_its_floor_only_is_named_in_the_second_pass(A):
    """harpsichord under a cap of 48 kb/s, 32 kb/s wanted, 3-block segments with a peak of 46 kb/s: in the one-batch call
    the first segment beyond its peak is one that fits at its own floor and not at the stream's target (units leave
    their cap as the target rises).  In chunks its row is gone when the stream's target is known: the call itself
    does not raise, the iterator does when that segment ends, with the one-batch message"""
    import re
    ex = load_excerpt("harpsichord")
    pcm, sr = np.ascontiguousarray(ex["pcm"][:len(ex["pcm"]) // 1024 * 1024]), int(ex["sr"])
    kw = dict(kbps_per_channel=32, max_kbps_per_channel=48, segment_hops=3, peak_kbps_per_channel=46, block_switching=True)
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, allocation="band", **kw)
    assert "it fits at its own floor" in str(one.value) and "but not at the stream's target" in str(one.value)
    seg = int(re.match(r"segment (\d+) ", str(one.value)).group(1))
    for chunk_hops in (4, 4096):
        it = A.pacfile.iter_encode_abr_chunked(pcm, sr, chunk_hops=chunk_hops, **kw)          # no raise here
        parts = []
        with pytest.raises(ValueError) as chunked:
            for part in it:
                parts.append(part)
        assert str(chunked.value) == str(one.value)
        hops, last = len(pcm) // 1024, (seg + 1) * 3 - 1                # the segment's last block
        assert last < hops and len(parts) == 1 + last // chunk_hops    # the header and the chunks before that block's
        with pytest.raises(ValueError) as chunked:
            A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=chunk_hops, **kw)
        assert str(chunked.value) == str(one.value)


def test_a_doubtful_segment_defers_the_message_to_the_second_pass(A, monkeypatch):
    """the peak of the test above, with the first pass made to report an earlier segment as doubtful (worst_above beyond
    its peak): nothing is certain up front, the second pass sums the segments, finds the doubtful one within its peak
    and names the same segment with the same message -- from the iterator, after the pieces before it"""
    pcm, sr = castanet()
    kbps, ref = peak_that_a_segment_exceeds(A)
    seg = int(np.argmin(ref["met"]))
    assert seg >= 1 and ref["floor_nmr_db"][seg] == 30                  # an unreachable one, with segments before it
    kw = dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=kbps, block_switching=True)
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, allocation="band", **kw)
    assert f"segment {seg} " in str(one.value)
    real = A.streaming.HostStreamRateEncoder.solve_peak

    def doubtful(self, limit_bytes):
        sol = real(self, limit_bytes)
        assert sol["floor_met"][:seg].all() and not sol["floor_met"][seg]
        sol["worst_above"] = sol["worst_above"].copy()
        sol["worst_above"][seg - 1] = 10 ** 12
        return sol
    monkeypatch.setattr(A.streaming.HostStreamRateEncoder, "solve_peak", doubtful)
    it = A.pacfile.iter_encode_abr_chunked(pcm, sr, chunk_hops=5, **kw)                # no raise here
    parts = []
    with pytest.raises(ValueError) as chunked:
        for part in it:
            parts.append(part)
    assert str(chunked.value) == str(one.value)
    hops, last = len(pcm) // 1024, (seg + 1) * 8 - 1                    # the segment's last block
    assert len(parts) == 1 + (last // 5 if last < hops else -(-hops // 5))          # the header, the chunks before its
    with pytest.raises(ValueError) as chunked:
        A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, **kw)
    assert str(chunked.value) == str(one.value)


def test_a_segment_over_its_limit_is_raised_where_it_ends(A):
    """the second pass's own check, driven by hand: per-segment targets, and a limit one byte below what one segment
    takes -- the raise comes in place of the body of the chunk in which that segment ends"""
    pcm, sr = castanet()
    pcm = pcm[:20 * 1024]
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    n_ch, blocks, S, F = cp.nChannels, view.n_frames, 4, 3
    n_seg = -(-blocks // S)
    targets = np.array([(-3 + 2 * (s % 4)) for s in range(n_seg)], np.float64)
    curve = enc.band_curve(view, flags, cp.targetBitsPerSample)
    n = enc.band_pick_segments(curve, S * n_ch, 0, (targets * GRID).astype(np.int64))["n_bytes"].cpu().numpy().astype(np.int64)
    took = np.array([np.sum(np.where(part > 0, part + 4, 0)) for part in
                     (n[s * S * n_ch:(s + 1) * S * n_ch] for s in range(n_seg))], np.int64)
    hr = A.streaming.HostStreamRateEncoder(enc, n_ch, F, cp.targetBitsPerSample, block_switching=True)
    whole = b"".join(b.tobytes() for b in hr.encode(pcm, targets, segment_hops=S, segment_limits=took))
    assert len(whole) == took.sum()                                     # every segment exactly at its limit: no raise
    for s in (0, 2, n_seg - 1):
        limits = took.copy()
        limits[s] -= 1
        bodies = []
        with pytest.raises(A.streaming.SegmentOverLimit) as err:
            for body in hr.encode(pcm, targets, segment_hops=S, segment_limits=limits):
                bodies.append(body.tobytes())
        assert (err.value.segment, err.value.total_bytes, err.value.limit_bytes) == (s, took[s], took[s] - 1)
        last_block = min((s + 1) * S, blocks) - 1                       # of the segment; chunks of F hops, then the tail's two
        hops = len(pcm) // 1024
        chunk = last_block // F if last_block < hops else -(-hops // F)
        assert len(bodies) == chunk and b"".join(bodies) == whole[:sum(map(len, bodies))]


# ------------------------------------------------------------------------------------------------ 5. nothing existing moves
def test_existing_calls_unchanged_by_the_new_ones(A):
    pcm, sr = castanet()
    pcm = pcm[:12 * 1024]
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    curve = enc.band_curve(view, flags, cp.targetBitsPerSample)
    n_ch, blocks = cp.nChannels, view.n_frames
    first, count, peaks = A.pacfile.segment_limits(128, n_ch, sr, blocks, 4)
    limit = int(enc.band_profile(curve)[1700].item())

    def snapshot():
        out = enc.encode_pack(view, flags)
        pick = enc.band_pick(curve, -1.5)
        sol = enc.band_solve_peak(curve, np.append(first, blocks) * n_ch, peaks, limit)
        return ([out[k].cpu().numpy().copy() for k in ("n_bytes", "bit_alloc", "overall", "status")] +
                [out["payload"].cpu().numpy()[:, :64].copy(), enc.band_profile(curve).cpu().numpy()] +
                [pick[k].cpu().numpy().copy() for k in ("bit_alloc", "n_bytes", "capped")] +
                [sol[k].cpu().numpy().copy() for k in ("bit_alloc", "n_bytes", "capped")] +
                [sol[k] for k in ("target_nmr_db", "met", "total_bytes", "floor_nmr_db")] +
                [np.frombuffer(A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=5,
                                                                   block_switching=True), np.uint8)])
    before = snapshot()
    rows = enc.band_profile_segments(curve, 4 * n_ch, 0)
    res = enc.profile_solve_segments(rows, peaks)
    enc.profile_clamp_add(rows, res["result"])
    enc.band_pick_segments(curve, 4 * n_ch, 0, np.zeros(len(peaks), np.int64))
    A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=5, block_switching=True, segment_hops=4,
                                        peak_kbps_per_channel=128)
    after = snapshot()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
