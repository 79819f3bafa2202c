"""The whole-grid profile of a rate curve and the chunked average-bit-rate encode with allocation="budget" on the GPU
(pacx_rate_profile / pacx_rate_profile_segments / pacx_rate_pick / pacx_rate_pick_segments, the Encoder methods of those
names, streaming.HostStreamRateEncoder(allocation="budget"), the allocation= keyword of
pacfile.encode_stream_abr_chunked / iter_encode_abr_chunked).

Everything here is integers, comparisons and bytes: every check is for equality, there is no tolerance.
  Profile and rows.  On synthetic curves (abr_model.synthetic, rate_profile_model.planted) the GPU's profile and rows are
  the model's threshold route (tests/rate_profile_model.py, which tests/test_rate_profile_model.py holds to the
  definition) for 0 - 5 frames and around the launch's maximum workgroup count, segments of 1, 2, 3, 64 and all frames
  starting at a segment's first and last frame, grids of 1 to PACX_PROFILE_MAX targets; they add up.
  profile_solve on a profile is rate_solve; rate_pick at its target gives its outputs; per segment rate_solve_segments'.
  End to end the chunked calls give the one-batch calls' bytes and messages.  Nothing existing moves.
"""
import functools

import numpy as np
import pytest

import abr_model as am
import rate_profile_model as rp
import seg_profile_model as sp
import segment_model as sm
import vq_band_model as vm
from conftest import load_excerpt

pytestmark = pytest.mark.gpu

GRID = am.GRID
NARROW = (-2 * GRID, 2 * GRID)
PROF_GROUPS = 512           # k_rate_profile.hip: workgroups of one launch at most; beyond it a workgroup walks a run of frames
PROFILE_MAX = rp.PROFILE_MAX
PER_CF = ("budget", "n_bytes", "capped")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def solver(A):
    """a scalar encoder: the calls on a curve's arrays need nothing else of it"""
    return A.context.encoder(44100, 128 / 44.1)


def on_device(enc, c, a=0, b=None):
    import torch
    d = {k: torch.as_tensor(np.ascontiguousarray(c[k][a:b]), device=enc.device) for k in ("worst", "bits", "steps")}
    d["row"], d["sub_stride"] = c["row"], c["sub_stride"]
    return d


@functools.lru_cache(maxsize=None)
def synthetic(n_cf, seed, **kw):
    return am.synthetic(n_cf, 40, 12, seed, **kw)


@functools.lru_cache(maxsize=None)
def frame_rows(n_cf, seed, t_lo, t_hi):
    """the model's profile of every single frame, [n_cf, G]: the rows of any segmentation are sums of these"""
    out = rp.rows(synthetic(n_cf, seed), np.arange(n_cf + 1), t_lo, t_hi)
    out.setflags(write=False)
    return out


def rows_from_frames(per_frame, seg_cf, first_off):
    n_cf = len(per_frame)
    out = np.zeros((-(-(first_off + n_cf) // seg_cf), per_frame.shape[1]), np.int64)
    np.add.at(out, (first_off + np.arange(n_cf)) // seg_cf, per_frame)
    return out


# ------------------------------------------------------------------------------------------------ 1. profile and rows
@pytest.mark.parametrize("n_cf,seed", [(0, 40), (1, 40), (2, 43), (3, 41), (4, 44), (5, 40), (PROF_GROUPS - 1, 50),
                                       (PROF_GROUPS, 51), (PROF_GROUPS + 1, 52), (2 * PROF_GROUPS + 1, 53)])
def test_profile_and_rows_frame_counts_and_segment_lengths(A, n_cf, seed):
    import torch
    enc = solver(A)
    t_lo, t_hi = NARROW
    lo, hi = t_lo / GRID, t_hi / GRID
    G = t_hi - t_lo + 1
    c = synthetic(n_cf, seed)
    dev = on_device(enc, c)
    per_frame = frame_rows(n_cf, seed, t_lo, t_hi)
    whole = enc.rate_profile(dev, lo, hi)
    assert whole.dtype == torch.int64 and tuple(whole.shape) == (G,)
    whole = whole.cpu().numpy()
    assert np.array_equal(whole, per_frame.sum(axis=0))
    if n_cf in (5, PROF_GROUPS + 1):                                    # the model's own whole, not the sum of its rows
        assert np.array_equal(whole, rp.profile_steps(c, t_lo, t_hi))
    # additive: two calls on two halves into one `out` give the whole, on top of what it held
    buf = torch.full((G,), 11, dtype=torch.int64, device=enc.device)
    for a, b in ((0, n_cf // 2), (n_cf // 2, n_cf)):
        assert enc.rate_profile(on_device(enc, c, a, b), lo, hi, out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), whole + 11)
    for seg_cf in (1, 2, 3, 64, n_cf + 3):
        for first_off in sorted({0, seg_cf - 1}):
            want = rows_from_frames(per_frame, seg_cf, first_off)
            got = enc.rate_profile_segments(dev, seg_cf, first_off, lo, hi)
            assert got.dtype == torch.int64 and tuple(got.shape) == want.shape == (-(-(first_off + n_cf) // seg_cf), G)
            assert np.array_equal(got.cpu().numpy(), want), (seg_cf, first_off)
            # a larger buffer, poisoned: a second call adds to the rows, the rows beyond n_seg are left alone
            buf = torch.full((len(want) + 2, G), 7, dtype=torch.int64, device=enc.device)
            buf[:len(want)] = got
            assert enc.rate_profile_segments(dev, seg_cf, first_off, lo, hi, out=buf) is buf
            assert np.array_equal(buf[:len(want)].cpu().numpy(), 2 * want) and bool((buf[len(want):] == 7).all())
    if n_cf:                                                            # one segment is rate_profile
        one = enc.rate_profile_segments(dev, n_cf, 0, lo, hi).cpu().numpy()
        assert one.shape == (1, G) and np.array_equal(one[0], whole)


@pytest.mark.parametrize("t_lo,t_hi,n_cf", [(-3 * GRID, -3 * GRID, 300), (17, 18, 300), (-512, 511, 300), (-512, 512, 300),
                                            (-30 * GRID, 30 * GRID, 5), (-64 * GRID, 64 * GRID, 5)])
def test_profile_grids(A, t_lo, t_hi, n_cf):
    """G = 1, 2, 1024, 1025 (a thread's second entry begins) on 300 frames, a segment boundary inside most workgroups'
    runs; 3841 and PACX_PROFILE_MAX on five, where every thread owns four and nine entries"""
    enc = solver(A)
    assert t_hi - t_lo + 1 in (1, 2, 1024, 1025, 3841, PROFILE_MAX)
    c = synthetic(n_cf, 7)
    dev = on_device(enc, c)
    lo, hi = t_lo / GRID, t_hi / GRID
    assert np.array_equal(enc.rate_profile(dev, lo, hi).cpu().numpy(), rp.profile_steps(c, t_lo, t_hi))
    seg_cf, first_off = (64, 5) if n_cf > 5 else (2, 1)
    want = rp.rows(c, sp.uniform_first(n_cf, seg_cf, first_off), t_lo, t_hi)
    assert np.array_equal(enc.rate_profile_segments(dev, seg_cf, first_off, lo, hi).cpu().numpy(), want)


@pytest.mark.parametrize("kind", ["mixed", "long", "short"])
def test_profile_planted_entries(A, kind):
    """grid points and their neighbours one ulp away, +-inf, NaN (at J too), units outside the range, 1e300, denormals;
    long-only, all-short and mixed frames"""
    enc = solver(A)
    kw = {"mixed": {}, "long": dict(p_short=0.0, p_drop=0.0), "short": dict(p_short=1.0, p_drop=0.0)}[kind]
    for t_lo, t_hi in (NARROW, (0, 1), (5, 5)):
        c = rp.planted(160, 21, t_lo, t_hi, **kw)
        shorts = (c["steps"][:, 1] >= 0).sum()
        assert shorts == {"long": 0, "short": 160}.get(kind, shorts) and (kind != "mixed" or 0 < shorts < 160)
        dev = on_device(enc, c)
        assert np.array_equal(enc.rate_profile(dev, t_lo / GRID, t_hi / GRID).cpu().numpy(), rp.profile_steps(c, t_lo, t_hi))
        for seg_cf, first_off in ((7, 3), (1, 0), (200, 199)):
            want = rp.rows(c, sp.uniform_first(160, seg_cf, first_off), t_lo, t_hi)
            got = enc.rate_profile_segments(dev, seg_cf, first_off, t_lo / GRID, t_hi / GRID)
            assert np.array_equal(got.cpu().numpy(), want), (t_lo, t_hi, seg_cf)


def test_profile_odd_rows(A):
    """units of one and two entries; a row that cuts J; a row too long for the kernel's LDS (8 x 513 entries), which
    the other instance of the kernel reads in place"""
    enc = solver(A)
    t_lo, t_hi = NARROW
    lo, hi = t_lo / GRID, t_hi / GRID
    rng = np.random.default_rng(3)
    cases = []
    for J in (0, 1):
        n_cf, sub = 24, 2
        c = {"worst": rng.uniform(-3, 3, (n_cf, 8 * sub)), "bits": rng.integers(50, 900, (n_cf, 8 * sub)).astype(np.int32),
             "steps": np.full((n_cf, am.SUB), -1, np.int32), "row": 8 * sub, "sub_stride": sub}
        c["steps"][: n_cf // 2, 0] = J
        c["steps"][n_cf // 2:, :] = J
        c["steps"][-1, :] = -1
        cases.append(c)
    full = am.synthetic(80, 40, 4, 9, p_short=0.5)
    cases.append(rp.narrowed(full, 7 * full["sub_stride"] + 1))
    assert (rp.cut(cases[-1])["steps"] < cases[-1]["steps"]).any()
    long_row = rp.planted(12, 5, t_lo, t_hi, j_long=2000, j_short=600)             # J < 2048: the bound on the halvings
    assert long_row["row"] > 8 * 513 and (long_row["steps"][:, 1] > 512).any() and (long_row["steps"][:, 1] < 0).any()
    cases.append(long_row)
    for c in cases:
        dev = on_device(enc, c)
        assert np.array_equal(enc.rate_profile(dev, lo, hi).cpu().numpy(), rp.profile_steps(c, t_lo, t_hi))
        first = sp.uniform_first(len(c["steps"]), 5, 2)
        assert np.array_equal(enc.rate_profile_segments(dev, 5, 2, lo, hi).cpu().numpy(), rp.rows(c, first, t_lo, t_hi))
        for t in (t_lo, 3, t_hi):
            got, want = enc.rate_pick(dev, t / GRID), rp.pick(c, t)
            for k in PER_CF:
                assert np.array_equal(got[k].cpu().numpy(), want[k]), (k, t)


# ------------------------------------------------------------------------------------------------ 2. solve and pick
@functools.lru_cache(maxsize=None)
def castanet():
    ex = load_excerpt("castanet")
    return np.ascontiguousarray(ex["pcm"][:len(ex["pcm"]) // 1024 * 1024]), int(ex["sr"])


def gpu_curve(A, block_switching=True):
    """the GPU's own curve of the castanet excerpt: (encoder, curve, flags, n_ch, blocks)"""
    pcm, sr = castanet()
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, block_switching, None)
    return enc, enc.rate_curve(view, flags, cp.targetBitsPerSample), flags, cp.nChannels, view.n_frames


def check_solve_and_pick(enc, dev, flags, limits, lo, hi):
    """profile_solve on rate_profile is rate_solve; rate_pick at the target it returns gives its per-frame outputs"""
    prof = enc.rate_profile(dev, lo, hi)
    met = []
    for limit in limits:
        want = enc.rate_solve(dev, flags, limit, lo, hi)
        got = enc.profile_solve(prof, limit, lo, hi)
        assert (got["target_nmr_db"], got["met"], got["total_bytes"]) == \
            (want["target_nmr_db"], want["met"], want["total_bytes"]), limit
        pick = enc.rate_pick(dev, want["target_nmr_db"])
        for k in PER_CF:
            assert np.array_equal(pick[k].cpu().numpy(), want[k].cpu().numpy()), (k, limit)
        met.append(want["met"])
    return met, prof.cpu().numpy()


@pytest.mark.parametrize("n_cf,seed", [(300, 7), (2 * PROF_GROUPS + 1, 53)])
def test_profile_solve_is_rate_solve_on_synthetic_curves(A, n_cf, seed):
    enc = solver(A)
    c = synthetic(n_cf, seed)
    t_lo, t_hi = NARROW
    small, big = am.total(c, t_hi), am.total(c, t_lo)
    met, prof = check_solve_and_pick(enc, on_device(enc, c), None, [(small + big) // 2, small - 1, small, big, 10 ** 12],
                                     t_lo / GRID, t_hi / GRID)
    assert met == [True, False, True, True, True] and prof[0] == big and prof[-1] == small
    want = am.solve(c, (small + big) // 2, t_lo, t_hi)                  # and the model's, once
    got = enc.profile_solve(enc.rate_profile(on_device(enc, c), t_lo / GRID, t_hi / GRID), (small + big) // 2,
                            t_lo / GRID, t_hi / GRID)
    assert (got["target_nmr_db"] * GRID, got["met"], got["total_bytes"]) == (want["t"], bool(want["met"]), want["total"])


@pytest.mark.parametrize("block_switching", [True, False])
def test_profile_solve_is_rate_solve_on_the_gpus_own_curve(A, block_switching):
    enc, curve, flags, n_ch, blocks = gpu_curve(A, block_switching)
    if block_switching:
        assert bool((curve["steps"][:, 1] >= 0).any()) and bool((curve["steps"][:, 1] < 0).any())     # short and long frames
    prof = enc.rate_profile(curve).cpu().numpy()
    small, big = int(prof[-1]), int(prof[0])
    assert big > small > 0
    met, _ = check_solve_and_pick(enc, curve, flags, [(small + big) // 2, small - 1, small, 10 ** 12], -30, 30)
    assert met == [True, False, True, True]
    # the rows of uniform segments: their solve is rate_solve_segments', their picks its outputs
    seg_cf = 8 * n_ch
    n_cf = blocks * n_ch
    first = sp.uniform_first(n_cf, seg_cf, 0)
    rows = enc.rate_profile_segments(curve, seg_cf, 0)
    assert np.array_equal(rows.sum(dim=0).cpu().numpy(), prof)
    top, bottom = rows[:, -1].cpu().numpy(), rows[:, 0].cpu().numpy()
    limits = np.where(np.arange(len(top)) % 3 == 1, np.maximum(top - 1, 0), (top + bottom) // 2)
    want = enc.rate_solve_segments(curve, first, limits)
    got = enc.profile_solve_segments(rows, limits)
    for k in ("target_nmr_db", "met", "total_bytes"):
        assert np.array_equal(got[k], want[k]), k
    assert want["met"].any() and not want["met"].all()
    pick = enc.rate_pick_segments(curve, seg_cf, 0, np.round(want["target_nmr_db"] * GRID).astype(np.int64))
    for k in PER_CF:
        assert np.array_equal(pick[k].cpu().numpy(), want[k].cpu().numpy()), k


@pytest.mark.parametrize("n_cf,seg_cf,first_off", [(300, 7, 3), (5, 1, 0), (513, 64, 63), (41, 100, 99)])
def test_pick_segments_is_rate_pick_per_slice(A, n_cf, seg_cf, first_off):
    enc = solver(A)
    c = synthetic(n_cf, 7)
    dev = on_device(enc, c)
    first = sp.uniform_first(n_cf, seg_cf, first_off)
    t = np.random.default_rng(5).integers(-2 * GRID, 2 * GRID + 1, len(first) - 1)
    got = enc.rate_pick_segments(dev, seg_cf, first_off, t)
    want = rp.pick_segments(c, first, t)
    for k in PER_CF:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    same = enc.rate_pick_segments(dev, seg_cf, first_off, np.full(len(t), 37))
    plain = enc.rate_pick(dev, 37 / GRID)
    model = rp.pick(c, 37)
    for k in PER_CF:
        assert np.array_equal(same[k].cpu().numpy(), plain[k].cpu().numpy()), k
        assert np.array_equal(plain[k].cpu().numpy(), model[k]), k
    if n_cf == 300:
        assert got["capped"].any() and not got["capped"].all()
        # per-segment targets from the segmented solve: its outputs
        limits = sm.limits_for("rate", c, first, *NARROW)
        sol = enc.rate_solve_segments(dev, first, limits, -2, 2)
        pick = enc.rate_pick_segments(dev, seg_cf, first_off, np.round(sol["target_nmr_db"] * GRID).astype(np.int64))
        for k in PER_CF:
            assert np.array_equal(pick[k].cpu().numpy(), sol[k].cpu().numpy()), k


def test_arguments_and_refusals(A):
    import ctypes
    import torch
    enc = solver(A)
    c = synthetic(5, 40)
    dev = on_device(enc, c)
    ptr = A.engine._ptr
    G = 257
    rows = torch.zeros((8, G), dtype=torch.int64, device=enc.device)
    t = torch.zeros(8, dtype=torch.int32, device=enc.device)
    bud = torch.zeros((5, 8), dtype=torch.int32, device=enc.device)
    nby, cpd = torch.zeros(5, dtype=torch.int32, device=enc.device), torch.zeros(5, dtype=torch.uint8, device=enc.device)
    i64, i32, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    curve = [ptr(dev[k]) for k in ("worst", "bits", "steps")]
    row, sub = c["row"], c["sub_stride"]

    def profile(n_cf=5, row=row, sub=sub, seg_cf=2, off=0, lo=-2.0, hi=2.0, out=rows, arrays=curve):
        return enc.lib.pacx_rate_profile_segments(enc.h, i64(n_cf), i32(row), i32(sub), *arrays, i64(seg_cf), i64(off),
                                                  f64(lo), f64(hi), ptr(out) if out is not None else None, None)

    def whole(n_cf=5, row=row, sub=sub, lo=-2.0, hi=2.0, out=rows, arrays=curve):
        return enc.lib.pacx_rate_profile(enc.h, i64(n_cf), i32(row), i32(sub), *arrays, f64(lo), f64(hi),
                                         ptr(out) if out is not None else None, None)

    def pick(n_cf=5, row=row, sub=sub, target=0.5, arrays=curve, budget=bud):
        return enc.lib.pacx_rate_pick(enc.h, i64(n_cf), i32(row), i32(sub), *arrays, f64(target),
                                      ptr(budget) if budget is not None else None, ptr(nby), ptr(cpd), None)

    def pick_seg(n_cf=5, row=row, sub=sub, seg_cf=2, off=0, targets=t, arrays=curve):
        return enc.lib.pacx_rate_pick_segments(enc.h, i64(n_cf), i32(row), i32(sub), *arrays, i64(seg_cf), i64(off),
                                               ptr(targets) if targets is not None else None, ptr(bud), ptr(nby), ptr(cpd),
                                               None)
    E_ARG = A._lib.E_ARG
    assert profile() == 0 and whole() == 0 and pick() == 0 and pick_seg() == 0
    rows.zero_()
    none = [None, curve[1], curve[2]]
    for rc in (profile(seg_cf=0), profile(seg_cf=-1), profile(off=2), profile(off=-1), profile(n_cf=-1), profile(out=None),
               profile(arrays=none), profile(lo=3, hi=-3), profile(lo=0.01), profile(lo=-64, hi=64 + 1 / 64),
               profile(lo=float("nan")), profile(seg_cf=2 ** 40 + 1), profile(row=7 * sub), profile(sub=0),
               whole(n_cf=-1), whole(out=None), whole(arrays=none), whole(lo=3, hi=-3), whole(hi=0.01),
               whole(lo=-64, hi=64 + 1 / 64), whole(hi=float("inf")), whole(row=7 * sub), whole(sub=0),
               pick(n_cf=-1), pick(arrays=none), pick(budget=None), pick(target=0.01), pick(target=float("nan")),
               pick(target=float("inf")), pick(row=7 * sub), pick(sub=0),
               pick_seg(seg_cf=2 ** 40 + 1), pick_seg(seg_cf=0), pick_seg(off=2), pick_seg(off=-1), pick_seg(n_cf=-1),
               pick_seg(targets=None), pick_seg(arrays=none), pick_seg(row=7 * sub)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert not rows.any()
    nothing = [None, None, None]
    assert profile(n_cf=0, arrays=nothing) == 0 and whole(n_cf=0, arrays=nothing) == 0 and \
        pick(n_cf=0, arrays=nothing, budget=None) == 0 and pick_seg(n_cf=0, arrays=nothing, targets=None) == 0
    torch.cuda.synchronize()
    assert not rows.any()                                               # n_cf = 0 adds nothing
    # the Python side: the band siblings' checks
    for bad in (dict(seg_cf=0), dict(seg_cf=2.5), dict(seg_cf=2 ** 40 + 1), dict(seg_cf=2, first_off=2),
                dict(seg_cf=2, first_off=-1), dict(seg_cf=2, nmr_lo_db=3, nmr_hi_db=-3), dict(seg_cf=2, out=rows[:2]),
                dict(seg_cf=2, out=rows.int())):
        with pytest.raises(ValueError):
            enc.rate_profile_segments(dev, **{"nmr_lo_db": -2, "nmr_hi_db": 2, **bad})
    for bad in (dict(nmr_lo_db=3, nmr_hi_db=-3), dict(nmr_lo_db=-70, nmr_hi_db=70), dict(out=rows[0, :5])):
        with pytest.raises(ValueError):
            enc.rate_profile(dev, **{"nmr_lo_db": -2, "nmr_hi_db": 2, **bad})
    with pytest.raises(ValueError):
        enc.rate_pick_segments(dev, 2, 0, [0, 0])                       # three segments, two targets
    with pytest.raises(ValueError):
        enc.rate_pick_segments(dev, 2, 0, [0, 0.5, 0])
    with pytest.raises(ValueError):
        enc.rate_profile({**dev, "bits": dev["bits"][:, :5]})
    with pytest.raises(A._lib.PacxError):
        enc.rate_pick(dev, 0.01)                                        # off the grid
    # handles that are not scalar answer NotImplementedError to all four
    for other in (A.context.encoder(44100, 96 / 44.1, use_vq=True), A.context.encoder(44100, 96 / 44.1, use_vq=True, use_sbr=True)):
        odev = on_device(other, c)
        for call in (lambda: other.rate_profile(odev, -2, 2), lambda: other.rate_profile_segments(odev, 2, 0, -2, 2),
                     lambda: other.rate_pick(odev, 0.5), lambda: other.rate_pick_segments(odev, 2, 0, [0, 0, 0])):
            with pytest.raises(NotImplementedError):
                call()


# ------------------------------------------------------------------------------------------------ 3. end to end
@functools.lru_cache(maxsize=None)
def one_batch(stream, block_switching, **kw):
    import audio_codec_amd as A
    pcm, sr = castanet() if stream == "castanet" else vm.fixture_stream()
    return A.pacfile.encode_stream_abr(pcm, sr, block_switching=block_switching, allocation="budget", **kw)


@pytest.mark.parametrize("block_switching", [True, False])
@pytest.mark.parametrize("chunk_hops", [1, 3, 4, 4096])
def test_chunked_budget_equals_one_batch_on_the_fixture_stream(A, chunk_hops, block_switching):
    """four hops: chunks of one block, of three and one, of all and of more blocks than there are"""
    pcm, sr = vm.fixture_stream()
    for kw in (dict(), dict(segment_hops=3), dict(segment_hops=8)):
        want = one_batch("fixture", block_switching, kbps_per_channel=96, **kw)
        got = A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=chunk_hops,
                                                  block_switching=block_switching, allocation="budget", **kw)
        assert got == want, kw
    assert one_batch("fixture", block_switching, kbps_per_channel=96) != \
        A.pacfile.encode_stream_abr(pcm, sr, 96, block_switching=block_switching, allocation="band")


@pytest.mark.parametrize("kw", [dict(), dict(segment_hops=3), dict(segment_hops=8),
                                dict(segment_hops=8, peak_kbps_per_channel=128),
                                dict(segment_hops=3, peak_kbps_per_channel=128)], ids=str)
@pytest.mark.parametrize("chunk_hops", [1, 5, 4096])
def test_chunked_budget_equals_one_batch_on_castanet(A, chunk_hops, kw):
    pcm, sr = castanet()
    want = one_batch("castanet", True, kbps_per_channel=96, **kw)
    got = A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=chunk_hops, block_switching=True,
                                              allocation="budget", **kw)
    assert got == want
    if kw and chunk_hops == 5:
        assert want != one_batch("castanet", True, kbps_per_channel=96)    # the segments bind


def test_chunked_budget_all_blocks_without_block_switching_and_a_file_size(A):
    pcm, sr = castanet()
    hops = len(pcm) // 1024
    want = one_batch("castanet", False, kbps_per_channel=96)
    assert A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=hops, allocation="budget") == want
    kw = dict(max_bytes=len(want) - 1500, segment_hops=8, peak_kbps_per_channel=128)
    want = one_batch("castanet", True, **kw)
    assert len(want) <= kw["max_bytes"]
    assert A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, allocation="budget", **kw) == want


def test_peak_solve_in_chunks_pins_segments(A):
    """the first pass on its own: floors, stream result and targets are the one-batch peak solve's, and the peak binds"""
    pcm, sr = castanet()
    enc, curve, flags, n_ch, blocks = gpu_curve(A)
    first, count, peaks = A.pacfile.segment_limits(128, n_ch, sr, blocks, 8)
    limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    want = enc.rate_solve_peak(curve, np.append(first, blocks) * n_ch, peaks, limit)
    hr = A.streaming.HostStreamRateEncoder(enc, n_ch, 5, 320 / (sr / 1000), block_switching=True, allocation="budget")
    hr.analyse(pcm, segment_hops=8, segment_limits=peaks, peak=True)
    got = hr.solve_peak(limit)
    assert (got["stream_target_nmr_db"], got["stream_met"], got["stream_total_bytes"]) == \
        (want["stream_target_nmr_db"], want["stream_met"], want["stream_total_bytes"])
    for k in ("floor_nmr_db", "target_nmr_db", "pinned"):
        assert np.array_equal(got[k], want[k]), k
    assert got["pinned"].any() and not got["pinned"].all()              # castanet: segments are pinned
    # the stream's profile by quality.stream_rate_profile is rate_profile of the whole curve
    targets, total = A.quality.stream_rate_profile(pcm, sr, chunk_hops=7, block_switching=True, allocation="budget")
    assert np.array_equal(total, enc.rate_profile(curve).cpu().numpy()) and targets[0] == -30 and targets[-1] == 30


def test_pieces_concatenate(A, tmp_path):
    pcm, sr = castanet()
    path = tmp_path / "pcm.i16"
    pcm.tofile(path)
    mm = np.memmap(path, dtype=np.int16, mode="r", shape=pcm.shape)
    kw = dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=128)
    parts = list(A.pacfile.iter_encode_abr_chunked(mm, sr, chunk_hops=12, block_switching=True, allocation="budget", **kw))
    assert len(parts) == 1 + -(-(len(pcm) // 1024) // 12) + 1 and all(isinstance(p, bytes) for p in parts)
    assert parts[0] == A.pacfile.header_bytes(A.pacfile._rate_coding_params(pcm, sr, 320, None))
    assert b"".join(parts) == one_batch("castanet", True, **kw)
    # positional calls as before the keyword: the band stream
    assert A.pacfile.encode_stream_abr_chunked(pcm, sr, 96, None, 12, 320, True) == \
        A.pacfile.encode_stream_abr(pcm, sr, 96, block_switching=True, allocation="band")


def both_messages(A, up_front, **kw):
    """up_front: the iterator form raises when it is called, before the header is given"""
    pcm, sr = castanet()
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, block_switching=True, allocation="budget", **kw)
    with pytest.raises(ValueError) as chunked:
        A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, allocation="budget", **kw)
    with pytest.raises(ValueError) as pieces:
        it = A.pacfile.iter_encode_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, allocation="budget", **kw)
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
        enc, curve, flags, n_ch, blocks = gpu_curve(A)
        limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
        for kbps in np.arange(48.0, 0.0, -0.5):
            fb, count, peaks = A.pacfile.segment_limits(kbps, n_ch, sr, blocks, 8)
            ref = enc.rate_solve_peak(curve, np.append(fb, blocks) * n_ch, peaks, limit)
            if not ref["met"].all():
                assert ref["stream_met"]
                _PEAK.append((float(kbps), {k: ref[k] for k in ("met", "floor_nmr_db", "total_bytes")}))
                break
    assert _PEAK
    return _PEAK[0]


def test_error_messages_are_the_one_batch_call_s(A):
    msg = both_messages(A, True, kbps_per_channel=8, segment_hops=8)
    assert "cannot be reached: its limit is" in msg
    msg = both_messages(A, True, kbps_per_channel=1)
    assert "cannot be reached: at the highest target" in msg
    msg = both_messages(A, True, kbps_per_channel=1, segment_hops=8, peak_kbps_per_channel=128)
    assert "cannot be reached: at the highest target" in msg
    found, ref = peak_that_a_segment_exceeds(A)
    s = int(np.argmin(ref["met"]))
    print(f"peak {found} kb/s: met {ref['met'].tolist()}, floors {ref['floor_nmr_db'].tolist()}, first segment {s}")
    # whether the iterator form raises up front or at that segment's end depends on the segments before it (a doubtful
    # one defers the message): either way the three messages are one
    pcm, sr = castanet()
    kw = dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=found, block_switching=True, allocation="budget")
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, **kw)
    assert f"segment {s} " in str(one.value) and "exceeds its peak" in str(one.value)
    with pytest.raises(ValueError) as chunked:
        A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, **kw)
    with pytest.raises(ValueError) as pieces:
        list(A.pacfile.iter_encode_abr_chunked(pcm, sr, chunk_hops=5, **kw))
    assert str(chunked.value) == str(one.value) == str(pieces.value)


def test_a_doubtful_segment_defers_the_message_to_the_second_pass(A, monkeypatch):
    """the peak of the test above, with the first pass made to report an earlier segment as doubtful (worst_above beyond
    its peak): nothing is certain up front, the second pass sums the segments' records as rate_pick_segments gives them,
    finds the doubtful one within its peak and names the same segment with the same message -- from the iterator,
    after the pieces before it"""
    pcm, sr = castanet()
    kbps, ref = peak_that_a_segment_exceeds(A)
    seg = int(np.argmin(ref["met"]))
    kw = dict(kbps_per_channel=96, segment_hops=8, peak_kbps_per_channel=kbps, block_switching=True, allocation="budget")
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, **kw)
    assert f"segment {seg} " in str(one.value)
    assert seg >= 1                                                     # there are segments before it
    real = A.streaming.HostStreamRateEncoder.solve_peak

    def doubtful(self, limit_bytes):
        sol = real(self, limit_bytes)
        assert sol["floor_met"][:seg].all()
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


def test_harpsichord_under_a_tight_cap_gives_what_one_batch_gives(A):
    """harpsichord under a cap of 48 kb/s, 32 kb/s wanted, 3-block segments with a peak of 46 kb/s -- where the band
    stream has a segment that fits at its floor only: whatever the one-batch call does here, bytes or message, the
    chunked call does"""
    ex = load_excerpt("harpsichord")
    pcm, sr = np.ascontiguousarray(ex["pcm"][:len(ex["pcm"]) // 1024 * 1024]), int(ex["sr"])
    kw = dict(kbps_per_channel=32, max_kbps_per_channel=48, segment_hops=3, peak_kbps_per_channel=46, block_switching=True,
              allocation="budget")

    def outcome(call):
        try:
            return call()
        except ValueError as e:
            return str(e)
    want = outcome(lambda: A.pacfile.encode_stream_abr(pcm, sr, **kw))
    print("one batch:", want if isinstance(want, str) else f"{len(want)} bytes")
    for chunk_hops in (4, 4096):
        assert outcome(lambda: A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=chunk_hops, **kw)) == want
        assert outcome(lambda: b"".join(A.pacfile.iter_encode_abr_chunked(pcm, sr, chunk_hops=chunk_hops, **kw))) == want


# ------------------------------------------------------------------------------------------------ 4. nothing existing moves
def test_existing_calls_unchanged_by_the_new_ones(A):
    pcm, sr = castanet()
    pcm = pcm[:12 * 1024]
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    curve = enc.rate_curve(view, flags, cp.targetBitsPerSample)
    n_ch, blocks = cp.nChannels, view.n_frames
    first, count, peaks = A.pacfile.segment_limits(128, n_ch, sr, blocks, 4)
    limit = int(enc.rate_profile(curve)[1700].item())

    def snapshot():
        out = enc.encode_pack(view, flags)
        sol = enc.rate_solve(curve, flags, limit)
        head = A.pacfile.header_bytes(A.pacfile._rate_coding_params(pcm, sr, 320, None))
        hs = A.streaming.HostStreamEncoder(enc, n_ch, 5, block_switching=True)
        return ([out[k].cpu().numpy().copy() for k in ("n_bytes", "bit_alloc", "overall", "status")] +
                [out["payload"].cpu().numpy()[:, :64].copy()] +
                [sol[k].cpu().numpy().copy() for k in PER_CF] +
                [np.array([sol["target_nmr_db"], sol["met"], sol["total_bytes"]])] +
                [np.frombuffer(A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=5,
                                                                   block_switching=True), np.uint8)] +
                [np.frombuffer(b"".join(bytes(b) for b in hs.encode(pcm)), np.uint8), np.frombuffer(head, np.uint8)])
    before = snapshot()
    assert bytes(before[-3]) == A.pacfile.encode_stream_abr(pcm, sr, 96, block_switching=True, allocation="band")
    rows = enc.rate_profile_segments(curve, 4 * n_ch, 0)
    res = enc.profile_solve_segments(rows, peaks)
    enc.profile_clamp_add(rows, res["result"])
    enc.rate_pick(curve, -1.5)
    enc.rate_pick_segments(curve, 4 * n_ch, 0, np.zeros(len(peaks), np.int64))
    A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=5, block_switching=True, segment_hops=4,
                                        peak_kbps_per_channel=128, allocation="budget")
    after = snapshot()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
