"""The whole-grid rate profile and the chunked average-bit-rate encode on the GPU (pacx_band_profile /
pacx_profile_solve, Encoder.band_profile / profile_solve, streaming.HostStreamRateEncoder,
pacfile.encode_stream_abr_chunked / iter_encode_abr_chunked, quality.stream_rate_profile).

Everything here is integers, comparisons and bytes: every check is for equality, there is no tolerance.
  Profile.  On synthetic curves (tests/band_model.synthetic, tests/profile_model.planted) the GPU's profile is the
  model's -- which tests/test_profile_model.py holds to band_model.total at every target -- for 0, 1, 3, 4, 5 frames, for
  one frame below, at and above the 512 frames the kernel's workgroups take per trip, for grids of 1, 2, 257, 3841 and
  PACX_PROFILE_MAX targets; it is additive; on the GPU's own curve of a block-switched excerpt it is what band_pick
  gives.  Solve.  profile_solve is band_solve on the same curve.  End to end.  The chunked encode gives the one-batch
  call's bytes for chunks of 1, 5, all and more than all blocks, with and without block switching, for the gain-shape
  coder too, and raises its message when the size cannot be reached.  Nothing existing moves.
"""
import ctypes
import functools

import numpy as np
import pytest

import band_model as bm
import profile_model as pm
import vq_band_model as vm
from conftest import load_excerpt

pytestmark = pytest.mark.gpu

GRID = bm.GRID
PER_TRIP = 512              # frames the workgroups of k_band_profile take per trip (PROF_GROUPS, one each)


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def solver(A):
    """a scalar encoder on the band tables of band_model.synthetic"""
    return A.context.encoder(44100, 128 / 44.1)


def on_device(enc, c, a=0, b=None):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(c[k][a:b]), device=enc.device) for k in ("nmr", "cap", "cap_alloc")}


@functools.lru_cache(maxsize=None)
def synthetic(n_cf, seed, cap_scale=1.0):
    return bm.synthetic(n_cf, seed, cap_scale=cap_scale)


@functools.lru_cache(maxsize=None)
def model_profile(n_cf, seed, t_lo, t_hi, cap_scale=1.0):
    return pm.profile(synthetic(n_cf, seed, cap_scale), t_lo, t_hi)


def excerpt(name, h0, h1):
    ex = load_excerpt(name)
    return np.ascontiguousarray(ex["pcm"][h0 * 1024:h1 * 1024]), int(ex["sr"])


# ------------------------------------------------------------------------------------------------ 1. the profile
# (frames, seed): one frame that is short-coded (8 units), long-coded, dropped; a few frames with a dropped one first
@pytest.mark.parametrize("n_cf,seed", [(0, 40), (1, 40), (1, 44), (1, 41), (3, 41), (4, 41), (5, 40), (PER_TRIP - 1, 50),
                                       (PER_TRIP, 51), (PER_TRIP + 1, 52)])
def test_profile_frame_counts(A, n_cf, seed):
    enc = solver(A)
    t_lo, t_hi = -2 * GRID, 2 * GRID
    c = synthetic(n_cf, seed)
    got = enc.band_profile(on_device(enc, c), t_lo / GRID, t_hi / GRID).cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (t_hi - t_lo + 1,)
    assert np.array_equal(got, model_profile(n_cf, seed, t_lo, t_hi))
    assert (got > 0).all() == bool((c["cap"] >= 0).any())


@pytest.mark.parametrize("t_lo,t_hi", [(-3 * GRID, -3 * GRID), (17, 18), (-2 * GRID, 2 * GRID), (-30 * GRID, 30 * GRID),
                                       (-64 * GRID, 64 * GRID)])
def test_profile_grids(A, t_lo, t_hi):
    """G = 1, 2, 257, 3841 and PACX_PROFILE_MAX on 300 frames (more than one tile per thread from 1025 targets on)"""
    enc = solver(A)
    assert t_hi - t_lo + 1 in (1, 2, 257, 3841, pm.PROFILE_MAX)
    got = enc.band_profile(on_device(enc, synthetic(300, 7)), t_lo / GRID, t_hi / GRID).cpu().numpy()
    assert np.array_equal(got, model_profile(300, 7, t_lo, t_hi))


@pytest.mark.parametrize("cap_scale", [1.0, 0.2])
def test_profile_planted_entries(A, cap_scale):
    """grid points and their neighbours one ulp away, +-inf, NaN, rows outside the range, huge and denormal values;
    cap_scale 0.2: many units take cap_alloc"""
    enc = solver(A)
    for t_lo, t_hi in ((-2 * GRID, 2 * GRID), (0, 1), (5, 5)):
        c = pm.planted(160, 21, t_lo, t_hi, cap_scale=cap_scale)
        got = enc.band_profile(on_device(enc, c), t_lo / GRID, t_hi / GRID).cpu().numpy()
        assert np.array_equal(got, pm.profile(c, t_lo, t_hi)), (t_lo, t_hi)


def test_profile_range_errors(A):
    import torch
    enc = solver(A)
    dev = on_device(enc, synthetic(3, 43))
    step = 1.0 / GRID
    for lo, hi in ((-64, 64 + step), (3, -3), (0.01, 3), (-3, 0.01), (float("nan"), 3), (-3, float("inf")),
                   (-2.0 ** 21, -2.0 ** 21 + 1)):
        with pytest.raises(ValueError):
            enc.band_profile(dev, lo, hi)
        with pytest.raises(ValueError):
            enc.profile_solve(torch.zeros(5, dtype=torch.int64, device=enc.device), 10, lo, hi)
        # and the C side on its own
        out = torch.zeros(pm.PROFILE_MAX + 1, dtype=torch.int64, device=enc.device)
        rc = enc.lib.pacx_band_profile(enc.h, ctypes.c_int64(3), *(ctypes.c_void_p(dev[k].data_ptr()) for k in
                                                                   ("nmr", "cap", "cap_alloc")), ctypes.c_double(lo),
                                       ctypes.c_double(hi), ctypes.c_void_p(out.data_ptr()), enc._stream())
        assert rc == A._lib.E_ARG
        res = torch.zeros(4, dtype=torch.int32, device=enc.device)
        rc = enc.lib.pacx_profile_solve(enc.h, ctypes.c_void_p(out.data_ptr()), ctypes.c_int64(10), ctypes.c_double(lo),
                                        ctypes.c_double(hi), ctypes.c_void_p(res.data_ptr()), enc._stream())
        assert rc == A._lib.E_ARG
        torch.cuda.synchronize()
        assert not out.any()
    # a profile of another length, type or place; a negative limit
    good = enc.band_profile(dev, -2, 2)
    for bad in (good[:-1], good.int(), good.cpu(), good.cpu().numpy(), torch.zeros((2, 257), dtype=torch.int64,
                                                                                  device=enc.device)[:, 0]):
        with pytest.raises(ValueError):
            enc.band_profile(dev, -2, 2, out=bad)
        with pytest.raises(ValueError):
            enc.profile_solve(bad, 10, -2, 2)
    with pytest.raises(ValueError):
        enc.profile_solve(good, -1, -2, 2)
    with pytest.raises(ValueError):
        enc.band_profile({"nmr": dev["nmr"][:, :-1], "cap": dev["cap"], "cap_alloc": dev["cap_alloc"]}, -2, 2)


def test_profile_is_additive(A):
    import torch
    enc = solver(A)
    c = synthetic(300, 7)
    t_lo, t_hi = -30 * GRID, 30 * GRID
    want = model_profile(300, 7, t_lo, t_hi)
    out = torch.full((len(want),), 7, dtype=torch.int64, device=enc.device)
    for a, b in ((0, 150), (150, 300)):
        back = enc.band_profile(on_device(enc, c, a, b), -30, 30, out=out)
        assert back is out
    assert np.array_equal(out.cpu().numpy(), want + 7)
    enc.band_profile(on_device(enc, c, 0, 0), -30, 30, out=out)               # no frames: nothing is added
    assert np.array_equal(out.cpu().numpy(), want + 7)


@functools.lru_cache(maxsize=None)
def castanet():
    """12 hops of the castanet excerpt, short-coded hops among them: (pcm, sr)"""
    return excerpt("castanet", 20, 32)


_GPU = {}


def gpu_curve(A):
    """the GPU's own band curve of the block-switched castanet stream, once"""
    if not _GPU:
        pcm, sr = castanet()
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
        curve = enc.band_curve(view, flags, cp.targetBitsPerSample)
        assert (curve["cap"][:, 1] >= 0).any() and (curve["cap"][:, 1] < 0).any()          # short- and long-coded frames
        _GPU.update(enc=enc, curve=curve, profile=enc.band_profile(curve).cpu().numpy())
    return _GPU


def test_profile_is_what_band_pick_gives(A):
    g = gpu_curve(A)
    enc, prof = g["enc"], g["profile"]
    assert prof.shape == (3841,)
    for i in (0, 1, 63, 64, 500, 1000, 1500, 1920, 2047, 2400, 3000, 3500, 3839, 3840):
        n = enc.band_pick(g["curve"], -30 + i / GRID)["n_bytes"].cpu().numpy().astype(np.int64)
        assert prof[i] == int(np.sum(n[n > 0] + 4)), i
    assert len(set(prof.tolist())) > 100


# ------------------------------------------------------------------------------------------------ 2. the solve
def limits_for(prof, path_totals):
    top = int(prof[-1])
    return [0, top - 1, top // 2, top, top + 1, int(prof[0]), int(prof[0]) + 5, int(prof.max()) + 1,
            int(prof[len(prof) // 3])] + list(path_totals) + [v - 1 for v in path_totals] + [v + 1 for v in path_totals]


def check_solve(enc, curve, prof_dev, prof, lo, hi):
    t_lo, t_hi = int(lo * GRID), int(hi * GRID)
    path = [tot for _, tot in _path(prof, int(prof[len(prof) // 2]), t_lo, t_hi)]
    unmet = 0
    for limit in limits_for(prof, path):
        want = enc.band_solve(curve, limit, lo, hi)
        got = enc.profile_solve(prof_dev, limit, lo, hi)
        assert set(got) == {"target_nmr_db", "met", "total_bytes"}
        assert (got["target_nmr_db"], got["met"], got["total_bytes"]) == \
            (want["target_nmr_db"], want["met"], want["total_bytes"]), limit
        model = pm.solve(prof, limit, t_lo, t_hi)
        assert (got["target_nmr_db"] * GRID, got["met"], got["total_bytes"]) == (model["t"], bool(model["met"]),
                                                                                 model["total"]), limit
        unmet += not got["met"]
    assert unmet >= 2                                       # the unreachable ones were among them


def _path(prof, limit, t_lo, t_hi):
    """the (t, total) a bisection for `limit` visits"""
    out, lo, hi = [(t_hi, int(prof[-1]))], t_lo - 1, t_hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        out.append((mid, int(prof[mid - t_lo])))
        lo, hi = (lo, mid) if prof[mid - t_lo] <= limit else (mid, hi)
    return out


def test_profile_solve_is_band_solve_excerpt(A):
    import torch
    g = gpu_curve(A)
    check_solve(g["enc"], g["curve"], torch.as_tensor(g["profile"], device=g["enc"].device), g["profile"], -30, 30)


@pytest.mark.parametrize("lo,hi", [(-2, 2), (0.25, 0.25), (0.25, 0.25 + 1 / 64)])
def test_profile_solve_is_band_solve_synthetic(A, lo, hi):
    enc = solver(A)
    dev = on_device(enc, synthetic(300, 7, 0.5))
    prof_dev = enc.band_profile(dev, lo, hi)
    check_solve(enc, dev, prof_dev, prof_dev.cpu().numpy(), lo, hi)


# ------------------------------------------------------------------------------------------------ 3. end to end
@functools.lru_cache(maxsize=None)
def one_batch(A_id, which, **size):
    import audio_codec_amd as A
    if which == "castanet":
        pcm, sr = castanet()
        return A.pacfile.encode_stream_abr(pcm, sr, block_switching=True, allocation="band", **size)
    pcm, sr = excerpt("harpsichord", 0, 7)
    return A.pacfile.encode_stream_abr(pcm, sr, block_switching=False, allocation="band", **size)


@pytest.mark.parametrize("chunk_hops", [1, 5, 12, 20])
def test_chunked_equals_one_batch_block_switched(A, chunk_hops):
    pcm, sr = castanet()
    assert len(pcm) == 12 * 1024
    want = one_batch(0, "castanet", kbps_per_channel=96)
    got = A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=chunk_hops, block_switching=True)
    assert got == want
    max_bytes = len(want) - 1500
    want = one_batch(0, "castanet", max_bytes=max_bytes)
    assert len(want) <= max_bytes
    got = A.pacfile.encode_stream_abr_chunked(pcm, sr, max_bytes=max_bytes, chunk_hops=chunk_hops, block_switching=True)
    assert got == want


@pytest.mark.parametrize("chunk_hops", [1, 3, 7, 4096])
def test_chunked_equals_one_batch_long_only(A, chunk_hops):
    pcm, sr = excerpt("harpsichord", 0, 7)
    want = one_batch(0, "harpsichord", kbps_per_channel=96)
    assert A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=chunk_hops) == want


def test_chunked_pieces_memmap_and_plot(A, tmp_path):
    """the generator form gives the header, then one body per chunk and one for the driver's last two blocks; an
    np.memmap is as good as an array; quality.stream_rate_profile is the first pass"""
    pcm, sr = castanet()
    path = tmp_path / "pcm.i16"
    pcm.tofile(path)
    mm = np.memmap(path, dtype=np.int16, mode="r", shape=pcm.shape)
    parts = list(A.pacfile.iter_encode_abr_chunked(mm, sr, kbps_per_channel=96, chunk_hops=5, block_switching=True))
    assert len(parts) == 1 + 3 + 1 and all(isinstance(p, bytes) for p in parts)
    cp = A.pacfile._rate_coding_params(pcm, sr, 320, None)
    assert parts[0] == A.pacfile.header_bytes(cp)
    assert b"".join(parts) == one_batch(0, "castanet", kbps_per_channel=96)
    targets, total = A.quality.stream_rate_profile(mm, sr, chunk_hops=5, block_switching=True)
    assert targets[0] == -30 and targets[-1] == 30 and np.array_equal(np.diff(targets), np.full(3840, 1 / 64))
    assert total.dtype == np.int64 and np.array_equal(total, gpu_curve(A)["profile"])


def test_unreachable_size_raises_the_one_batch_message(A):
    pcm, sr = castanet()
    head = len(A.pacfile.header_bytes(A.pacfile._rate_coding_params(pcm, sr, 320, None)))
    for size in (dict(max_bytes=head + 100), dict(max_bytes=head), dict(kbps_per_channel=0.5)):
        with pytest.raises(ValueError) as one:
            A.pacfile.encode_stream_abr(pcm, sr, block_switching=True, allocation="band", **size)
        assert "cannot be reached" in str(one.value) and "smallest size" in str(one.value)
        with pytest.raises(ValueError) as chunked:
            A.pacfile.encode_stream_abr_chunked(pcm, sr, chunk_hops=5, block_switching=True, **size)
        assert str(chunked.value) == str(one.value)
    # a narrow range that cannot reach the size either: the total named is the profile's last entry
    with pytest.raises(ValueError) as one:
        A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=8, block_switching=True, allocation="band",
                                    nmr_range_db=(-12, -6))
    with pytest.raises(ValueError) as chunked:
        A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=8, chunk_hops=5, block_switching=True,
                                            nmr_range_db=(-12, -6))
    assert str(chunked.value) == str(one.value)
    at_top = int(gpu_curve(A)["profile"][(-6 + 30) * GRID])
    assert f"it takes {at_top} bytes" in str(one.value)


def test_gain_shape_chunked_equals_one_batch(A):
    pcm, sr = vm.fixture_stream()                           # 4 hops, 6 blocks, 12 channel-frames
    want = A.pacfile.encode_stream_vq_abr(pcm, sr, kbps_per_channel=96, max_kbps_per_channel=vm.CAP_KBPS,
                                          block_switching=True)
    got = A.pacfile.encode_stream_abr_chunked(pcm, sr, kbps_per_channel=96, chunk_hops=2,
                                              max_kbps_per_channel=vm.CAP_KBPS, block_switching=True, use_vq=True)
    assert got == want


# ------------------------------------------------------------------------------------------------ 4. nothing existing moves
def test_other_handles_are_refused(A):
    import torch
    pcm, sr = vm.fixture_stream()
    _, vq, _, _ = A.pacfile._rate_stream_setup(pcm, sr, vm.CAP_KBPS, True, None, use_vq=True)
    sbr = A.context.encoder(44100, 96 / 44.1, use_vq=True, use_sbr=True)
    for enc in (vq, sbr):
        dev = on_device(enc, synthetic(3, 43))
        with pytest.raises(NotImplementedError):
            enc.band_profile(dev, -2, 2)
        with pytest.raises(NotImplementedError):
            enc.profile_solve(torch.zeros(257, dtype=torch.int64, device=enc.device), 10, -2, 2)


def test_encode_pack_and_band_solve_unchanged_by_a_profile(A):
    g = gpu_curve(A)
    pcm, sr = castanet()
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    assert enc is g["enc"]
    limit = int(g["profile"][1700])

    def snapshot():
        out = enc.encode_pack(view, flags)
        sol = enc.band_solve(g["curve"], limit)
        return ([out[k].cpu().numpy().copy() for k in ("n_bytes", "bit_alloc", "overall", "status")] +
                [out["payload"].cpu().numpy()[:, :64].copy()] +
                [sol[k].cpu().numpy().copy() for k in ("bit_alloc", "n_bytes", "capped")] +
                [np.array([sol["target_nmr_db"], sol["met"], sol["total_bytes"]])])
    before = snapshot()
    enc.band_profile(g["curve"])
    enc.profile_solve(enc.band_profile(g["curve"], -64, 64), limit, -64, 64)
    after = snapshot()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_host_stream_encoder_still_equals_one_batch(A):
    """streaming.HostStreamEncoder after its front end moved into _chunk_front (the full matrix: test_gpu_round3.py)"""
    pcm, sr = castanet()
    want = A.pacfile.encode_stream(pcm, sr, 128, block_switching=True)
    assert A.pacfile.encode_stream(pcm, sr, 128, block_switching=True, chunk_hops=5) == want
