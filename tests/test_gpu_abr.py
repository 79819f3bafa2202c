"""Coding to an average bit rate on the GPU (pacx_rate_curve_batch / pacx_rate_solve, Encoder.rate_curve / rate_solve,
pacfile.encode_stream_abr, quality.encode_stream_to_rate) against the NumPy statement of tests/abr_model.py.

Bars.
  Curve.  bits and steps equal the model's; worst within 1e-5 dB of it, the bar tests/test_gpu_nmr.py holds for the
  same quantity (band NMRs of the GPU against nmr_model.band_values), and finite for every live unit; entries of a
  row that no unit uses keep the sentinel they were given.
  Solve.  On the GPU's own curve (or a synthetic one) t, met, total, every budget, every n_bytes and the capped
  mask equal the model's: both sides read the same numbers, so there is no tie window.
  Closed loop.  The stream of encode_stream_abr is as long as predicted, record by record, fits the limit, is
  encode_stream_nmr's at the target found byte for byte (the search and the curve share one evaluation function) and
  rate_model.encode's with the budgets returned.
"""
import ctypes
import functools

import numpy as np
import pytest

import abr_model as am
import nmr_model as nm
import rate_model as rm
import soak_programmes as sp
from conftest import EXCERPTS, load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

WORST_TOL = 1e-5            # dB
SENTINEL_W, SENTINEL_B = -12345.0, -77


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


# ------------------------------------------------------------------------------------------------------ material
# the constructions of tests/test_gpu_rate.py's SHAPES
def excerpt(name, h0, h1):
    ex = load_excerpt(name)
    return np.ascontiguousarray(ex["pcm"][h0 * 1024:h1 * 1024]), int(ex["sr"])


def three_channels():
    a, sr = excerpt("castanet", 24, 29)
    b, _ = excerpt("spmg", 0, 5)
    return np.ascontiguousarray(np.concatenate((a, b[:, :1]), axis=1)), sr


def windows():
    """sustained material with a click in hops 2 and 4: blocks with start, stop and start-stop windows around two
    short-coded ones"""
    pcm, sr = excerpt("harpsichord", 0, 7)
    pcm = pcm.copy()
    for h in (2, 4):
        pcm[h * 1024 + 600:h * 1024 + 606] = 30000
    return pcm, sr


def silence_and_drop():
    """digital silence, a short-coded hop the reference drops (zeros before a burst), ordinary hops"""
    rng = np.random.default_rng(5)
    pcm = np.zeros((6 * 1024, 2), np.int16)
    pcm[1024:2048] = rng.integers(-3000, 3000, (1024, 2))
    pcm[3 * 1024 + 900:4 * 1024] = rng.integers(-30000, 30000, (124, 2))
    pcm[4 * 1024:] = rng.integers(-3000, 3000, (2 * 1024, 2))
    return pcm, 48000


# name -> (material, block switching, cap kb/s).  The cap sets J and with it the model's work (J + 1 evaluations per
# unit on the CPU): 320 kb/s is one case of its own on a mono cut, the others take the cap at which the prototype ran
SHAPES = {
    "mono_odd": (lambda: (excerpt("castanet", 24, 29)[0][:, :1].copy(), 44100), True, 160),
    "three_channels_odd": (three_channels, True, 128),
    "stereo_long_only": (lambda: excerpt("harpsichord", 0, 5), False, 160),               # frame_flags = NULL
    "one_hop": (lambda: excerpt("castanet", 26, 27), True, 160),
    "windows": (windows, True, 128),
    "silence_and_drop": (silence_and_drop, True, 160),
    "rate_32k": (lambda: (sp.programme(30_011, 5, 2, 32000), 32000), True, 128),
    "rate_96k": (lambda: (sp.programme(30_012, 5, 3, 96000), 96000), True, 160),
    "cap_48": (lambda: excerpt("spmg", 0, 8), True, 48),
    "cap_320": (lambda: (excerpt("castanet", 24, 29)[0][:, 1:].copy(), 44100), True, 320),
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    make, bs, cap = SHAPES[name]
    pcm, sr = make()
    a = rm.analysis(pcm, sr, bs)
    return pcm, sr, bs, cap, a, am.curve(a, cap)


@functools.lru_cache(maxsize=None)
def excerpt_case(name):
    pcm, sr = excerpt(name, 0, 24)
    return pcm, sr, rm.analysis(pcm, sr, True)


def gpu_curve(A, pcm, sr, bs, cap, sentinel=True, view_of=None):
    """Encoder.rate_curve on the stream's blocks, into arrays that hold a sentinel -> (dict of NumPy arrays, encoder
    state for further calls).  view_of(enc, pcm): another view of the same blocks (tests/test_gpu_pcm_views.py)"""
    import torch
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, cap, bs, None)
    if view_of is not None:
        view = view_of(enc, pcm)
    row, sub = enc.rate_curve_layout(cp.targetBitsPerSample)
    out = None
    if sentinel:
        out = {"worst": torch.full((view.n_cf, row), SENTINEL_W, dtype=torch.float64, device=enc.device),
               "bits": torch.full((view.n_cf, row), SENTINEL_B, dtype=torch.int32, device=enc.device),
               "steps": torch.full((view.n_cf, 8), -99, dtype=torch.int32, device=enc.device)}
    c = enc.rate_curve(view, flags, cp.targetBitsPerSample, out=out)
    host = {k: c[k].cpu().numpy() for k in ("worst", "bits", "steps")}
    host["row"], host["sub_stride"] = c["row"], c["sub_stride"]
    return host, c, enc, view, flags


def used_mask(c):
    """entries of the rows that a unit uses"""
    used = np.zeros(c["worst"].shape, bool)
    for cf, sb in zip(*np.nonzero(c["steps"] >= 0)):
        at = sb * c["sub_stride"]
        used[cf, at:at + c["steps"][cf, sb] + 1] = True
    return used


def check_solve(A, enc, dev_curve, host_curve, limit, lo_db, hi_db, what):
    """Encoder.rate_solve against abr_model.solve on the same arrays: everything equal"""
    sol = enc.rate_solve(dev_curve, None, limit, lo_db, hi_db)
    ref = am.solve(host_curve, limit, int(lo_db * 64), int(hi_db * 64))
    got = (int(round(sol["target_nmr_db"] * 64)), int(sol["met"]), sol["total_bytes"])
    print(f"{what}: limit {limit}: t {got[0]} ({got[0] / 64:+.3f} dB), met {got[1]}, total {got[2]}; model "
          f"{ref['t']}, {ref['met']}, {ref['total']}; {len(ref['path'])} probes")
    assert got == (ref["t"], ref["met"], ref["total"]), what
    assert sol["target_nmr_db"] * 64 == got[0], what
    assert np.array_equal(sol["budget"].cpu().numpy(), ref["budget"]), what
    assert np.array_equal(sol["n_bytes"].cpu().numpy(), ref["n_bytes"]), what
    assert np.array_equal(sol["capped"].cpu().numpy(), ref["capped"]), what
    return sol, ref


def compare_curve(name, a, cap, model, host, flags):
    """the curve of the GPU (host arrays made with the sentinels) against the model's, with this file's bars"""
    assert (host["row"], host["sub_stride"]) == (model["row"], model["sub_stride"]) == am.layout(a, cap)
    if flags is not None:
        want = np.array([l * 1 + c * 2 + n * 4 for (l, c, n) in a["flags"]], np.uint8)
        assert np.array_equal(flags.cpu().numpy(), want)                    # the GPU's detector gave the model's flags
    else:
        assert not any(f[1] for f in a["flags"])
    assert np.array_equal(host["steps"], model["steps"])
    used = used_mask(model)
    live = int((model["steps"] >= 0).sum())
    assert used.sum() == model["evals"]
    assert np.array_equal(host["bits"][used], model["bits"][used])
    assert np.isfinite(host["worst"][used]).all() and np.isfinite(model["worst"][used]).all()
    err = np.abs(host["worst"][used] - model["worst"][used]).max() if used.any() else 0.0
    print(f"{name}: {live} units, {model['evals']} evaluations, row {host['row']}, sub_stride {host['sub_stride']}, "
          f"max |worst - model| {err:.3g} dB")
    assert err <= WORST_TOL
    assert (host["worst"][~used] == SENTINEL_W).all() and (host["bits"][~used] == SENTINEL_B).all()


# ------------------------------------------------------------------ 1. the curve, 2. the solve on it
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_curve_and_solve_on_shapes(A, name):
    """1, 2 and 3 channels (odd numbers of channel-frames), one hop, no flags, every window kind (start / stop flags
    change J), digital silence and a dropped hop, the 32 and 96 kHz band layouts (the dummy band), a cap at which
    short sub-blocks have a tiny J, the default cap"""
    pcm, sr, bs, cap, a, model = shape_case(name)
    host, dev, enc, view, flags = gpu_curve(A, pcm, sr, bs, cap)
    compare_curve(name, a, cap, model, host, flags)
    kinds = {(bool(l), bool(c), bool(n)) for (l, c, n) in a["flags"]}
    if name == "windows":
        assert {(False, False, True), (True, False, False), (True, False, True), (False, True, False)} <= kinds
        assert len({int(j) for j in model["steps"][:, 0][~np.array([bool(f[1]) for f in a["flags"]]).repeat(a["n_ch"])]}) == 2
    if name == "stereo_long_only":
        assert flags is None and (model["steps"][:, 1:] == -1).all()
    if name == "silence_and_drop":
        assert any(a["dropped"]) and (model["steps"] == -1).all(axis=1).any()
    if name == "cap_48":
        assert model["steps"][model["steps"] >= 0].min() <= 3                # short sub-blocks: J small or 0
    if name in ("rate_32k", "rate_96k"):
        assert any(f[1] for f in a["flags"])                                 # short band layout in use
    # the solve on the GPU's own curve, three limits between the totals of the two ends of the range
    small, big = am.total(host, 30 * 64), am.total(host, -30 * 64)
    for share in (0.2, 0.5, 0.9):
        check_solve(A, enc, dev, host, int(small + share * (big - small)), -30, 30, name)


def test_curve_without_sentinel_and_bad_rows(A):
    """rate_curve's own arrays: NaN / 0 / -1 where nothing is written; a row below the layout's is refused"""
    import torch
    pcm, sr, bs, cap, a, model = shape_case("one_hop")
    host, dev, enc, view, flags = gpu_curve(A, pcm, sr, bs, cap, sentinel=False)
    used = used_mask(model)
    assert np.isnan(host["worst"][~used]).all() and np.array_equal(host["steps"], model["steps"])
    row = host["row"]
    small = {"worst": torch.zeros((view.n_cf, row - 1), dtype=torch.float64, device=enc.device),
             "bits": torch.zeros((view.n_cf, row - 1), dtype=torch.int32, device=enc.device),
             "steps": torch.zeros((view.n_cf, 8), dtype=torch.int32, device=enc.device)}
    with pytest.raises(ValueError):
        enc.rate_curve(view, flags, cap / (sr / 1000), out=small)
    rc = enc.lib.pacx_rate_curve_batch(enc.h, ctypes.byref(view.c), None, cap / (sr / 1000), row - 1,
                                       A.engine._ptr(small["worst"]), A.engine._ptr(small["bits"]),
                                       A.engine._ptr(small["steps"]), None)
    assert rc == A._lib.E_ARG


# ------------------------------------------------------------------ 2b. the solve on curves no encoder made
@functools.lru_cache(maxsize=None)
def synthetic_case():
    return am.synthetic(3000, 232, 36, seed=3)


def on_device(A, c):
    import torch
    enc = A.engine.Encoder(48000, 128 / 48.0)
    dev = {k: torch.as_tensor(c[k], device=enc.device) for k in ("worst", "bits", "steps")}
    dev["row"], dev["sub_stride"] = c["row"], c["sub_stride"]
    return enc, dev


def test_solve_on_synthetic_curves(A):
    """3000 channel-frames (12 workgroups of the pick), long / short / dropped mixed, non-monotone worst, and the
    edges: unreachable, everything fits at t_lo, limit == total(t) exactly, a single grid point, other ranges"""
    c = synthetic_case()
    assert (c["steps"][:, 1] >= 0).any() and (c["steps"] < 0).all(axis=1).any()
    enc, dev = on_device(A, c)
    small, big = am.total(c, 30 * 64), am.total(c, -30 * 64)
    for share in (0.03, 0.25, 0.5, 0.75, 0.99):
        check_solve(A, enc, dev, c, int(small + share * (big - small)), -30, 30, f"synthetic {share}")
    sol, ref = check_solve(A, enc, dev, c, small - 1, -30, 30, "unreachable")
    assert not sol["met"] and sol["target_nmr_db"] == 30.0 and sol["total_bytes"] == small
    sol, ref = check_solve(A, enc, dev, c, small, -30, 30, "limit == total(t_hi)")
    assert sol["met"] and sol["total_bytes"] <= small
    sol, ref = check_solve(A, enc, dev, c, 10 * big, -30, 30, "everything fits")
    assert sol["met"] and sol["target_nmr_db"] == -30.0 and sol["total_bytes"] == big
    mid = am.solve(c, (small + big) // 2)
    sol, ref = check_solve(A, enc, dev, c, mid["total"], -30, 30, "limit == total(t)")
    assert sol["total_bytes"] <= mid["total"]
    check_solve(A, enc, dev, c, mid["total"] - 1, -30, 30, "limit == total(t) - 1")
    check_solve(A, enc, dev, c, 0, -30, 30, "limit 0")
    check_solve(A, enc, dev, c, (small + big) // 2, 0.078125, 0.078125, "one grid point")
    check_solve(A, enc, dev, c, (small + big) // 2, -3.015625, 12.5, "odd range")
    check_solve(A, enc, dev, c, (small + big) // 2, -100, 200, "wide range")
    check_solve(A, enc, dev, c, (small + big) // 2, -0.015625, 0, "two grid points")
    enc.close()


def test_solve_sums_do_not_depend_on_the_launch(A):
    """the same solve twice, and on a curve cut to 257 channel-frames (one thread into a second workgroup)"""
    c = synthetic_case()
    enc, dev = on_device(A, c)
    limit = (am.total(c, 30 * 64) + am.total(c, -30 * 64)) // 2
    one = enc.rate_solve(dev, None, limit)
    two = enc.rate_solve(dev, None, limit)
    for k in ("budget", "n_bytes", "capped"):
        assert np.array_equal(one[k].cpu().numpy(), two[k].cpu().numpy())
    assert (one["target_nmr_db"], one["total_bytes"]) == (two["target_nmr_db"], two["total_bytes"])
    cut = {k: np.ascontiguousarray(c[k][:257]) for k in ("worst", "bits", "steps")}
    cut["row"], cut["sub_stride"] = c["row"], c["sub_stride"]
    enc2, dev2 = on_device(A, cut)
    check_solve(A, enc2, dev2, cut, (am.total(cut, 30 * 64) + am.total(cut, -30 * 64)) // 2, -30, 30, "257 cf")
    enc.close()
    enc2.close()


# ------------------------------------------------------------------ 3. closed loop
@pytest.mark.parametrize("kbps", [96, 128])
@pytest.mark.parametrize("name", EXCERPTS)
def test_closed_loop(A, name, kbps):
    pcm, sr, a = excerpt_case(name)
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    data, rep, info = A.quality.encode_stream_to_rate(pcm, sr, kbps_per_channel=kbps, block_switching=True)
    assert data == A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=kbps, block_switching=True)
    limit = int(np.floor(kbps * 1000 * n_ch * blocks * 1024 / sr / 8))
    assert info["limit_bytes"] == limit
    recs, _ = nm.records(data)
    head = recs[0][0] - 4                                # the header ends where the first length prefix begins
    body = len(data) - head
    print(f"{name} {kbps} kb/s: target {info['target_nmr_db']:+.3f} dB, body {body} of {limit} bytes "
          f"(fill {body / limit:.4f}), {info['kbps_per_channel']:.2f} kb/s per channel")
    assert body == info["total_bytes"] <= limit
    assert body == sum(n + 4 for _, n in recs)
    # the record lengths are the predicted ones
    want = info["n_bytes"][info["n_bytes"] > 0]
    assert np.array_equal(np.array([n for _, n in recs]), want)
    assert np.array_equal(info["written"], ~np.array(a["dropped"]))
    assert np.array_equal(rep.short, np.array([bool(f[1]) for f in a["flags"]]))
    # the stream of the constant-quality search at the target found: one evaluation function serves both
    T = info["target_nmr_db"]
    assert T * 64 == np.floor(T * 64)
    assert data == A.pacfile.encode_stream_nmr(pcm, sr, T, max_kbps_per_channel=320, block_switching=True)
    # and the model encoder's with the budgets returned
    assert data == rm.encode(a, info["budget"], len(pcm))
    assert abs(info["kbps_per_channel"] - rm.kbps_per_channel(a, data)) < 1e-9
    assert info["kbps_per_channel"] <= kbps
    assert np.array_equal(A.pacfile.decode_stream(data), po.decode_stream(data))          # int16 for int16
    # max_bytes counts the header too: the same stream from the same limit given that way
    assert data == A.pacfile.encode_stream_abr(pcm, sr, max_bytes=limit + head, block_switching=True)


def test_two_sizes_from_one_curve(A):
    pcm, sr, a = excerpt_case("spmg")
    both = A.quality.encode_stream_to_rate(pcm, sr, kbps_per_channel=[96, 128], block_switching=True)
    assert len(both) == 2
    for (data, rep, info), kbps in zip(both, (96, 128)):
        assert data == A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=kbps, block_switching=True)
    assert both[0][2]["target_nmr_db"] > both[1][2]["target_nmr_db"] and len(both[0][0]) < len(both[1][0])
    c = A.quality.rate_curve(pcm, sr, block_switching=True)
    assert c["worst"].shape == (26, 2, c["row"]) and c["steps"].shape == (26, 2, 8)
    assert np.array_equal(c["steps"][..., 0] >= 0, np.repeat(~np.array(a["dropped"])[:, None], 2, axis=1))


# ------------------------------------------------------------------ 4. arguments
def test_unsupported_and_bad_arguments(A):
    import torch
    pcm, sr = excerpt("castanet", 24, 26)
    abr = A.pacfile.encode_stream_abr
    for kw in ({}, {"kbps_per_channel": 96, "max_bytes": 10_000}):
        with pytest.raises(ValueError):
            abr(pcm, sr, **kw)
    for rng in ((3, -3), (float("nan"), 3), (-30, float("inf")), (-30.01, 30), (0,), "ab"):
        with pytest.raises(ValueError):
            abr(pcm, sr, kbps_per_channel=96, nmr_range_db=rng)
    for kw in ({"n_lines": 512}, {"chunk_hops": 4}, {"use_vq": True}, {"use_sbr": True}):
        with pytest.raises(NotImplementedError):
            abr(pcm, sr, kbps_per_channel=96, **kw)
    with pytest.raises(ValueError):                              # 320 kb/s at 16 kHz: 20 bits per sample
        abr(pcm, 16000, kbps_per_channel=96)
    with pytest.raises(ValueError, match="smallest size"):       # unreachable
        abr(pcm, sr, kbps_per_channel=0.5)
    with pytest.raises(ValueError, match="smallest size"):
        abr(pcm, sr, max_bytes=200)
    with pytest.raises(ValueError):                              # smaller than the header
        abr(pcm, sr, max_bytes=10)
    assert abr(pcm, sr, max_bytes=10 ** 9, nmr_range_db=(-6, 6)) == A.pacfile.encode_stream_nmr(pcm, sr, -6.0)
    for kw in ({"use_vq": True}, {"use_vq": True, "use_sbr": True}, {"use_sbr": True}):
        enc = A.engine.Encoder(sr, 128 / (sr / 1000), **kw)
        view = A.engine.PcmView.stream(A.pacfile.device_stream(enc, pcm), 1024)
        with pytest.raises(NotImplementedError):
            enc.rate_curve(view, None, 7.0)
        row, sub = ctypes.c_int32(), ctypes.c_int32()
        assert enc.lib.pacx_rate_curve_layout(enc.h, 7.0, ctypes.byref(row), ctypes.byref(sub)) == A._lib.E_UNSUPPORTED
        assert enc.lib.pacx_rate_curve_batch(enc.h, ctypes.byref(view.c), None, 7.0, 4096, None, None, None,
                                             None) == A._lib.E_UNSUPPORTED
        assert enc.lib.pacx_rate_solve(enc.h, 1, 64, 8, None, None, None, 100, -30.0, 30.0, None, None, None, None,
                                       None) == A._lib.E_UNSUPPORTED
        enc.close()
    enc = A.engine.Encoder(sr, 128 / (sr / 1000))
    view = A.engine.PcmView.stream(A.pacfile.device_stream(enc, pcm), 1024)
    for cap in (0.0, -1.0, float("nan"), 16.5):
        with pytest.raises(A._lib.PacxError):
            enc.rate_curve(view, None, cap)
    c = enc.rate_curve(view, None, 7.0)
    ptr = A.engine._ptr
    for missing in range(3):                                     # every output of the curve in turn
        args = [ptr(c["worst"]), ptr(c["bits"]), ptr(c["steps"])]
        args[missing] = None
        assert enc.lib.pacx_rate_curve_batch(enc.h, ctypes.byref(view.c), None, 7.0, c["row"], *args,
                                             None) == A._lib.E_ARG, missing
    for lo, hi in ((float("nan"), 3.0), (-3.0, float("inf")), (3.0, -3.0), (-30.01, 30.0), (-30.0, 0.001), (-2e6, 0.0)):
        with pytest.raises(A._lib.PacxError):
            enc.rate_solve(c, None, 1000, lo, hi)
    with pytest.raises(A._lib.PacxError):
        enc.rate_solve(c, None, -1)
    bud = torch.zeros((view.n_cf, 8), dtype=torch.int32, device=enc.device)
    nby = torch.zeros((view.n_cf,), dtype=torch.int32, device=enc.device)
    cpd = torch.zeros((view.n_cf,), dtype=torch.uint8, device=enc.device)
    res = torch.zeros((4,), dtype=torch.int32, device=enc.device)
    good = [ptr(c["worst"]), ptr(c["bits"]), ptr(c["steps"]), 1000, -30.0, 30.0, ptr(bud), ptr(nby), ptr(cpd), ptr(res)]
    assert enc.lib.pacx_rate_solve(enc.h, view.n_cf, c["row"], c["sub_stride"], *good, None) == 0
    for missing in (0, 1, 2, 6, 7, 8, 9):                        # every pointer in turn
        args = list(good)
        args[missing] = None
        rc = enc.lib.pacx_rate_solve(enc.h, view.n_cf, c["row"], c["sub_stride"], *args, None)
        assert rc == A._lib.E_ARG, missing
    # a row that cannot hold eight sub-blocks
    assert enc.lib.pacx_rate_solve(enc.h, view.n_cf, 7 * c["sub_stride"], c["sub_stride"], *good, None) == A._lib.E_ARG
    assert enc.lib.pacx_rate_solve(enc.h, view.n_cf, c["row"], 0, *good, None) == A._lib.E_ARG
    torch.cuda.synchronize()
    enc.close()


@pytest.mark.parametrize("bs", [False, True])
def test_constant_rate_bytes_do_not_move(A, bs):
    """the new path shares the handle's workspace (and grows it) and leaves no state behind"""
    ex = load_excerpt("castanet")
    pcm, sr = np.ascontiguousarray(ex["pcm"][:48 * 1024]), int(ex["sr"])
    before = A.pacfile.encode_stream(pcm, sr, 128, block_switching=bs)
    # max_kbps_per_channel = 128: the handle of the call above
    abr = A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=96, max_kbps_per_channel=128, block_switching=bs)
    assert abr != before
    assert A.pacfile.encode_stream(pcm, sr, 128, block_switching=bs) == before
    assert A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=96, max_kbps_per_channel=128, block_switching=bs) == abr
