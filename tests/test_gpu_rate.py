"""Coding to a target noise-to-mask ratio on the GPU (pacx_encode_pack_nmr_batch / pacx_encode_pack_budget_batch,
pacfile.encode_stream_nmr, quality.encode_stream_to_nmr) against the NumPy statement of tests/rate_model.py.

Bars.
  Bytes.  With the budgets given -- the GPU's own or any others -- the stream is the model encoder's, byte for byte.
  Budgets.  Equal to the model's search for every unit (a long block or a short sub-block) whose model margin -- the
  smallest |max_b NMR_b - target| over the evaluations the bisection made -- is at least WINDOW = 1e-4 dB: ten times
  the 1e-5 dB to which GPU and model NMRs are held to agree (tests/test_gpu_nmr.py).  A unit inside the window may
  take the other branch and is left out; at most 1 % of a case's units may be, and the inputs are chosen so that the
  model alone leaves out none.  Smallest model margins, measured on the CPU with the model:
    first 24 hops of castanet / harpsichord / quar48_1 / spmg, block switching on, cap 320 kb/s, targets 0 and -6 dB:
    880 units (248 / 136 / 234 / 262), smallest margin 2.0e-3 dB (quar48_1 at 0 dB);
    the cases of SHAPES below: the figure is printed by the test and recorded beside each case.
  Closed loop.  quality.nmr_of_file of the finished bytes -- the decoders and k_nmr, code the search does not share --
  gives every live band of every uncapped unit at most target + 1e-4 dB.
"""
import ctypes
import functools

import numpy as np
import pytest

import nmr_model as nm
import rate_model as rm
import soak_programmes as sp
from conftest import EXCERPTS, load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

WINDOW = 1e-4               # dB
LEFT_OUT = 0.01             # share of a case's units


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


# ------------------------------------------------------------------------------------------------------ material
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


# name -> (material, block switching, target dB, cap kb/s).  In the comment: units, smallest model margin (dB)
SHAPES = {
    "mono_odd": (lambda: (excerpt("castanet", 24, 29)[0][:, :1].copy(), 44100), True, -3.0, 320),
    "three_channels_odd": (three_channels, True, -3.0, 320),
    "stereo_long_only": (lambda: excerpt("harpsichord", 0, 5), False, -6.0, 320),         # frame_flags = NULL
    "one_hop": (lambda: excerpt("castanet", 26, 27), True, 0.0, 320),
    "windows": (windows, True, -3.0, 320),
    "attack": (lambda: excerpt("castanet", 24, 48), True, -6.0, 320),
    "silent_opening": (lambda: excerpt("castanet", 0, 3), True, 0.0, 320),
    "silence_and_drop": (silence_and_drop, True, -3.0, 320),
    "rate_32k": (lambda: (sp.programme(30_011, 5, 2, 32000), 32000), True, -3.0, 320),
    "rate_96k": (lambda: (sp.programme(30_012, 5, 3, 96000), 96000), True, -3.0, 320),
    "cap_48": (lambda: excerpt("spmg", 0, 8), True, -6.0, 48),
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    make, bs, target, cap = SHAPES[name]
    pcm, sr = make()
    return pcm, sr, bs, target, cap, rm.analysis(pcm, sr, bs)


@functools.lru_cache(maxsize=None)
def analysis_of(name, bs):
    """the model's analysis of a SHAPES material with the other block-switching setting"""
    pcm, sr = shape_case(name)[:2]
    return rm.analysis(pcm, sr, bs)


@functools.lru_cache(maxsize=None)
def excerpt_case(name):
    pcm, sr = excerpt(name, 0, 24)
    return pcm, sr, rm.analysis(pcm, sr, True)


# ------------------------------------------------------------------------------------------------------- helpers
def gpu_stream(A, pcm, sr, target, cap, bs):
    data, rep, info = A.quality.encode_stream_to_nmr(pcm, sr, target, max_kbps_per_channel=cap, block_switching=bs)
    assert data == A.pacfile.encode_stream_nmr(pcm, sr, target, max_kbps_per_channel=cap, block_switching=bs)
    return data, rep, info


def budget_stream(A, pcm, sr, budget, bs, kbps=128):
    """Encoder.encode_pack_budget through the whole stream -> .pac bytes, and the outputs"""
    import torch
    from audio_codec_amd.audiofile import CodingParams
    cp = CodingParams()
    cp.sampleRate, cp.nChannels, cp.numSamples = sr, pcm.shape[1], len(pcm)
    cp.nMDCTLines = cp.nSamplesPerBlock = 1024
    cp.nScaleBits, cp.nMantSizeBits = 4, 12
    cp.targetBitsPerSample = kbps / (sr / 1000)
    cp.useSBR = cp.useVQ = False
    enc = A.context.encoder_for_params(cp)
    planar = A.pacfile.device_stream(enc, pcm)
    view = A.engine.PcmView.stream(planar, 1024)
    flags = enc.transient_flags(planar, len(pcm) // 1024)[1] if bs else None
    out = enc.encode_pack_budget(view, flags, torch.as_tensor(np.ascontiguousarray(budget).reshape(-1, 8)))
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    return A.pacfile.header_bytes(cp) + body[:int(total.item())].cpu().numpy().tobytes(), out


def check_flags(a, rep):
    """the GPU's detector gave the model's flags (the model's analysis is of the same blocks)"""
    assert np.array_equal(rep.short, np.array([bool(f[1]) for f in a["flags"]]))
    assert np.array_equal(rep.record < 0, np.array(a["dropped"]))


def compare_budgets(a, info, target, cap, what):
    """budgets against the model's search outside the window; -> (model budgets, capped, live)"""
    budget, capped, margin, live = rm.search(a, target, cap)
    near = live & (margin < WINDOW)
    print(f"{what}: {int(live.sum())} units, {int(capped.sum())} capped, smallest model margin "
          f"{margin[live].min() if live.any() else float('nan'):.3g} dB, {int(near.sum())} inside the window")
    assert near.sum() <= LEFT_OUT * live.sum(), what
    cmp = live & ~near
    assert np.array_equal(info["budget"][cmp], budget[cmp]), what
    assert not info["budget"][~live].any(), what                      # dropped hops and unused slots: 0
    # the cap flag is kept per channel-block
    cmp_cf = ~near.any(axis=2)
    assert np.array_equal(info["capped"][cmp_cf], capped.any(axis=2)[cmp_cf]), what
    return budget, capped, live


# ------------------------------------------------------------------ 1. given budgets -> exact bytes
def test_own_budgets_give_the_model_encoders_bytes(A):
    pcm, sr, a = excerpt_case("spmg")
    data, rep, info = gpu_stream(A, pcm, sr, -6.0, 320, True)
    check_flags(a, rep)
    assert data == rm.encode(a, info["budget"], len(pcm))
    # the budget path writes the search's stream again from the search's budgets
    again, out = budget_stream(A, pcm, sr, info["budget"], True)
    assert again == data


@pytest.mark.parametrize("kind", ["random", "zero", "cbr_floor"])
def test_given_budgets_give_the_model_encoders_bytes(A, kind):
    pcm, sr, a = excerpt_case("quar48_1")
    shape = (len(a["flags"]), 2, 8)
    if kind == "random":
        budget = 32 * np.random.default_rng(7).integers(0, 233, shape).astype(np.int32)
    elif kind == "zero":
        budget = np.zeros(shape, np.int32)
    else:                                               # the 128 kb/s rule's value, rounded down to whole bits
        budget = np.zeros(shape, np.int32)
        p = po.make_params(sr, 2, 128)
        for f, (last_t, cur_t, next_t) in enumerate(a["flags"]):
            p.nMDCTLines = rm.SHORT if cur_t else rm.HOP
            budget[f] = int(np.floor(po.bit_budget(p, last_t, cur_t, next_t)))
    data, out = budget_stream(A, pcm, sr, budget, True)
    assert data == rm.encode(a, budget, len(pcm))
    assert not (out["status"].cpu().numpy() & A._lib.ST_RATE_CAP).any()


@pytest.mark.parametrize("name", ["stereo_long_only", "mono_odd", "three_channels_odd", "rate_96k"])
@pytest.mark.parametrize("bs", [False, True])
def test_given_budgets_on_odd_shapes(A, name, bs):
    """budgets that are not the search's, without flags (every frame long, one unit per channel-frame: 7, 14 or 21
    units, the odd counts leave half of the paired launch's last wave empty) and with them"""
    pcm, sr = shape_case(name)[:2]
    a = shape_case(name)[5] if bs == shape_case(name)[2] else analysis_of(name, bs)
    shape = (len(a["flags"]), pcm.shape[1], 8)
    budget = 32 * np.random.default_rng(11).integers(0, 200, shape).astype(np.int32)
    budget[0] = 0
    data, out = budget_stream(A, pcm, sr, budget, bs)
    assert out["budget"].shape[0] == shape[0] * shape[1]
    assert data == rm.encode(a, budget, len(pcm))


# ------------------------------------------------------------------ 2. budgets against the model's search
@pytest.mark.parametrize("target", [0.0, -6.0])
@pytest.mark.parametrize("name", EXCERPTS)
def test_budgets_equal_the_models_search(A, name, target):
    pcm, sr, a = excerpt_case(name)
    data, rep, info = gpu_stream(A, pcm, sr, target, 320, True)
    check_flags(a, rep)
    compare_budgets(a, info, target, 320, f"{name} {target:+.0f} dB")
    assert data == rm.encode(a, info["budget"], len(pcm))


# ------------------------------------------------------------------ 3. closed loop, 4. decodes, 5. shapes
def closed_loop(a, rep, info, target, cap, what):
    """nmr_of_file's values of every uncapped unit stay below target + WINDOW; a capped unit has the cap budget"""
    nbl, nbs = rep.n_bands_long, rep.n_bands_short
    n_capped = n_units = 0
    for f, row in enumerate(a["units"]):
        if row is None:
            assert np.isnan(rep.nmr_db[f]).all(), what
            continue
        for ch, us in enumerate(row):
            for j, u in enumerate(us):
                vals = rep.nmr_db[f, ch, j * nbs:(j + 1) * nbs] if u.short else rep.nmr_db[f, ch, :nbl]
                assert not np.isnan(vals).any(), what
                n_units += 1
                at_cap = info["budget"][f, ch, j] == rm.STEP * rm.cap_steps(a, u, cap)
                if vals.max() > target + WINDOW:
                    assert info["capped"][f, ch] and at_cap, (what, f, ch, j, float(vals.max()))
                    n_capped += 1
            if info["capped"][f, ch]:
                assert any(info["budget"][f, ch, j] == rm.STEP * rm.cap_steps(a, u, cap) for j, u in enumerate(us)), what
    return n_units, n_capped


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(A, name):
    """1, 2 and 3 channels (an odd number of channel-frames with 1 and 3: a stream of n channels holds n (hops + 2)),
    one hop, no flags, every window kind, the attack and the silent opening of castanet, digital silence and a
    dropped hop, the 32 and 96 kHz band layouts, a cap that most units reach.  Units / smallest model margin, dB:
      attack 276 / 1.4e-2   cap_48 104 / 3.8e-2 (93 capped)   mono_odd 28 / 1.6e-2   one_hop 20 / 1.7e-2
      rate_32k 52 / 1.6e-3   rate_96k 54 / 5.1e-3   silence_and_drop 14 / 9.3e-2   silent_opening 38 / 19.8
      stereo_long_only 14 / 1.1e-1   three_channels_odd 126 / 1.6e-2   windows 46 / 2.7e-2"""
    pcm, sr, bs, target, cap, a = shape_case(name)
    data, rep, info = gpu_stream(A, pcm, sr, target, cap, bs)
    check_flags(a, rep)
    budget, capped, live = compare_budgets(a, info, target, cap, name)
    assert data == rm.encode(a, info["budget"], len(pcm))                                  # exact, ties or not
    # the budget path (k_bitalloc_budget pairs two units per wave: odd unit counts without flags leave the last
    # wave half empty) writes the same stream from the same budgets
    assert budget_stream(A, pcm, sr, info["budget"], bs)[0] == data
    n_units, n_capped = closed_loop(a, rep, info, target, cap, name)
    assert n_units == live.sum()
    assert np.array_equal(A.pacfile.decode_stream(data), po.decode_stream(data))           # int16 for int16
    kinds = {(bool(l), bool(c), bool(n)) for (l, c, n) in a["flags"]}
    if name == "windows":
        assert {(False, False, True), (True, False, False), (True, False, True), (False, True, False)} <= kinds
    if name == "stereo_long_only":
        assert kinds == {(False, False, False)}
    if name == "silent_opening":
        assert not info["budget"].any() and not info["capped"].any()
    if name == "silence_and_drop":
        assert any(a["dropped"]) and (rep.record < 0).any()
    if name == "cap_48":
        assert capped[live].mean() > 0.5 and n_capped > 0
        assert (info["budget"][capped] == 0).any() or info["budget"][capped].min() <= 3 * rm.STEP      # J small or 0
    if name in ("rate_32k", "rate_96k"):
        assert any(a["flags"][f][1] for f in range(len(a["flags"])))                       # short band layout in use
    assert abs(info["kbps_per_channel"] - rm.kbps_per_channel(a, data)) < 1e-9


def test_closed_loop_on_an_excerpt(A):
    pcm, sr, a = excerpt_case("spmg")
    data, rep, info = gpu_stream(A, pcm, sr, -6.0, 320, True)
    n_units, n_capped = closed_loop(a, rep, info, -6.0, 320, "spmg -6 dB")
    assert n_units > 0 and n_capped == 0 and not info["capped"].any()
    assert np.nanmax(rep.nmr_db) <= -6.0 + WINDOW
    assert np.array_equal(A.pacfile.decode_stream(data), po.decode_stream(data))


# ------------------------------------------------------------------ 6. unsupported and bad arguments
def test_unsupported_and_bad_arguments(A):
    import torch
    pcm, sr = excerpt("castanet", 24, 26)
    budget = np.zeros((8, 8), np.int32)                     # 2 hops + 2 = 4 blocks of 2 channels
    for kw in ({"use_vq": True}, {"use_vq": True, "use_sbr": True}, {"use_sbr": True}):
        enc = A.engine.Encoder(sr, 128 / (sr / 1000), **kw)
        view = A.engine.PcmView.stream(A.pacfile.device_stream(enc, pcm), 1024)
        with pytest.raises(NotImplementedError):
            enc.encode_pack_nmr(view, None, -3.0, 7.0)
        with pytest.raises(NotImplementedError):
            enc.encode_pack_budget(view, None, budget)
        rc = enc.lib.pacx_encode_pack_nmr_batch(enc.h, ctypes.byref(view.c), None, -3.0, 7.0, *([None] * 9))
        assert rc == A._lib.E_UNSUPPORTED
        enc.close()
    enc = A.engine.Encoder(sr, 128 / (sr / 1000))
    view = A.engine.PcmView.stream(A.pacfile.device_stream(enc, pcm), 1024)
    for target, cap in ((float("nan"), 7.0), (float("inf"), 7.0), (-3.0, 0.0), (-3.0, -1.0), (-3.0, float("nan")),
                        (-3.0, 16.5)):
        with pytest.raises(A._lib.PacxError):
            enc.encode_pack_nmr(view, None, target, cap)
    out = enc.alloc_outputs(view.n_cf, with_payload=True)
    ptr = A.engine._ptr
    good = [ptr(out[k]) for k in ("overall", "scale_factor", "bit_alloc", "mantissa", "status", "payload", "n_bytes")]
    bud = torch.zeros((view.n_cf, 8), dtype=torch.int32, device=enc.device)
    for missing in (0, 1, 2, 4, 5, 6, 7):                         # every required output in turn (3: mantissa is optional)
        args = good + [ptr(bud)]
        args[missing] = None
        rc = enc.lib.pacx_encode_pack_nmr_batch(enc.h, ctypes.byref(view.c), None, -3.0, 7.0, *args, None)
        assert rc == A._lib.E_ARG, missing
    rc = enc.lib.pacx_encode_pack_budget_batch(enc.h, ctypes.byref(view.c), None, None, *good, None)
    assert rc == A._lib.E_ARG
    with pytest.raises(ValueError):
        enc.encode_pack_budget(view, None, np.zeros((3, 8), np.int32))
    enc.close()
    with pytest.raises(ValueError):                              # 320 kb/s at 16 kHz: 20 bits per sample
        A.pacfile.encode_stream_nmr(pcm, 16000, -3.0)
    for kw in ({"n_lines": 512}, {"chunk_hops": 4}, {"use_vq": True}, {"use_sbr": True}):
        with pytest.raises(NotImplementedError):
            A.pacfile.encode_stream_nmr(pcm, sr, -3.0, **kw)


# ------------------------------------------------------------------ 7. the constant-rate path is untouched
@pytest.mark.parametrize("bs", [False, True])
def test_constant_rate_bytes_do_not_move(A, bs):
    """the new path shares the handle's workspace (and grows it) and leaves no state behind"""
    ex = load_excerpt("castanet")
    pcm, sr = np.ascontiguousarray(ex["pcm"][:48 * 1024]), int(ex["sr"])
    before = A.pacfile.encode_stream(pcm, sr, 128, block_switching=bs)
    # max_kbps_per_channel = 128: the handle of the call above
    vbr = A.pacfile.encode_stream_nmr(pcm, sr, -3.0, max_kbps_per_channel=128, block_switching=bs)
    assert vbr != before
    assert A.pacfile.encode_stream(pcm, sr, 128, block_switching=bs) == before
    assert A.pacfile.encode_stream_nmr(pcm, sr, -3.0, max_kbps_per_channel=128, block_switching=bs) == vbr
