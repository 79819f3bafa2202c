"""Bits handed to the bands one by one on the GPU (pacx_band_curve_batch / pacx_band_pick / pacx_band_solve /
pacx_encode_pack_alloc_batch, Encoder.band_curve / band_pick / band_solve / encode_pack_alloc, the allocation="band"
keyword of pacfile and quality) against the NumPy statement of tests/band_model.py.

Bars.
  Curve.  Every finite nmr entry of every live unit within 1e-5 dB of the model (the agreement tests/test_gpu_nmr.py
  holds GPU and model NMRs to), +inf exactly where defined, cap equal, cap_alloc equal wherever the cf's status has no
  PACX_ST_GUARD.
  Pick.  Allocation, capped and n_bytes equal the model's pick for every unit whose margin -- the smallest
  |nmr - target| over its bands and candidates -- is at least WINDOW = 1e-4 dB; a unit inside the window is left out
  whole, at most 1 % of a case's units may be, and the inputs are such that the model alone leaves out none (smallest
  margin over the first six cases, measured on the CPU with the model: 4.1e-3 dB, mono_odd).  Beyond that the GPU's pick
  on the GPU's own curve equals the model's pick on that same array exactly: integers and comparisons only, no window.
  Measured on one MI355X: max |nmr - model| 4.2e-9 dB over all cases; smallest margins on the excerpts (first 24 hops,
  136 to 262 units each) 4.8e-4 dB (quar48_1 at 0 dB), no unit inside the window anywhere; cap_48: 89 of 104 units over
  their cap.
  Bytes.  encode_pack_alloc gives the model encoder's stream byte for byte for the GPU's own allocation, a random
  valid one, zeros and one carrying 1, -3 and 99; the pick's n_bytes are the record lengths written; every record
  parses to its end; the decoder's PCM is the oracle's, int16 for int16.
  Solve.  On the GPU's curve every output equals the model's solve; the ABR stream is the NMR stream at the target
  found and fits; with nothing capped t is the brute-force minimum over the grid and total falls along a sweep.
  Never more than the search.  Unit by unit, outside the window and where neither path caps, every band's size is at
  most the one encode_pack_nmr gives at the same target and cap, and the stream is no larger.
  Closed loop.  quality.nmr_of_file of the finished bytes gives at most target + 1e-4 dB for every live band of every
  uncapped unit.
"""
import ctypes
import functools

import numpy as np
import pytest

import band_model as bm
import nmr_model as nm
import rate_model as rm
import soak_programmes as sp
from conftest import EXCERPTS, load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

NMR_TOL = 1e-5              # dB
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
# the constructions of tests/test_gpu_rate.py's SHAPES
def excerpt(name, h0, h1):
    ex = load_excerpt(name)
    return np.ascontiguousarray(ex["pcm"][h0 * 1024:h1 * 1024]), int(ex["sr"])


def silence_and_drop():
    """digital silence, a short-coded hop the reference drops (zeros before a burst), ordinary hops"""
    rng = np.random.default_rng(5)
    pcm = np.zeros((6 * 1024, 2), np.int16)
    pcm[1024:2048] = rng.integers(-3000, 3000, (1024, 2))
    pcm[3 * 1024 + 900:4 * 1024] = rng.integers(-30000, 30000, (124, 2))
    pcm[4 * 1024:] = rng.integers(-3000, 3000, (2 * 1024, 2))
    return pcm, 48000


# name -> (material, block switching, target dB, cap kb/s)
SHAPES = {
    "mono_odd": (lambda: (excerpt("castanet", 24, 29)[0][:, :1].copy(), 44100), True, -3.0, 320),
    "stereo_long_only": (lambda: excerpt("harpsichord", 0, 5), False, -6.0, 320),         # frame_flags = NULL
    "one_hop": (lambda: excerpt("castanet", 26, 27), True, 0.0, 320),
    "silence_and_drop": (silence_and_drop, True, -3.0, 320),
    "rate_96k": (lambda: (sp.programme(30_012, 5, 3, 96000), 96000), True, -3.0, 320),    # three channels, dummy band
    "cap_48": (lambda: excerpt("spmg", 0, 8), True, -6.0, 48),                            # the cap engages
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(pcm, sr, block switching, target, cap, analysis, model curve): computed once, shared, never changed"""
    make, bs, target, cap = SHAPES[name]
    pcm, sr = make()
    a = rm.analysis(pcm, sr, bs)
    return pcm, sr, bs, target, cap, a, bm.curve(a, cap)


@functools.lru_cache(maxsize=None)
def excerpt_case(name):
    pcm, sr = excerpt(name, 0, 24)
    a = rm.analysis(pcm, sr, True)
    return pcm, sr, a, bm.curve(a, 320)


_GPU = {}


def gpu_curve(A, key, pcm, sr, bs, cap, view_of=None):
    """Encoder.band_curve on the stream's blocks, once per case -> dict: host arrays, device curve, enc, view, flags,
    status (the words of a search that caps every unit: BitAlloc at the cap budget, as the curve runs it).
    view_of(enc, pcm): another view of the same blocks (tests/test_gpu_pcm_views.py; its key must be its own)"""
    if key not in _GPU:
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, cap, bs, None)
        if view_of is not None:
            view = view_of(enc, pcm)
        dev = enc.band_curve(view, flags, cp.targetBitsPerSample)
        host = {k: dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")}
        status = enc.encode_pack_nmr(view, flags, -1000.0, cp.targetBitsPerSample)["status"].cpu().numpy()
        # the header once: header_bytes() adds the delay block to cp.numSamples, as the reference's writer does
        _GPU[key] = {"host": host, "dev": dev, "enc": enc, "view": view, "flags": flags, "status": status, "cp": cp,
                     "head": A.pacfile.header_bytes(cp)}
    return _GPU[key]


def check_flags(a, flags):
    if flags is not None:
        want = np.array([l * 1 + c * 2 + n * 4 for (l, c, n) in a["flags"]], np.uint8)
        assert np.array_equal(flags.cpu().numpy(), want)                    # the GPU's detector gave the model's flags
    else:
        assert not any(f[1] for f in a["flags"])


def alloc_stream(A, g, pcm, alloc):
    """Encoder.encode_pack_alloc through the whole stream -> (.pac bytes, outputs)"""
    out = g["enc"].encode_pack_alloc(g["view"], g["flags"], np.ascontiguousarray(alloc))
    body, total = g["enc"].gather_body(out["payload"], out["n_bytes"])
    return g["head"] + body[:int(total.item())].cpu().numpy().tobytes(), out


def compare_curve(model, g, what):
    host = g["host"]
    unit, _ = bm.layout(model)
    live = unit >= 0
    assert np.array_equal(host["cap"], model["cap"]), what
    fin = np.isfinite(model["nmr"])
    assert np.array_equal(np.isposinf(host["nmr"]), np.isposinf(model["nmr"])), what
    assert np.array_equal(np.isfinite(host["nmr"]), fin), what
    assert fin[live][:, :model["n_cand"]].all(), what                       # every live band, every size: a value
    assert np.isnan(host["nmr"][~live]).all(), what                         # no band: not written
    err = np.abs(host["nmr"][fin] - model["nmr"][fin]).max() if fin.any() else 0.0
    guard = (g["status"] & 16) != 0
    print(f"{what}: {int((model['cap'] >= 0).sum())} units, {int(live.sum())} bands, max |nmr - model| {err:.3g} dB, "
          f"{int(guard.sum())} cf with PACX_ST_GUARD")
    assert err <= NMR_TOL, what
    assert np.array_equal(host["cap_alloc"][~guard], model["cap_alloc"][~guard]), what
    assert not host["cap_alloc"][~live].any(), what
    return err


def compare_pick(A, model, g, target, what):
    """-> (the GPU's pick as NumPy, model evaluate() detail, near [n_cf, 8])"""
    t = int(round(target * 64))
    assert t == target * 64
    pick = {k: v.cpu().numpy() for k, v in g["enc"].band_pick(g["dev"], target).items()}
    ref = bm.evaluate(model, t, detail=True)
    margin = bm.margins(model, target)
    live = model["cap"] >= 0
    near = live & (margin < WINDOW)
    capped_units = (ref[4] | ref[5]) & live
    print(f"{what}: {int(live.sum())} units, {int(capped_units.sum())} capped ({int((ref[5] & live).sum())} over the "
          f"cap, {int((ref[4] & live).sum())} with a band missed), smallest margin "
          f"{margin[live].min() if live.any() else float('nan'):.3g} dB, {int(near.sum())} inside the window")
    assert near.sum() <= LEFT_OUT * live.sum(), what
    unit, _ = bm.layout(model)
    near_slot = np.take_along_axis(near, np.maximum(unit, 0), axis=1) & (unit >= 0)
    assert np.array_equal(pick["bit_alloc"][~near_slot], ref[1][~near_slot]), what
    cf_ok = ~near.any(axis=1)
    assert np.array_equal(pick["n_bytes"][cf_ok], ref[2][cf_ok]), what
    assert np.array_equal(pick["capped"][cf_ok], ref[3][cf_ok]), what
    # on the GPU's own curve: integers and comparisons only, no window
    own = bm.evaluate(bm.with_arrays(model, **g["host"]), t)
    assert np.array_equal(pick["bit_alloc"], own[1]), what
    assert np.array_equal(pick["n_bytes"], own[2]) and np.array_equal(pick["capped"], own[3]), what
    return pick, ref, near


def check_stream(A, data, n_bytes, what):
    """every record parses to its end and has the predicted length; the decoder's PCM is the oracle's"""
    recs, _ = nm.records(data)
    assert (recs[-1][0] + recs[-1][1] if recs else len(data)) == len(data), what
    if n_bytes is not None:
        assert np.array_equal(np.array([n for _, n in recs]), n_bytes[n_bytes > 0]), what
    assert np.array_equal(A.pacfile.decode_stream(data), po.decode_stream(data)), what


# ------------------------------------------------------------------ 1. curve, 2. pick, 3. bytes on the shapes
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(A, name):
    """one channel (an odd number of channel-frames), no flags, a single hop, digital silence and a dropped hop, three
    channels on the 96 kHz band layout (the dummy band), a cap most units exceed"""
    pcm, sr, bs, target, cap, a, model = shape_case(name)
    g = gpu_curve(A, name, pcm, sr, bs, cap)
    check_flags(a, g["flags"])
    compare_curve(model, g, name)
    pick, ref, near = compare_pick(A, model, g, target, name)
    assert not near.any(), name                                  # the model alone leaves out none of these
    live = model["cap"] >= 0
    if name == "stereo_long_only":
        assert g["flags"] is None and (model["cap"][:, 1:] == -1).all()
    if name == "silence_and_drop":
        assert any(a["dropped"]) and (model["cap"] == -1).all(axis=1).any()
    if name == "rate_96k":
        assert a["n_ch"] == 3 and any(f[1] for f in a["flags"]) and model["lines_long"].sum() < 1024
    if name == "cap_48":
        assert (ref[5] & live).sum() > 0.5 * live.sum()          # the cap_alloc path is exercised
    else:
        assert not (ref[4] & live).any()                         # no band misses its target at 16 bits
    # the second pass: the GPU's own allocation -> the model encoder's bytes, records of the predicted lengths
    data, out = alloc_stream(A, g, pcm, pick["bit_alloc"])
    assert data == bm.encode(a, pick["bit_alloc"], len(pcm)), name
    assert np.array_equal(out["n_bytes"].cpu().numpy(), pick["n_bytes"]), name
    assert np.array_equal(out["bit_alloc"].cpu().numpy(), pick["bit_alloc"]), name
    check_stream(A, data, pick["n_bytes"], name)
    # the stream functions give that stream
    assert data == A.pacfile.encode_stream_nmr(pcm, sr, target, max_kbps_per_channel=cap, block_switching=bs,
                                               allocation="band"), name


@pytest.mark.parametrize("kind", ["random", "zero", "unclean"])
@pytest.mark.parametrize("name", ["mono_odd", "stereo_long_only", "rate_96k"])
def test_given_allocations_give_the_model_encoders_bytes(A, name, kind):
    pcm, sr, bs, target, cap, a, model = shape_case(name)
    g = gpu_curve(A, name, pcm, sr, bs, cap)
    shape = model["cap_alloc"].shape
    rng = np.random.default_rng(13)
    if kind == "random":                                         # representable sizes only, slots without a band too
        alloc = rng.choice(np.array([0] + list(range(2, 17))), shape).astype(np.int32)
    elif kind == "zero":
        alloc = np.zeros(shape, np.int32)
    else:                                                        # sanitised as defined: 1, -3 -> 0, 99 -> 16
        alloc = rng.choice(np.array([1, -3, 99, 0, 2, 5, 9]), shape, p=[.15, .15, .1, .15, .15, .15, .15]).astype(np.int32)
    data, out = alloc_stream(A, g, pcm, alloc)
    assert data == bm.encode(a, alloc, len(pcm)), (name, kind)
    unit, _ = bm.layout(model)
    assert np.array_equal(out["bit_alloc"].cpu().numpy()[unit >= 0], bm.sanitise(model, alloc)[unit >= 0]), (name, kind)
    assert not (out["status"].cpu().numpy() & A._lib.ST_RATE_CAP).any()
    check_stream(A, data, out["n_bytes"].cpu().numpy(), (name, kind))


# ------------------------------------------------------------------ 4. the excerpts: pick, never more than the search
def closed_loop(a, rep, capped, target, what):
    """nmr_of_file's values of every live band of every uncapped channel-block stay below target + WINDOW"""
    n = 0
    for f, row in enumerate(a["units"]):
        if row is None:
            assert np.isnan(rep.nmr_db[f]).all(), what
            continue
        for ch in range(len(row)):
            if not capped[f, ch]:
                vals = rep.nmr_db[f, ch]
                assert np.nanmax(vals) <= target + WINDOW, (what, f, ch, float(np.nanmax(vals)))
                n += 1
    return n


@pytest.mark.parametrize("target", [0.0, -6.0])
@pytest.mark.parametrize("name", EXCERPTS)
def test_excerpts(A, name, target):
    pcm, sr, a, model = excerpt_case(name)
    what = f"{name} {target:+.0f} dB"
    g = gpu_curve(A, ("excerpt", name), pcm, sr, True, 320)
    check_flags(a, g["flags"])
    compare_curve(model, g, what)
    pick, ref, near = compare_pick(A, model, g, target, what)
    data, rep, info = A.quality.encode_stream_to_nmr(pcm, sr, target, block_switching=True, allocation="band")
    n_ch, n_blocks = a["n_ch"], len(a["flags"])
    assert info["allocation"] == "band" and "budget" not in info
    assert np.array_equal(info["bit_alloc"].reshape(n_blocks * n_ch, -1), pick["bit_alloc"]), what
    assert np.array_equal(info["capped"].reshape(-1), pick["capped"]), what
    assert data == bm.encode(a, pick["bit_alloc"], len(pcm)), what
    check_stream(A, data, pick["n_bytes"], what)
    assert abs(info["kbps_per_channel"] - rm.kbps_per_channel(a, data)) < 1e-9
    # ---- never more than the search: same target, same cap
    cp = g["cp"]
    s = g["enc"].encode_pack_nmr(g["view"], g["flags"], target, cp.targetBitsPerSample)
    s_alloc, s_status = s["bit_alloc"].cpu().numpy(), s["status"].cpu().numpy()
    s_bytes = s["n_bytes"].cpu().numpy()
    # the search flags a capped unit on its cf: such channel-frames are left out whole, as are those with a unit inside
    # the window
    cf_ok = ~pick["capped"] & ((s_status & A._lib.ST_RATE_CAP) == 0) & ~near.any(axis=1)
    assert cf_ok.sum() > 0.5 * len(cf_ok), what
    assert (pick["bit_alloc"][cf_ok] <= s_alloc[cf_ok]).all(), what
    assert (pick["n_bytes"][cf_ok] <= s_bytes[cf_ok]).all(), what
    ratio = pick["n_bytes"][cf_ok].sum() / max(int(s_bytes[cf_ok].sum()), 1)
    print(f"{what}: band / search bytes {int(pick['n_bytes'][cf_ok].sum())} / {int(s_bytes[cf_ok].sum())} = {ratio:.3f} "
          f"over {int(cf_ok.sum())} of {len(cf_ok)} channel-frames, {info['kbps_per_channel']:.2f} kb/s per channel")
    assert ratio <= 1.0
    # ---- closed loop through the decoders and k_nmr
    assert closed_loop(a, rep, info["capped"], target, what) > 0


# ------------------------------------------------------------------ 5. the solve
def check_solve(g, model, limit, lo_db, hi_db, what):
    """Encoder.band_solve against band_model.solve on the same arrays: everything equal"""
    sol = g["enc"].band_solve(g["dev"], limit, lo_db, hi_db)
    ref = bm.solve(bm.with_arrays(model, **g["host"]), limit, int(lo_db * 64), int(hi_db * 64))
    got = (int(round(sol["target_nmr_db"] * 64)), int(sol["met"]), sol["total_bytes"])
    print(f"{what}: limit {limit}: t {got[0]} ({got[0] / 64:+.3f} dB), met {got[1]}, total {got[2]}; model "
          f"{ref['t']}, {ref['met']}, {ref['total']}; {len(ref['path'])} probes")
    assert got == (ref["t"], ref["met"], ref["total"]), what
    assert np.array_equal(sol["bit_alloc"].cpu().numpy(), ref["bit_alloc"]), what
    assert np.array_equal(sol["n_bytes"].cpu().numpy(), ref["n_bytes"]), what
    assert np.array_equal(sol["capped"].cpu().numpy(), ref["capped"]), what
    return sol, ref


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_solve_on_shapes(A, name):
    pcm, sr, bs, target, cap, a, model = shape_case(name)
    g = gpu_curve(A, name, pcm, sr, bs, cap)
    own = bm.with_arrays(model, **g["host"])
    small, big = bm.total(own, 30 * 64), bm.total(own, -30 * 64)
    for share in (0.2, 0.5, 0.9):
        check_solve(g, model, int(small + share * (big - small)), -30, 30, name)
    sol, ref = check_solve(g, model, small - 1, -30, 30, f"{name} unreachable")
    assert not sol["met"] and sol["target_nmr_db"] == 30.0 and sol["total_bytes"] == small
    sol, ref = check_solve(g, model, small, -30, 30, f"{name} limit == total(t_hi)")
    assert sol["met"] and sol["total_bytes"] <= small
    mid = bm.solve(own, (small + big) // 2)
    sol, ref = check_solve(g, model, mid["total"], -30, 30, f"{name} limit == total(t)")
    assert sol["total_bytes"] <= mid["total"]
    check_solve(g, model, (small + big) // 2, 0.078125, 0.078125, f"{name} one grid point")


def test_solve_is_the_grid_minimum_when_nothing_is_capped(A):
    pcm, sr, bs, target, cap, a, model = shape_case("stereo_long_only")
    g = gpu_curve(A, "stereo_long_only", pcm, sr, bs, cap)
    own = bm.with_arrays(model, **g["host"])
    t_lo, t_hi = -12 * 64, 20 * 64
    ev = {t: bm.evaluate(own, t) for t in range(t_lo, t_hi + 1)}
    assert not any(e[3].any() for e in ev.values())              # nothing capped anywhere on the grid
    totals = {t: e[0] for t, e in ev.items()}
    for share in (0.1, 0.5, 0.9):
        limit = int(totals[t_hi] + share * (totals[t_lo] - totals[t_hi]))
        sol, ref = check_solve(g, model, limit, t_lo / 64, t_hi / 64, f"grid minimum {share}")
        assert int(round(sol["target_nmr_db"] * 64)) == min(t for t, tot in totals.items() if tot <= limit)
    # the GPU's own totals along a sweep of 100 grid targets: non-increasing
    sweep = [int(g["enc"].band_pick(g["dev"], t / 64)["n_bytes"].sum().item()) for t in
             np.linspace(t_lo, t_hi, 100).astype(int)]
    assert all(b <= a_ for a_, b in zip(sweep, sweep[1:])) and sweep[-1] < sweep[0]


@pytest.mark.parametrize("kbps", [96, 128])
def test_abr_stream_is_the_nmr_stream_at_the_target_found(A, kbps):
    pcm, sr, a, model = excerpt_case("spmg")
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    data, rep, info = A.quality.encode_stream_to_rate(pcm, sr, kbps_per_channel=kbps, block_switching=True,
                                                      allocation="band")
    assert data == A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=kbps, block_switching=True, allocation="band")
    limit = int(np.floor(kbps * 1000 * n_ch * blocks * 1024 / sr / 8))
    recs, _ = nm.records(data)
    body = len(data) - (recs[0][0] - 4)
    budget = A.quality.encode_stream_to_rate(pcm, sr, kbps_per_channel=kbps, block_switching=True)[2]
    print(f"spmg {kbps} kb/s: band target {info['target_nmr_db']:+.3f} dB (budget allocation: "
          f"{budget['target_nmr_db']:+.3f} dB), body {body} of {limit} bytes")
    assert info["limit_bytes"] == limit and body == info["total_bytes"] <= limit
    assert np.array_equal(np.array([n for _, n in recs]), info["n_bytes"][info["n_bytes"] > 0])
    T = info["target_nmr_db"]
    assert data == A.pacfile.encode_stream_nmr(pcm, sr, T, block_switching=True, allocation="band")
    assert data == bm.encode(a, info["bit_alloc"].reshape(blocks * n_ch, -1), len(pcm))
    check_stream(A, data, None, kbps)
    assert info["allocation"] == "band" and info["kbps_per_channel"] <= kbps
    # the same guarantee takes fewer bits, so the same size buys a target at least as low
    if not info["capped"].any() and not budget["capped"].any():
        assert T <= budget["target_nmr_db"]


def test_two_sizes_from_one_curve_and_the_plot_arrays(A):
    pcm, sr, a, model = excerpt_case("spmg")
    both = A.quality.encode_stream_to_rate(pcm, sr, kbps_per_channel=[96, 128], block_switching=True, allocation="band")
    assert len(both) == 2
    for (data, rep, info), kbps in zip(both, (96, 128)):
        assert data == A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=kbps, block_switching=True,
                                                   allocation="band")
    assert both[0][2]["target_nmr_db"] > both[1][2]["target_nmr_db"] and len(both[0][0]) < len(both[1][0])
    c = A.quality.band_curve(pcm, sr, block_switching=True)
    stride = model["band_stride"]
    assert c["nmr"].shape == (26, 2, stride, 16) and c["cap"].shape == (26, 2, 8) and c["cap_alloc"].shape == (26, 2, stride)
    assert np.array_equal(c["cap"].reshape(-1, 8), model["cap"])


# ------------------------------------------------------------------ 6. defaults, unsupported, bad arguments
def test_defaults_and_the_keyword(A):
    pcm, sr = excerpt("castanet", 24, 27)
    nmr, abr = A.pacfile.encode_stream_nmr, A.pacfile.encode_stream_abr
    assert nmr(pcm, sr, -3.0, block_switching=True) == nmr(pcm, sr, -3.0, block_switching=True, allocation="budget")
    assert abr(pcm, sr, kbps_per_channel=96, block_switching=True) == \
        abr(pcm, sr, kbps_per_channel=96, block_switching=True, allocation="budget")
    assert nmr(pcm, sr, -3.0, block_switching=True, allocation="band") != nmr(pcm, sr, -3.0, block_switching=True)
    info = A.quality.encode_stream_to_nmr(pcm, sr, -3.0, block_switching=True)[2]
    assert info["allocation"] == "budget" and "budget" in info and "bit_alloc" in info
    for fn, args in ((nmr, (-3.0,)), (A.quality.encode_stream_to_nmr, (-3.0,))):
        with pytest.raises(ValueError, match="allocation"):
            fn(pcm, sr, *args, allocation="bands")
    for fn in (abr, A.quality.encode_stream_to_rate):
        with pytest.raises(ValueError, match="allocation"):
            fn(pcm, sr, kbps_per_channel=96, allocation=None)
    with pytest.raises(ValueError, match="smallest size"):       # unreachable: the message names the smallest size
        abr(pcm, sr, kbps_per_channel=0.5, allocation="band")
    for kw in ({"n_lines": 512}, {"chunk_hops": 4}, {"use_vq": True}, {"use_sbr": True}):
        with pytest.raises(NotImplementedError):
            nmr(pcm, sr, -3.0, allocation="band", **kw)
    with pytest.raises(ValueError):
        nmr(pcm, sr, float("nan"), allocation="band")


def test_unsupported_and_bad_arguments(A):
    import torch
    pcm, sr = excerpt("castanet", 24, 26)
    ptr = A.engine._ptr
    for kw in ({"use_vq": True}, {"use_vq": True, "use_sbr": True}, {"use_sbr": True}):
        enc = A.engine.Encoder(sr, 128 / (sr / 1000), **kw)
        view = A.engine.PcmView.stream(A.pacfile.device_stream(enc, pcm), 1024)
        with pytest.raises(NotImplementedError):
            enc.band_curve(view, None, 7.0)
        with pytest.raises(NotImplementedError):
            enc.encode_pack_alloc(view, None, np.zeros((view.n_cf, enc.band_stride), np.int32))
        assert enc.lib.pacx_band_curve_batch(enc.h, ctypes.byref(view.c), None, 7.0, None, None, None,
                                             None) == A._lib.E_UNSUPPORTED
        assert enc.lib.pacx_band_pick(enc.h, 1, None, None, None, 0.0, None, None, None, None) == A._lib.E_UNSUPPORTED
        assert enc.lib.pacx_band_solve(enc.h, 1, None, None, None, 100, -30.0, 30.0, None, None, None, None,
                                       None) == A._lib.E_UNSUPPORTED
        assert enc.lib.pacx_encode_pack_alloc_batch(enc.h, ctypes.byref(view.c), None, *([None] * 9)) == A._lib.E_UNSUPPORTED
        enc.close()
    enc = A.engine.Encoder(sr, 128 / (sr / 1000))
    view = A.engine.PcmView.stream(A.pacfile.device_stream(enc, pcm), 1024)
    for cap in (0.0, -1.0, float("nan"), 16.5):
        with pytest.raises(A._lib.PacxError, match="max_bits_per_sample"):
            enc.band_curve(view, None, cap)
    c = enc.band_curve(view, None, 7.0)
    for missing in range(3):                                     # every output of the curve in turn
        args = [ptr(c["nmr"]), ptr(c["cap"]), ptr(c["cap_alloc"])]
        args[missing] = None
        assert enc.lib.pacx_band_curve_batch(enc.h, ctypes.byref(view.c), None, 7.0, *args, None) == A._lib.E_ARG, missing
        assert b"null pointer" in enc.lib.pacx_last_error(enc.h)
    with pytest.raises(ValueError):
        enc.band_curve(view, None, 7.0, out={"nmr": c["nmr"][:, :, :8], "cap": c["cap"], "cap_alloc": c["cap_alloc"]})
    for target in (float("nan"), float("inf")):
        with pytest.raises(A._lib.PacxError, match="not finite"):
            enc.band_pick(c, target)
    for lo, hi in ((float("nan"), 3.0), (-3.0, float("inf")), (3.0, -3.0), (-30.01, 30.0), (-30.0, 0.001), (-2e6, 0.0)):
        with pytest.raises(A._lib.PacxError):
            enc.band_solve(c, 1000, lo, hi)
    with pytest.raises(A._lib.PacxError, match="negative"):
        enc.band_solve(c, -1)
    with pytest.raises(ValueError):
        enc.band_pick({"nmr": c["nmr"], "cap": c["cap"][:, :4], "cap_alloc": c["cap_alloc"]}, 0.0)
    alloc = torch.zeros((view.n_cf, enc.band_stride), dtype=torch.int32, device=enc.device)
    nby = torch.zeros((view.n_cf,), dtype=torch.int32, device=enc.device)
    cpd = torch.zeros((view.n_cf,), dtype=torch.uint8, device=enc.device)
    res = torch.zeros((4,), dtype=torch.int32, device=enc.device)
    good = [ptr(c["nmr"]), ptr(c["cap"]), ptr(c["cap_alloc"]), 0.0, ptr(alloc), ptr(nby), ptr(cpd)]
    assert enc.lib.pacx_band_pick(enc.h, view.n_cf, *good, None) == 0
    for missing in (0, 1, 2, 4, 5, 6):
        args = list(good)
        args[missing] = None
        assert enc.lib.pacx_band_pick(enc.h, view.n_cf, *args, None) == A._lib.E_ARG, missing
    assert enc.lib.pacx_band_pick(enc.h, -1, *good, None) == A._lib.E_ARG
    good = [ptr(c["nmr"]), ptr(c["cap"]), ptr(c["cap_alloc"]), 1000, -30.0, 30.0, ptr(alloc), ptr(nby), ptr(cpd), ptr(res)]
    assert enc.lib.pacx_band_solve(enc.h, view.n_cf, *good, None) == 0
    for missing in (0, 1, 2, 6, 7, 8, 9):
        args = list(good)
        args[missing] = None
        assert enc.lib.pacx_band_solve(enc.h, view.n_cf, *args, None) == A._lib.E_ARG, missing
    # an empty batch: no pointers needed but the result's; everything fits at the lowest target
    res.fill_(-1)
    assert enc.lib.pacx_band_solve(enc.h, 0, None, None, None, 0, -30.0, 30.0, None, None, None, ptr(res), None) == 0
    r = res.cpu().numpy()
    assert (int(r[0]), int(r[1]), int(r.view(np.int64)[1])) == (-30 * 64, 1, 0)
    assert enc.lib.pacx_band_pick(enc.h, 0, None, None, None, 0.0, None, None, None, None) == 0
    out = enc.alloc_outputs(view.n_cf, with_payload=True)
    good = [ptr(alloc)] + [ptr(out[k]) for k in ("overall", "scale_factor", "bit_alloc", "mantissa", "status", "payload",
                                                 "n_bytes")]
    assert enc.lib.pacx_encode_pack_alloc_batch(enc.h, ctypes.byref(view.c), None, *good, None) == 0
    for missing in (0, 1, 2, 3, 5, 6, 7):                        # 4: mantissa is optional
        args = list(good)
        args[missing] = None
        assert enc.lib.pacx_encode_pack_alloc_batch(enc.h, ctypes.byref(view.c), None, *args, None) == A._lib.E_ARG, missing
    with pytest.raises(ValueError):
        enc.encode_pack_alloc(view, None, np.zeros((3, enc.band_stride), np.int32))
    torch.cuda.synchronize()
    enc.close()


@pytest.mark.parametrize("bs", [False, True])
def test_other_paths_do_not_move(A, bs):
    """the new path shares the handle's workspace (and grows it) and leaves no state behind"""
    ex = load_excerpt("castanet")
    pcm, sr = np.ascontiguousarray(ex["pcm"][24 * 1024:48 * 1024]), int(ex["sr"])       # the attack: the opening is silent
    before = A.pacfile.encode_stream(pcm, sr, 128, block_switching=bs)
    vbr = A.pacfile.encode_stream_nmr(pcm, sr, -3.0, max_kbps_per_channel=128, block_switching=bs)
    band = A.pacfile.encode_stream_nmr(pcm, sr, -3.0, max_kbps_per_channel=128, block_switching=bs, allocation="band")
    assert len(band) <= len(vbr) and band != vbr
    assert A.pacfile.encode_stream(pcm, sr, 128, block_switching=bs) == before
    assert A.pacfile.encode_stream_nmr(pcm, sr, -3.0, max_kbps_per_channel=128, block_switching=bs) == vbr
    assert A.pacfile.encode_stream_nmr(pcm, sr, -3.0, max_kbps_per_channel=128, block_switching=bs,
                                       allocation="band") == band
