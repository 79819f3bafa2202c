"""Gain-shape streams coded to an NMR target or a size, band by band, on the GPU (pacx_vq_band_curve_batch /
pacx_encode_vq_alloc_batch, Encoder.vq_band_curve / encode_vq_alloc, context.scalar_sibling,
pacfile.encode_stream_vq_nmr / _abr, quality.encode_stream_vq_to_nmr / _to_rate) against the NumPy statement of
tests/vq_band_model.py, whose curve for the test stream is the fixture tests/golden/vq_band.npz.

The stream: vq_band_model.STREAM, 4 hops of the castanet excerpt with block switching -- 6 blocks, 12 channel-frames,
two blocks short-coded -- at a cap of 320 kb/s per channel.

Bars.
  Curve.  Every finite entry within 1e-5 dB of the fixture (the project's NMR bar, tests/test_gpu_nmr.py); -inf, +inf
  and NaN (no band) at the same places; cap and cap_alloc equal.  No entry is excluded.
  Independent check.  A uniform allocation of 2, 9 and 16 bits through encode_vq_alloc, the existing decode_vq and
  Encoder.nmr gives the curve's column bit for bit.
  Pick.  On the GPU's own curve the sibling's band_pick is exactly band_model's pick; against the fixture's curve it is
  equal too, and no unit of the stream lies inside the project's tie window of 1e-4 dB at the targets used (asserted).
  Second pass.  n_bytes are the pick's, the bytes are vq_band_model.encode_stream_alloc's, the final allocation is the
  sanitised input outside all-zero bands.
  Closed loop.  quality.nmr_of_file of the finished bytes is at or below the target in every band of every uncapped
  channel-frame (no tolerance: curve and report run the same decoder and the same k_nmr); the oracle's decoder and the
  GPU's give the same PCM.
Measured on one MI355X: max |nmr - model| 9.1e-11 dB over the 5376 finite entries; smallest margins 0.058 / 0.0050 /
0.0048 dB at -6 / 0 / +6 dB; the closed loops' worst bands -3.013 dB (castanet) and -3.001 dB (harpsichord) at -3 dB.
"""
import functools

import numpy as np
import pytest

import band_model as bm
import nmr_model as nm
import rate_model as rm
import vq_band_model as vm
from conftest import load_excerpt
from oracle import pac_oracle_vq as pv

pytestmark = pytest.mark.gpu

NMR_TOL = 1e-5              # dB
WINDOW = 1e-4               # dB
CAP = vm.CAP_KBPS
TARGETS = (-6.0, 0.0, 6.0)


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


@functools.lru_cache(maxsize=None)
def case():
    """(pcm, sr, analysis, the fixture's curve): computed once, shared, never changed"""
    pcm, sr = vm.fixture_stream()
    return pcm, sr, rm.analysis(pcm, sr, True), vm.load_fixture()


_GPU = {}


def gpu_curve(A, key, pcm, sr, bs=True):
    """Encoder.vq_band_curve on the stream's blocks, once per stream"""
    if key not in _GPU:
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, CAP, bs, None, use_vq=True)
        assert enc.use_vq and not enc.use_sbr
        dev = enc.vq_band_curve(view, flags, cp.targetBitsPerSample)
        host = {k: dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")}
        _GPU[key] = {"host": host, "dev": dev, "enc": enc, "view": view, "flags": flags, "cp": cp,
                     "sib": A.context.scalar_sibling(enc), "head": A.pacfile.header_bytes(cp), "n_ch": pcm.shape[1]}
    return _GPU[key]


def main(A):
    pcm, sr, _, _ = case()
    return gpu_curve(A, "main", pcm, sr)


def tables_for(sr, n_ch):
    from oracle import pac_oracle as po
    return bm.tables(po.make_params(sr, n_ch, 128))


def stream_of(g, out):
    body, total = g["enc"].gather_body(out["payload"], out["n_bytes"])
    return g["head"] + body[:int(total.item())].cpu().numpy().tobytes()


def column_by_the_decoder(g, bits):
    """NMR rows of every band coded with `bits` bits a line, through encode_vq_alloc, decode_vq and Encoder.nmr"""
    import torch
    enc = g["enc"]
    alloc = torch.full((g["view"].n_cf, enc.band_stride), bits, dtype=torch.int32, device=enc.device)
    out = enc.encode_vq_alloc(g["view"], g["flags"], alloc)
    dec = enc.decode_vq(out["payload"], out["n_bytes"], g["n_ch"], want_lines=True, want_pcm=False)
    assert not (dec["status"].cpu().numpy() & (8 | 32)).any()
    return enc.nmr(g["view"], g["flags"], dec["lines"], dec["overall"])["nmr_db"].cpu().numpy(), out


def check_columns(g, sizes, what):
    nmr = g["host"]["nmr"]
    for bits in sizes:
        col, _ = column_by_the_decoder(g, bits)
        mine = nmr[:, :, bits - 1]
        fin = np.isfinite(mine)
        assert fin.any(), what
        assert np.array_equal(mine[fin].view(np.int64), col[fin].view(np.int64)), (what, bits)     # bit for bit
        assert np.array_equal(np.isnan(mine), np.isnan(col)), (what, bits)


# ------------------------------------------------------------------------------------------------ 1. the curve
def test_curve_is_the_fixtures(A):
    pcm, sr, a, F = case()
    g = main(A)
    want = np.array([l * 1 + c * 2 + n * 4 for (l, c, n) in a["flags"]], np.uint8)
    assert np.array_equal(g["flags"].cpu().numpy(), want)                   # the GPU's detector gave the model's flags
    host = g["host"]
    unit, _ = bm.layout(F)
    live = unit >= 0
    assert np.array_equal(host["cap"], F["cap"])
    for test in (np.isposinf, np.isneginf, np.isnan, np.isfinite):
        assert np.array_equal(test(host["nmr"]), test(F["nmr"])), test.__name__
    assert np.isnan(host["nmr"][~live]).all() and not np.isnan(host["nmr"][live]).any()
    fin = np.isfinite(F["nmr"])
    err = np.abs(host["nmr"][fin] - F["nmr"][fin])
    print(f"curve: {int((F['cap'] >= 0).sum())} units, {int(live.sum())} bands, {int(fin.sum())} finite entries, "
          f"max |nmr - model| {err.max():.3g} dB, {int(np.isneginf(F['nmr'][:, :, 1]).sum())} all-zero bands")
    assert err.max() <= NMR_TOL
    assert np.array_equal(host["cap_alloc"], F["cap_alloc"])


# ------------------------------------------------------------------------- 2. the same column by another road
def test_columns_by_encode_decode_nmr(A):
    check_columns(main(A), (2, 9, 16), "main")


# ------------------------------------------------------------------------------------------------ 3. the picks
@pytest.mark.parametrize("target", TARGETS)
def test_pick(A, target):
    _, _, _, F = case()
    g = main(A)
    t = int(round(target * bm.GRID))
    pick = {k: v.cpu().numpy() for k, v in g["sib"].band_pick(g["dev"], target).items()}
    own = bm.evaluate(bm.with_arrays(F, **g["host"]), t)
    assert np.array_equal(pick["bit_alloc"], own[1]) and np.array_equal(pick["n_bytes"], own[2])
    assert np.array_equal(pick["capped"], own[3])
    margin = bm.margins(F, target)
    live = F["cap"] >= 0
    print(f"pick at {target:g} dB: smallest margin {margin[live].min():.3g} dB, {int(own[3].sum())} cf capped")
    assert (margin[live] >= WINDOW).all()                  # no unit of the stream lies inside the tie window
    ref = bm.evaluate(F, t)
    assert np.array_equal(pick["bit_alloc"], ref[1]) and np.array_equal(pick["n_bytes"], ref[2])
    assert np.array_equal(pick["capped"], ref[3])


# ------------------------------------------------------------------------------------------ 4. the second pass
def test_second_pass(A):
    pcm, sr, a, F = case()
    g = main(A)
    pick = g["sib"].band_pick(g["dev"], 0.0)
    out = g["enc"].encode_vq_alloc(g["view"], g["flags"], pick["bit_alloc"])
    alloc = pick["bit_alloc"].cpu().numpy()
    assert np.array_equal(out["n_bytes"].cpu().numpy(), pick["n_bytes"].cpu().numpy())
    assert not (out["status"].cpu().numpy() & (8 | 128)).any()
    data, final, n_bytes = vm.encode_stream_alloc(a, alloc, len(pcm))
    assert np.array_equal(out["n_bytes"].cpu().numpy(), n_bytes)
    assert stream_of(g, out) == data
    unit, _ = bm.layout(F)
    zero = np.isneginf(F["nmr"][:, :, 1]) & (unit >= 0)
    got = out["bit_alloc"].cpu().numpy()
    assert np.array_equal(got, final)
    assert np.array_equal(got[~zero], bm.sanitise(F, alloc)[~zero]) and not got[zero].any()


# -------------------------------------------------------------------------------------------- 5. closed loop
def closed_loop(A, pcm, sr, target, what):
    data, rep, info = A.quality.encode_stream_vq_to_nmr(pcm, sr, target, CAP, block_switching=True)
    assert info["allocation"] == "band" and info["written"].all()
    assert not info["capped"].any(), what
    worst = np.nanmax(rep.nmr_db[~info["capped"]])
    print(f"{what}: {len(data)} bytes, {info['kbps_per_channel']:.1f} kb/s per channel, worst band {worst:.4f} dB "
          f"at a target of {target:g} dB")
    assert worst <= target, what
    assert data == A.pacfile.encode_stream_vq_nmr(pcm, sr, target, CAP, block_switching=True)
    assert np.array_equal(A.pacfile.decode_stream(data), pv.decode_stream_vq(data)), what
    return data, info


def test_closed_loop_castanet(A):
    pcm, sr, _, F = case()
    assert not bm.evaluate(F, int(-3.0 * bm.GRID))[3].any()             # the model caps no unit at this target
    closed_loop(A, pcm, sr, -3.0, "castanet")


def test_closed_loop_harpsichord(A):
    ex = load_excerpt("harpsichord")
    pcm, sr = np.ascontiguousarray(ex["pcm"][12 * 1024:16 * 1024]), int(ex["sr"])
    g = gpu_curve(A, "harpsichord", pcm, sr)
    assert (g["flags"].cpu().numpy() & 2).any() and not (g["flags"].cpu().numpy() & 2).all()
    own = bm.evaluate(bm.with_arrays(tables_for(sr, 2), **g["host"]), int(-3.0 * bm.GRID))
    assert not own[3].any()                                              # the model's pick on this curve caps no unit
    closed_loop(A, pcm, sr, -3.0, "harpsichord")


# ---------------------------------------------------------------------------------------- 6. to a size
def body_bytes(data):
    recs, _ = nm.records(data)
    return sum(n + 4 for _, n in recs), recs


@pytest.mark.parametrize("kbps", (96, 128))
def test_abr(A, kbps):
    pcm, sr, _, _ = case()
    data, rep, info = A.quality.encode_stream_vq_to_rate(pcm, sr, kbps, max_kbps_per_channel=CAP, block_switching=True)
    assert data == A.pacfile.encode_stream_vq_abr(pcm, sr, kbps, max_kbps_per_channel=CAP, block_switching=True)
    body, _ = body_bytes(data)
    limit = int(np.floor(kbps * 1000.0 * 2 * 6 * 1024 / sr / 8.0))
    print(f"{kbps} kb/s: target {info['target_nmr_db']:g} dB, body {body} of {limit} bytes")
    assert info["limit_bytes"] == limit and body == info["total_bytes"] <= limit
    assert data == A.pacfile.encode_stream_vq_nmr(pcm, sr, info["target_nmr_db"], CAP, block_switching=True)
    # a peak that never binds: the plain solve's bytes
    assert data == A.pacfile.encode_stream_vq_abr(pcm, sr, kbps, max_kbps_per_channel=CAP, block_switching=True,
                                                  segment_hops=2, peak_kbps_per_channel=100 * CAP)


def test_abr_segments(A):
    pcm, sr, _, _ = case()
    data, rep, info = A.quality.encode_stream_vq_to_rate(pcm, sr, 96, max_kbps_per_channel=CAP, block_switching=True,
                                                         segment_hops=2)
    seg = info["segments"]
    _, recs = body_bytes(data)
    assert len(recs) == 12 and len(seg["blocks"]) == 3
    for s in range(3):
        first, blocks = int(seg["first_block"][s]), int(seg["blocks"][s])
        at = A.pacfile.encode_stream_vq_nmr(pcm, sr, float(seg["target_nmr_db"][s]), CAP, block_switching=True)
        _, theirs = body_bytes(at)
        mine = [data[o:o + n] for o, n in recs[2 * first:2 * (first + blocks)]]
        assert mine == [at[o:o + n] for o, n in theirs[2 * first:2 * (first + blocks)]], s
        assert sum(len(r) + 4 for r in mine) == int(seg["total_bytes"][s]) <= int(seg["limit_bytes"][s]), s


# ------------------------------------------------------------------------------------------------ 7. edges
def test_no_frames(A):
    import torch
    g = main(A)
    enc = g["enc"]
    view = A.engine.PcmView.frames(torch.zeros((0, 2, 2048), dtype=torch.int16, device=enc.device))
    c = enc.vq_band_curve(view, None, CAP / (44100 / 1000))
    assert tuple(c["nmr"].shape) == (0, enc.band_stride, 16)
    out = enc.encode_vq_alloc(view, None, torch.zeros((0, enc.band_stride), dtype=torch.int32))
    assert out["n_bytes"].numel() == 0


def small_case(A, key, pcm, sr):
    """a stream without a fixture: cap and cap_alloc against the model (BitAlloc only: cheap), a column against the
    decoder's road, and the pick's lengths against the second pass"""
    g = gpu_curve(A, key, pcm, sr)
    a = rm.analysis(pcm, sr, True)
    n_ch = pcm.shape[1]
    assert g["view"].n_cf == len(a["flags"]) * n_ch
    for f, row in enumerate(a["units"]):
        assert row is not None
        for ch, us in enumerate(row):
            cf = f * n_ch + ch
            for sb, u in enumerate(us):
                nb = u.bands.nBands
                J = rm.cap_steps(a, u, CAP)
                assert g["host"]["cap"][cf, sb] == 32 * J
                assert np.array_equal(g["host"]["cap_alloc"][cf, sb * nb:(sb + 1) * nb], vm.cap_alloc_of(a["p"], u, J))
    check_columns(g, (9,), key)
    pick = g["sib"].band_pick(g["dev"], -3.0)
    out = g["enc"].encode_vq_alloc(g["view"], g["flags"], pick["bit_alloc"])
    assert np.array_equal(out["n_bytes"].cpu().numpy(), pick["n_bytes"].cpu().numpy())
    data = stream_of(g, out)
    assert np.array_equal(A.pacfile.decode_stream(data), pv.decode_stream_vq(data))
    return g


def test_one_channel_one_hop(A):
    pcm, sr, _, _ = case()
    g = small_case(A, "mono", np.ascontiguousarray(pcm[1024:2048, :1]), sr)
    assert g["view"].n_cf == 3


def test_three_channels(A):
    pcm, sr, _, _ = case()
    three = np.stack([pcm[1024:2048, 0], pcm[1024:2048, 1], pcm[2048:3072, 0]], axis=1)
    g = small_case(A, "three", np.ascontiguousarray(three), sr)
    assert g["view"].n_cf == 9


def test_digital_silence(A):
    pcm = np.zeros((2048, 2), np.int16)
    g = gpu_curve(A, "silence", pcm, 48000)
    c = tables_for(48000, 2)
    unit, _ = bm.layout(bm.with_arrays(c, **g["host"]))
    live = unit >= 0
    assert live.any() and np.isneginf(g["host"]["nmr"][live]).all() and not g["host"]["cap_alloc"].any()
    least = (4 + len(c["lines_long"]) * (12 + 4) + 4 + 7) >> 3
    pick = g["sib"].band_pick(g["dev"], -30.0)
    assert not pick["bit_alloc"].cpu().numpy().any() and (pick["n_bytes"].cpu().numpy() == least).all()
    import torch
    nine = torch.full((g["view"].n_cf, g["enc"].band_stride), 9, dtype=torch.int32)
    out = g["enc"].encode_vq_alloc(g["view"], g["flags"], nine)
    assert (out["n_bytes"].cpu().numpy() == least).all() and not out["bit_alloc"].cpu().numpy().any()


def test_garbage_allocations(A):
    pcm, sr, a, F = case()
    g = main(A)
    alloc = np.resize(np.array([-5, 1, 40, 7, 0, 2, 16, 17], np.int32), F["cap_alloc"].shape)
    out = g["enc"].encode_vq_alloc(g["view"], g["flags"], alloc)
    data, final, n_bytes = vm.encode_stream_alloc(a, alloc, len(pcm))
    assert np.array_equal(out["n_bytes"].cpu().numpy(), n_bytes)
    assert stream_of(g, out) == data
    unit, _ = bm.layout(F)
    live = unit >= 0
    zero = np.isneginf(F["nmr"][:, :, 1]) & live
    got = out["bit_alloc"].cpu().numpy()
    assert np.array_equal(got[live & ~zero], bm.sanitise(F, alloc)[live & ~zero])
    assert np.array_equal(got[live], final[live])


def test_encode_vq_unchanged_by_a_curve(A):
    g = main(A)
    enc = g["enc"]
    before = stream_of(g, enc.encode_vq(g["view"], g["flags"]))
    status = enc.encode_vq(g["view"], g["flags"])["status"].cpu().numpy()
    enc.vq_band_curve(g["view"], g["flags"], g["cp"].targetBitsPerSample)
    after = enc.encode_vq(g["view"], g["flags"])
    assert stream_of(g, after) == before and np.array_equal(after["status"].cpu().numpy(), status)


def test_other_handles_are_refused(A):
    import torch
    g = main(A)
    enc = g["enc"]
    sbr = A.context.encoder(enc.sample_rate, 96 / 44.1, use_vq=True, use_sbr=True)
    zeros = torch.zeros((g["view"].n_cf, enc.band_stride), dtype=torch.int32)
    for other in (g["sib"], sbr):
        assert other.band_stride == enc.band_stride
        with pytest.raises(NotImplementedError):
            other.vq_band_curve(g["view"], g["flags"], 7.0)
        with pytest.raises(NotImplementedError):
            other.encode_vq_alloc(g["view"], g["flags"], zeros)
    with pytest.raises(NotImplementedError):
        A.pacfile.encode_stream_nmr(case()[0], case()[1], -3.0, use_vq=True)
    with pytest.raises(NotImplementedError):
        enc.band_pick(g["dev"], 0.0)                       # the pick itself still wants a scalar handle
