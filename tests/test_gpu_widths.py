"""Field widths other than nScaleBits = 4 / nMantSizeBits = 12 on the GPU: the stream coders at every case of
tests/widths_cases.py against what the REFERENCE wrote and decoded (tests/golden/widths.part*.npz), and rate control at
three width pairs against the NumPy models, which tests/test_oracle_widths.py holds to the reference and to themselves
at these widths.

Material: one stream, six hops of the castanet excerpt with block switching (three short-coded hops, a start and a stop
window), stereo.

Bars.  Bytes, int16 PCM, allocations, scale factors, mantissas, budgets, record lengths, profiles and solves: equal.
NMR reports of the reference's bytes against the encode path's own: bit for bit (tests/test_gpu_nmr.py's same_report).
The two float comparisons are the project's own and are made by the functions of the tests that
state them: finite band-curve entries and the rate curve's worst within 1e-5 dB of the model
(tests/test_gpu_band.compare_curve, tests/test_gpu_abr.compare_curve), budgets and picks equal outside the tie window
of 1e-4 dB -- and tests/test_oracle_widths.py asserts that no unit of this stream lies inside it at the targets used,
so none is left out here (asserted again below).
"""
import functools
import itertools

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import profile_model as pm
import rate_model as rm
import seg_profile_model as sm
import vq_band_model as vm
import widths_cases as wc
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv
from test_gpu_abr import SENTINEL_B, SENTINEL_W
from test_gpu_abr import check_solve as check_rate_solve
from test_gpu_abr import compare_curve as compare_rate_curve
from test_gpu_band import WINDOW, check_solve, check_stream, closed_loop, compare_curve, compare_pick
from test_gpu_nmr import same_report
from test_gpu_round3 import _set, fresh_handles                          # noqa: F401  (fresh_handles is a fixture)

pytestmark = pytest.mark.gpu

GRID = bm.GRID
ROUTED = [c for c in wc.CASES if c[1:3] in ((3, 5), (4, 3))]
SCALAR = [c for c in wc.CASES if not wc.is_vq(c)]


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def kw_of(case):
    coder, ns, nm_bits, kbps = case
    return dict(n_scale_bits=ns, n_mant_size_bits=nm_bits, use_vq=wc.is_vq(case), use_sbr=wc.uses_sbr(case))


def gpu_encode(A, case, block_switching=True, **more):
    pcm, sr = wc.stream()
    return A.pacfile.encode_stream(pcm, sr, case[3], block_switching, **kw_of(case), **more)


def reference(case, block_switching=True):
    return bytes(wc.fixture()[("pac_bs_" if block_switching else "pac_long_") + wc.tag_of(case)])


def first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}, first difference at byte {at}"


# ------------------------------------------------------------------------- 1. the stream coders at every case
@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_encode_stream_writes_the_references_bytes(A, case):
    got, want = gpu_encode(A, case), reference(case)
    assert got == want, first_difference(got, want)
    got = gpu_encode(A, case, chunk_hops=2)
    assert got == want, "chunk_hops=2: " + first_difference(got, want)


@pytest.mark.parametrize("case", SCALAR, ids=wc.case_id)
def test_encode_stream_writes_the_references_bytes_long_only(A, case):
    """no flags: the all-long route through the fused front end"""
    got, want = gpu_encode(A, case, False), reference(case, False)
    assert got == want, first_difference(got, want)
    got = gpu_encode(A, case, False, chunk_hops=2)
    assert got == want, "chunk_hops=2: " + first_difference(got, want)


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_decode_stream_gives_the_references_pcm(A, case):
    g = wc.fixture()
    data, want = reference(case), g["dec_bs_" + wc.tag_of(case)]
    got = A.pacfile.decode_stream(data)
    assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)
    got = A.pacfile.decode_stream(data, chunk_bytes=2 * 2196)
    assert got.shape == want.shape and np.array_equal(got, want), "in chunks"


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_nmr_of_the_references_file_is_the_encode_paths_own(A, case):
    pcm, sr = wc.stream()
    data, rep = A.quality.encode_stream_report(pcm, sr, case[3], block_switching=True, **kw_of(case))
    assert data == reference(case)
    other = A.quality.nmr_of_file(pcm, reference(case))
    same_report(other, rep)
    assert rep.short.tolist() == [bool(f[1]) for f in wc.FLAGS] + [False] and (rep.record >= 0).all()
    live = ~np.isnan(rep.nmr_db)
    assert live.any() and np.isfinite(rep.nmr_db[live]).all()


@functools.lru_cache(maxsize=None)
def oracle_parts(case):
    """(flags, parts per channel) of every block the oracle writes for the case"""
    pcm, sr = wc.stream()
    coder, ns, nm_bits, kbps = case
    collect = []
    if wc.is_vq(case):
        data = pv.encode_stream_vq(pcm, sr, kbps, True, collect=collect, n_scale_bits=ns, n_mant_size_bits=nm_bits)
    else:
        data = po.encode_stream(pcm, sr, kbps, True, collect=collect, n_scale_bits=ns, n_mant_size_bits=nm_bits)
    assert data == reference(case)
    return collect


def stage_view(A, case):
    """(encoder, view, flags) of the case's stream, as encode_stream makes them"""
    pcm, sr = wc.stream()
    enc = A.context.encoder(sr, case[3] / (sr / 1000), case[1], case[2], use_vq=wc.is_vq(case), use_sbr=wc.uses_sbr(case))
    planar = A.pacfile.device_stream(enc, pcm)
    flags = enc.transient_flags(planar, len(pcm) // 1024)[1]
    return enc, A.engine.PcmView.stream(planar, 1024), flags


def check_status(A, status):
    """every channel-frame has a defined payload: no hop dropped, nothing the reference's coder fails on"""
    L = A._lib
    assert len(status) == 16
    assert not (status & (L.ST_ZERO_SUBBLOCK | L.ST_VQ_UNDEFINED | L.ST_MALFORMED | L.ST_REF_RAISES)).any(), status


@pytest.mark.parametrize("case", SCALAR, ids=wc.case_id)
def test_encode_equals_the_oracle_stage_by_stage(A, case):
    """Encoder.encode unpacked: a mismatch names the block, the channel, the unit, the stage and the band"""
    enc, view, flags = stage_view(A, case)
    out = enc.encode(view, flags)
    host = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    want_flags = [l * 1 + c * 2 + n * 4 for (l, c, n) in wc.FLAGS + [(0, 0, 0)]]
    assert host["flags"].tolist() == want_flags
    check_status(A, host["status"])
    parts = oracle_parts(case)
    assert len(parts) == view.n_frames == 8
    top, cap = (1 << case[1]) - 1, min(1 << case[2], 16)
    seen_sf, seen_alloc = set(), set()
    for f, (fl, per_ch) in enumerate(parts):
        for ch in range(2):
            i = f * 2 + ch
            for sb, (sf, alloc, mant, overall) in enumerate(per_ch[ch]):
                got = A.codec.unpack_short(enc, host, i, sb) if fl[1] else A.codec.unpack_long(enc, host, i)
                where = f"block {f} {tuple(int(v) for v in fl)} channel {ch} unit {sb}"
                assert got[3] == overall, f"{where}: overall scale {got[3]} against {overall}"
                for name, g_, w_ in (("allocation", got[1], alloc), ("scale factor", got[0], sf)):
                    bad = np.nonzero(np.asarray(g_) != np.asarray(w_))[0]
                    assert not len(bad), f"{where}: {name} of band {bad[0]}: {g_[bad[0]]} against {w_[bad[0]]}"
                bad = np.nonzero(got[2] != mant)[0] if len(got[2]) == len(mant) else [0]
                assert len(got[2]) == len(mant) and not len(bad), f"{where}: mantissa {bad[0]} of the coded lines"
                seen_sf |= set(int(v) for v in sf) | {int(overall)}
                seen_alloc |= set(int(v) for v in alloc)
    assert max(seen_sf) <= top and max(seen_alloc) <= cap
    if case[1:3] in ((1, 4), (2, 2)):
        assert top in seen_sf                                   # the cap 2^nScaleBits - 1 is reached
    if case == ("sc", 4, 3, 320):
        assert 8 in seen_alloc


@pytest.mark.parametrize("case", [c for c in wc.CASES if wc.is_vq(c)], ids=wc.case_id)
def test_encode_vq_heads_equal_the_oracles(A, case):
    """the gain-shape coder's overall scales and final allocations, block by block"""
    enc, view, flags = stage_view(A, case)
    out = enc.encode_vq(view, flags)
    overall, alloc = out["overall"].cpu().numpy(), out["bit_alloc"].cpu().numpy()
    check_status(A, out["status"].cpu().numpy())
    for f, (fl, per_ch) in enumerate(oracle_parts(case)):
        for ch in range(2):
            for sb, (want_alloc, _, _, want_overall) in enumerate(per_ch[ch]):
                nb = len(want_alloc)
                where = f"block {f} {tuple(int(v) for v in fl)} channel {ch} unit {sb}"
                assert overall[f * 2 + ch, sb] == want_overall, f"{where}: overall scale"
                got = alloc[f * 2 + ch, sb * nb:(sb + 1) * nb]
                bad = np.nonzero(got != np.asarray(want_alloc))[0]
                assert not len(bad), f"{where}: allocation of band {bad[0]}: {got[bad[0]]} against {want_alloc[bad[0]]}"


# ------------------------------------------------------------------------- 2. routing at 3 / 5 and 4 / 3
@pytest.mark.parametrize("case", [c for c in ROUTED if not wc.is_vq(c)], ids=wc.case_id)
def test_scalar_path_switches(A, monkeypatch, fresh_handles, case):
    n = 0
    for bs in (True, False):
        want = reference(case, bs)
        for fuse, split in itertools.product((None, "0", "1"), (None, "0")):
            _set(A, monkeypatch, {"PACX_FUSE_TAIL": fuse, "PACX_SPLIT_SHORT": split})
            got = gpu_encode(A, case, bs)
            assert got == want, (bs, fuse, split, first_difference(got, want))
            n += 1
    assert n == 12
    _set(A, monkeypatch, {})


@pytest.mark.parametrize("case", [c for c in ROUTED if wc.is_vq(c)], ids=wc.case_id)
def test_gain_shape_path_switches(A, monkeypatch, fresh_handles, case):
    want = reference(case)
    pcm_want = wc.fixture()["dec_bs_" + wc.tag_of(case)]
    for env in ({}, {"PACX_VQ_FRAME": "0", "PACX_VQ_BFS": "0"}, {"PACX_VQ_FRAME": "0", "PACX_VQ_BFS": "1"},
                {"PACX_VQ_FUSE_ALLOC": "0"}, {"PACX_VQ_FRAME": "0", "PACX_VQ_BFS": "1", "PACX_VQ_FUSE_ALLOC": "0"}):
        _set(A, monkeypatch, env)
        got = gpu_encode(A, case)
        assert got == want, (env, first_difference(got, want))
    for env in ({}, {"PACX_VQ_DEC_FRAME": "0"}):
        _set(A, monkeypatch, env)
        assert np.array_equal(A.pacfile.decode_stream(want), pcm_want), env
    _set(A, monkeypatch, {})


# ------------------------------------------------------------------------- 3. widths the library refuses
def test_widths_out_of_range_are_refused(A):
    sr = 44100
    for ns, nm_bits in ((0, 12), (5, 12), (4, 0), (4, 17)):
        with pytest.raises(A._lib.PacxError, match=r"nScaleBits must be 1\.\.4, nMantSizeBits 1\.\.16"):
            A.engine.Encoder(sr, 128 / (sr / 1000), ns, nm_bits)
    for ns, nm_bits in ((1, 1), (4, 16)):                       # the corners of the range are taken
        enc = A.engine.Encoder(sr, 128 / (sr / 1000), ns, nm_bits)
        assert (enc.n_scale_bits, enc.n_mant_size_bits) == (ns, nm_bits) and enc.payload_stride > 0
        enc.close()


# ------------------------------------------------------------------------- 4. rate control at three width pairs
_RATE = {}


def rate_setup(A, ns, nm_bits, cap):
    """the handle, view and flags of the stream at these widths with the cap rate as the handle's, the band curve and
    the rate curve of the GPU: once per case"""
    import torch
    from audio_codec_amd.audiofile import CodingParams
    key = (ns, nm_bits, cap)
    if key in _RATE:
        return _RATE[key]
    pcm, sr = wc.stream()
    cap_bps = cap / (sr / 1000)
    enc = A.context.encoder(sr, cap_bps, ns, nm_bits)
    planar = A.pacfile.device_stream(enc, pcm)
    view = A.engine.PcmView.stream(planar, 1024)
    flags = enc.transient_flags(planar, len(pcm) // 1024)[1]
    cp = CodingParams()
    cp.sampleRate, cp.nChannels, cp.numSamples = sr, 2, len(pcm)
    cp.nMDCTLines = cp.nSamplesPerBlock = 1024
    cp.nScaleBits, cp.nMantSizeBits = ns, nm_bits
    cp.targetBitsPerSample = cap_bps
    cp.useSBR = cp.useVQ = False
    dev = enc.band_curve(view, flags, cap_bps)
    g = {"enc": enc, "view": view, "flags": flags, "cp": cp, "head": A.pacfile.header_bytes(cp), "cap_bps": cap_bps,
         "dev": dev, "host": {k: dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")},
         "status": enc.encode_pack_nmr(view, flags, -1000.0, cap_bps)["status"].cpu().numpy()}
    row, sub = enc.rate_curve_layout(cap_bps)
    out = {"worst": torch.full((view.n_cf, row), SENTINEL_W, dtype=torch.float64, device=enc.device),
           "bits": torch.full((view.n_cf, row), SENTINEL_B, dtype=torch.int32, device=enc.device),
           "steps": torch.full((view.n_cf, 8), -99, dtype=torch.int32, device=enc.device)}
    g["rate_dev"] = enc.rate_curve(view, flags, cap_bps, out=out)
    g["rate_host"] = {k: g["rate_dev"][k].cpu().numpy() for k in ("worst", "bits", "steps")}
    g["rate_host"]["row"], g["rate_host"]["sub_stride"] = g["rate_dev"]["row"], g["rate_dev"]["sub_stride"]
    _RATE[key] = g
    return g


def body_of(g, out):
    body, total = g["enc"].gather_body(out["payload"], out["n_bytes"])
    return g["head"] + body[:int(total.item())].cpu().numpy().tobytes()


@pytest.mark.parametrize("ns,nm_bits,cap", wc.RATE_CASES)
def test_rate_curve_and_solve(A, ns, nm_bits, cap):
    a, model = wc.rate_analysis(ns, nm_bits), wc.rate_curve(ns, nm_bits, cap)
    g = rate_setup(A, ns, nm_bits, cap)
    compare_rate_curve(f"{ns}/{nm_bits} cap {cap}", a, cap, model, g["rate_host"], g["flags"])
    host = g["rate_host"]
    small, big = am.total(host, 30 * GRID), am.total(host, -30 * GRID)
    sol, _ = check_rate_solve(A, g["enc"], g["rate_dev"], host, (small + big) // 2, -30, 30, "reachable")
    assert sol["met"]
    sol, _ = check_rate_solve(A, g["enc"], g["rate_dev"], host, small - 1, -30, 30, "unreachable")
    assert not sol["met"] and sol["target_nmr_db"] == 30.0 and sol["total_bytes"] == small


@pytest.mark.parametrize("target", wc.NMR_TARGETS)
@pytest.mark.parametrize("ns,nm_bits,cap", wc.RATE_CASES)
def test_budget_search_equals_the_models(A, ns, nm_bits, cap, target):
    pcm, _ = wc.stream()
    a = wc.rate_analysis(ns, nm_bits)
    budget, capped, margin, live = wc.rate_search(ns, nm_bits, cap, target)
    assert margin[live].min() >= WINDOW                          # no unit inside the tie window: none is left out
    g = rate_setup(A, ns, nm_bits, cap)
    out = g["enc"].encode_pack_nmr(g["view"], g["flags"], target, g["cap_bps"])
    got = out["budget"].cpu().numpy().reshape(budget.shape)
    assert np.array_equal(got[live], budget[live]) and not got[~live].any()
    got_cap = (out["status"].cpu().numpy().reshape(-1, 2) & A._lib.ST_RATE_CAP) != 0
    assert np.array_equal(got_cap, capped.any(axis=2))
    data = body_of(g, out)
    assert data == rm.encode(a, budget, len(pcm))
    check_stream(A, data, out["n_bytes"].cpu().numpy(), (ns, nm_bits, cap, target))
    if cap == 48:
        assert capped.sum() > 0.5 * live.sum()


@pytest.mark.parametrize("ns,nm_bits,cap", wc.RATE_CASES)
def test_band_curve_pick_and_second_pass(A, ns, nm_bits, cap):
    pcm, sr = wc.stream()
    a, model = wc.rate_analysis(ns, nm_bits), wc.band_curve(ns, nm_bits, cap)
    g = rate_setup(A, ns, nm_bits, cap)
    what = f"{ns}/{nm_bits} cap {cap}"
    assert model["n_cand"] == min(1 << nm_bits, 16)
    compare_curve(model, g, what)
    for target in wc.NMR_TARGETS:
        pick, ref, near = compare_pick(A, model, g, target, f"{what} {target:+.0f} dB")
        assert not near.any(), what                              # tests/test_oracle_widths.py: the margins
        assert pick["bit_alloc"].max() <= model["n_cand"]
        if cap == 48:
            assert (ref[5] & (model["cap"] >= 0)).any()          # units over their cap take cap_alloc
        out = g["enc"].encode_pack_alloc(g["view"], g["flags"], np.ascontiguousarray(pick["bit_alloc"]))
        data = body_of(g, out)
        assert data == bm.encode(a, pick["bit_alloc"], len(pcm)), (what, target)
        assert np.array_equal(out["n_bytes"].cpu().numpy(), pick["n_bytes"]), (what, target)
        assert np.array_equal(out["bit_alloc"].cpu().numpy(), pick["bit_alloc"]), (what, target)
        check_stream(A, data, pick["n_bytes"], (what, target))
        rep = A.quality.nmr_of_file(pcm, data)
        assert closed_loop(a, rep, pick["capped"].reshape(-1, 2), target, what) > 0 or cap == 48
    # an allocation above maxMantBits is coded at maxMantBits
    alloc = np.full(model["cap_alloc"].shape, 99, np.int32)
    out = g["enc"].encode_pack_alloc(g["view"], g["flags"], alloc)
    unit, _ = bm.layout(model)
    assert (out["bit_alloc"].cpu().numpy()[unit >= 0] == model["n_cand"]).all()
    assert body_of(g, out) == bm.encode(a, alloc, len(pcm)), what


@pytest.mark.parametrize("ns,nm_bits,cap", wc.RATE_CASES)
def test_band_solve_profile_and_segments(A, ns, nm_bits, cap):
    model = wc.band_curve(ns, nm_bits, cap)
    g = rate_setup(A, ns, nm_bits, cap)
    enc, what = g["enc"], f"{ns}/{nm_bits} cap {cap}"
    own = bm.with_arrays(model, **g["host"])
    t_lo, t_hi = -30 * GRID, 30 * GRID
    prof = enc.band_profile(g["dev"], -30, 30).cpu().numpy()
    want = pm.profile(own, t_lo, t_hi)
    assert np.array_equal(prof, want), what
    assert np.array_equal(prof[::331], [bm.total(own, t) for t in range(t_lo, t_hi + 1, 331)]), what
    small = int(prof[-1])
    for limit, met in (((small + int(prof[0])) // 2, True), (small - 1, False)):
        sol, ref = check_solve(g, model, limit, -30, 30, f"{what} limit {limit}")
        assert bool(sol["met"]) == met and sol["bit_alloc"].cpu().numpy().max() <= model["n_cand"]
        ps = enc.profile_solve(enc.band_profile(g["dev"], -30, 30), limit, -30, 30)
        assert (ps["target_nmr_db"], ps["met"], ps["total_bytes"]) == (sol["target_nmr_db"], sol["met"], sol["total_bytes"])
    n_cf = len(model["cap"])
    rows = enc.band_profile_segments(g["dev"], 3 * 2, 0, -30, 30).cpu().numpy()
    first = sm.uniform_first(n_cf, 3 * 2, 0)
    assert len(first) == 4 and np.array_equal(rows, sm.rows(own, first, t_lo, t_hi)), what
    assert np.array_equal(rows.sum(axis=0), prof), what


# ------------------------------------------------------------------------- 5. the gain-shape band curve at 4 / 3
@functools.lru_cache(maxsize=None)
def vq_case():
    """(pcm, sr, analysis, the fixture's curve as a band_model dict) of the first two hops at 4 / 3"""
    g = wc.fixture()
    pcm, sr = wc.stream()
    pcm = np.ascontiguousarray(pcm[:wc.VQ_CURVE["hops"] * 1024])
    a = rm.analysis(pcm, sr, True, *wc.VQ_CURVE["widths"])
    c = bm.tables(a["p"])
    c["nmr"], c["cap"], c["cap_alloc"], c["written"] = (g["vqcurve_" + k] for k in ("nmr", "cap", "cap_alloc", "written"))
    return pcm, sr, a, c


def test_vq_band_curve_and_second_pass(A):
    from audio_codec_amd.audiofile import CodingParams
    pcm, sr, a, F = vq_case()
    ns, nm_bits = wc.VQ_CURVE["widths"]
    cap_bps = wc.VQ_CURVE["cap_kbps"] / (sr / 1000)
    enc = A.context.encoder(sr, cap_bps, ns, nm_bits, use_vq=True)
    sib = A.context.scalar_sibling(enc)
    assert (sib.n_scale_bits, sib.n_mant_size_bits, sib.use_vq) == (ns, nm_bits, False)
    planar = A.pacfile.device_stream(enc, pcm)
    view = A.engine.PcmView.stream(planar, 1024)
    flags = enc.transient_flags(planar, len(pcm) // 1024)[1]
    assert flags.cpu().numpy().tolist() == [l * 1 + c * 2 + n * 4 for (l, c, n) in a["flags"]]
    dev = enc.vq_band_curve(view, flags, cap_bps)
    host = {k: dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")}
    unit, _ = bm.layout(F)
    live = unit >= 0
    assert F["n_cand"] == 8 and np.array_equal(host["cap"], F["cap"])
    for test in (np.isposinf, np.isneginf, np.isnan, np.isfinite):
        assert np.array_equal(test(host["nmr"]), test(F["nmr"])), test.__name__
    assert np.isposinf(host["nmr"][live][:, 8:]).all() and not np.isposinf(host["nmr"][live][:, :8]).any()
    fin = np.isfinite(F["nmr"])
    err = np.abs(host["nmr"][fin] - F["nmr"][fin]).max()
    print(f"gain-shape curve at {ns}/{nm_bits}: {int(live.sum())} bands, {int(fin.sum())} finite entries, "
          f"max |nmr - model| {err:.3g} dB")
    assert err <= 1e-5
    assert np.array_equal(host["cap_alloc"], F["cap_alloc"])
    cp = CodingParams()
    cp.sampleRate, cp.nChannels, cp.numSamples = sr, 2, len(pcm)
    cp.nMDCTLines = cp.nSamplesPerBlock = 1024
    cp.nScaleBits, cp.nMantSizeBits = ns, nm_bits
    cp.targetBitsPerSample = cap_bps
    cp.useSBR, cp.useVQ = False, True
    head = A.pacfile.header_bytes(cp)
    for target in wc.NMR_TARGETS:
        t = int(target * GRID)
        margin = bm.margins(F, target)
        assert margin[F["cap"] >= 0].min() >= WINDOW, target         # no unit inside the tie window
        pick = {k: v.cpu().numpy() for k, v in sib.band_pick(dev, target).items()}
        for ref in (bm.evaluate(bm.with_arrays(F, **host), t), bm.evaluate(F, t)):
            assert np.array_equal(pick["bit_alloc"], ref[1]) and np.array_equal(pick["n_bytes"], ref[2])
            assert np.array_equal(pick["capped"], ref[3])
        out = enc.encode_vq_alloc(view, flags, np.ascontiguousarray(pick["bit_alloc"]))
        data, final, n_bytes = vm.encode_stream_alloc(a, pick["bit_alloc"], len(pcm))
        assert np.array_equal(out["n_bytes"].cpu().numpy(), n_bytes)
        assert np.array_equal(out["n_bytes"].cpu().numpy(), pick["n_bytes"])
        body, total = enc.gather_body(out["payload"], out["n_bytes"])
        assert head + body[:int(total.item())].cpu().numpy().tobytes() == data, target
        assert np.array_equal(out["bit_alloc"].cpu().numpy(), final)
        assert np.array_equal(A.pacfile.decode_stream(data), pv.decode_stream_vq(data)), target
