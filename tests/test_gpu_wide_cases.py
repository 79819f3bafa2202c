"""4 to 8 channels and sample rates above 96 kHz on the GPU, through every entry point: the stream coders and decoders at
the ten cases of tests/wide_cases.py against what the oracle wrote and decoded (tests/golden/wide.part*.npz), and rate
control at four of them against the NumPy models, which tests/test_wide_cases.py holds to the oracle at these shapes.

What is new at these shapes: k_transient's strided body (more than two channels), the sibling loop of k_mdct_short over
up to eight channels, n_ch list entries per frame in k_frame_lists*, band layouts of 15 / 13 / 9 long and 5 / 4 / 2
short bands that stop short of the last line (the dummy band), and at 176.4 and 192 kHz a band_stride that comes from
the short layout, 16 slots of which a long block uses 9.

Bars.  Section 1: bytes, int16 PCM, codes, flags, record offsets: equal, no tolerance.  A stream that differs from the
oracle's is taken apart by the parity soak's classifiers (tests/soak_parity.py); a block they cannot put down to the
reference's own rounding noise fails the test, and so does a second stream of the forty that needs them at all.
Section 2: integers, bytes, picks and profiles equal; finite band-curve entries and the rate curve's worst within 1e-5
dB of the model (tests/test_gpu_band.compare_curve, tests/test_gpu_abr.compare_curve); budgets and allocations equal
outside the tie window of 1e-4 dB -- and tests/test_wide_cases.py asserts that no unit of these cases lies inside it at
the targets used, so none is left out (asserted again here).
"""
import functools

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import kept_model as km
import nmr_model as nm
import profile_model as pm
import rate_model as rm
import rate_profile_model as rp
import seg_profile_model as sm
import vq_band_model as vm
import wide_cases as wc
from oracle import pac_oracle_vq as pv
from test_gpu_abr import SENTINEL_B, SENTINEL_W
from test_gpu_abr import check_solve as check_rate_solve
from test_gpu_abr import compare_curve as compare_rate_curve
from test_gpu_band import check_solve, check_stream, compare_curve, compare_pick
from test_gpu_kept import BAND_OUT, RATE_OUT, check_band_thresholds, check_rate_thresholds, same
from test_gpu_nmr import compare as compare_nmr
from test_gpu_round3 import fresh_handles                                 # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

GRID = bm.GRID
SCALAR = [s for s in wc.STREAMS if not wc.CODERS[s[1]][2]]
SWITCHES = ("PACX_FUSE_FRONT", "PACX_FUSE_TAIL", "PACX_SPLIT_SHORT", "PACX_VQ_FRAME", "PACX_VQ_DEC_FRAME")
CLASSIFIED = []                     # streams that needed the soak's classifiers: at most one of the forty


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def kw_of(coder):
    kbps, bs, vq, sbr = wc.CODERS[coder]
    return dict(kbps_per_channel=kbps, block_switching=bs, use_vq=vq, use_sbr=sbr)


def gpu_encode(A, case, coder, **more):
    return A.pacfile.encode_stream(wc.material(case)[0], case[0], **kw_of(coder), **more)


def first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}, first difference at byte {at}"


def handle(A, case, coder):
    kbps, _, vq, sbr = wc.CODERS[coder]
    return A.context.encoder(case[0], kbps / (case[0] / 1000), 4, 12, use_vq=vq, use_sbr=sbr)


def stage_view(A, case, coder):
    """(encoder, view, flags or None, transient decisions) of the stream, as encode_stream makes them"""
    enc = handle(A, case, coder)
    planar = A.pacfile.device_stream(enc, wc.material(case)[0])
    tr, flags = enc.transient_flags(planar, wc.N_HOPS)
    return enc, A.engine.PcmView.stream(planar, 1024), (flags if wc.CODERS[coder][1] else None), tr


def expected_flags(case):
    return wc.block_flags([bool(v) for v in wc.fixture()["tr_" + wc.tag_of(case)]])


def classified(A, case, coder, got, want):
    """a stream that is not the oracle's: every differing block in a class of the soak, and no second such stream"""
    import soak_parity
    kbps, bs, vq, _ = wc.CODERS[coder]
    soak_case = dict(sr=case[0], n_ch=case[1], kbps=kbps, coder="vq" if vq else ("scalar_bs" if bs else "scalar"))
    classify = soak_parity.classify_vq_mismatch if vq else soak_parity.classify_scalar_mismatch
    classes = classify(A, soak_case, wc.material(case)[0], got, want)
    print(f"{wc.stream_id((case, coder))}: {first_difference(got, want)}; {classes}")
    assert classes and not any(c.startswith("REAL") for c in classes), (wc.stream_id((case, coder)), classes)
    if (case, coder) not in CLASSIFIED:
        CLASSIFIED.append((case, coder))
    assert len(CLASSIFIED) <= 1, [wc.stream_id(s) for s in CLASSIFIED]


# ------------------------------------------------------------------------- 1. coders and decoders, no tolerance
@pytest.mark.parametrize("stream", wc.STREAMS, ids=wc.stream_id)
def test_encode_stream_writes_the_oracles_bytes(A, stream):
    """one batch, and through HostStreamEncoder in chunks of two hops"""
    case, coder = stream
    want = wc.reference(case, coder)
    got = gpu_encode(A, case, coder)
    if got != want:
        classified(A, case, coder, got, want)
    chunked = gpu_encode(A, case, coder, chunk_hops=2)
    assert chunked == got, "chunk_hops=2: " + first_difference(chunked, got)


@pytest.mark.parametrize("stream", wc.STREAMS, ids=wc.stream_id)
def test_decode_stream_gives_the_oracles_pcm(A, stream):
    """whole and in chunks that hold two hops of longest records; above 48 kHz the SBR decoder has no output"""
    case, coder = stream
    data = wc.reference(case, coder)
    want, raised = wc.decoded(case, coder)
    chunk = 2 * case[1] * 2196
    if raised is not None:
        assert raised == "IndexError" and coder == "vqsbr" and case[0] > 48000
        with pytest.raises(RuntimeError, match="PACX_ST_VQ_UNDEFINED"):
            A.pacfile.decode_stream(data)
        with pytest.raises(RuntimeError, match="PACX_ST_VQ_UNDEFINED"):
            A.pacfile.decode_stream(data, chunk_bytes=chunk)
        return
    got = A.pacfile.decode_stream(data)
    assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)
    got = A.pacfile.decode_stream(data, chunk_bytes=chunk)
    assert got.shape == want.shape and np.array_equal(got, want), "in chunks"


@pytest.mark.parametrize("stream", wc.STREAMS, ids=wc.stream_id)
def test_index_body_equals_the_host_walk(A, stream):
    import torch
    case, coder = stream
    data = wc.reference(case, coder)
    cp, pos = A.pacfile.parse_header(data)
    assert cp.nChannels == case[1] and cp.sampleRate == case[0]
    enc = A.context.encoder_for_params(cp)
    offs, sizes = A.pacfile.record_chain(data, pos, enc.payload_stride)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(enc.device)
    got_offs, got_sizes, result = enc.index_body(dev[pos:], case[1])
    n = int(result[0])
    assert result.cpu().tolist() == [len(offs), len(data) - pos, -1] and n % case[1] == 0
    assert got_offs[:n].cpu().tolist() == [o - pos for o in offs] and got_sizes[:n].cpu().tolist() == sizes


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_transient_flags_and_dropped_hops(A, case):
    """the detector's decisions and the flag bytes are the oracle's; a dropped hop carries PACX_ST_ZERO_SUBBLOCK and
    n_bytes 0 in EVERY channel-frame, whichever channel holds the silent sub-block, and no other hop does"""
    n_ch = case[1]
    pcm, _ = wc.material(case)
    flags = expected_flags(case)
    drop = wc.dropped_blocks(pcm, [bool(f[2]) for f in flags[:wc.N_HOPS]])
    assert drop and any(chs - {0} for chs in drop.values())
    for coder in ("bs", "vq", "vqsbr"):
        enc, view, fl, tr = stage_view(A, case, coder)
        assert tr.cpu().numpy().tolist() == wc.fixture()["tr_" + wc.tag_of(case)].tolist(), coder
        assert fl.cpu().numpy().tolist() == [l * 1 + c * 2 + n * 4 for (l, c, n) in flags], coder
        out = enc.encode_vq(view, fl) if wc.CODERS[coder][2] else enc.encode_pack(view, fl)
        status = out["status"].cpu().numpy().reshape(wc.N_BLOCKS, n_ch)
        n_bytes = out["n_bytes"].cpu().numpy().reshape(wc.N_BLOCKS, n_ch)
        zero = (status & A._lib.ST_ZERO_SUBBLOCK) != 0
        for f in range(wc.N_BLOCKS):
            assert zero[f].all() == zero[f].any() == (f in drop), (coder, f, status[f].tolist())
            assert (n_bytes[f] == 0).all() == (n_bytes[f] == 0).any() == (f in drop), (coder, f, n_bytes[f].tolist())
    enc, view, fl, _ = stage_view(A, case, "long")                        # without flags nothing is dropped
    out = enc.encode_pack(view, fl)
    assert fl is None and (out["n_bytes"].cpu().numpy() > 0).all()
    assert not (out["status"].cpu().numpy() & A._lib.ST_ZERO_SUBBLOCK).any()


@pytest.mark.parametrize("stream", SCALAR, ids=wc.stream_id)
def test_encode_equals_the_oracle_stage_by_stage(A, stream):
    """Encoder.encode unpacked against the units of the oracle's file: a mismatch names the block, the channel, the
    unit, the stage and the band"""
    case, coder = stream
    n_ch = case[1]
    enc, view, flags, _ = stage_view(A, case, coder)
    out = enc.encode(view, flags)
    host = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    want_flags = expected_flags(case) if flags is not None else [(0, 0, 0)] * wc.N_BLOCKS
    assert view.n_frames == wc.N_BLOCKS and len(host["status"]) == wc.N_BLOCKS * n_ch
    records = wc.scalar_units(wc.reference(case, coder))
    kept = [f for f in range(wc.N_BLOCKS)
            if not (host["status"][f * n_ch:(f + 1) * n_ch] & A._lib.ST_ZERO_SUBBLOCK).any()]
    assert len(records) == len(kept) * n_ch, (len(records), kept)
    bad_status = A._lib.ST_VQ_UNDEFINED | A._lib.ST_MALFORMED | A._lib.ST_REF_RAISES
    n_units = 0
    for r, (fl, units) in enumerate(records):
        f, ch = kept[r // n_ch], r % n_ch
        i = f * n_ch + ch
        assert fl == tuple(int(v) for v in want_flags[f]), (f, fl)
        assert not host["status"][i] & bad_status, (f, ch, host["status"][i])
        for sb, (overall, alloc, sf, mant) in enumerate(units):
            got = A.codec.unpack_short(enc, host, i, sb) if fl[1] else A.codec.unpack_long(enc, host, i)
            where = f"block {f} {fl} channel {ch} unit {sb}"
            assert got[3] == overall, f"{where}: overall scale {got[3]} against {overall}"
            for name, g_, w_ in (("allocation", got[1], alloc), ("scale factor", got[0], sf)):
                bad = np.nonzero(np.asarray(g_) != np.asarray(w_))[0]
                assert not len(bad), f"{where}: {name} of band {bad[0]}: {g_[bad[0]]} against {w_[bad[0]]}"
            bad = np.nonzero(got[2] != mant)[0] if len(got[2]) == len(mant) else [0]
            assert len(got[2]) == len(mant) and not len(bad), f"{where}: mantissa {bad[0]} of the coded lines"
            n_units += 1
    assert n_units >= len(records)


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_path_switches_change_nothing(A, monkeypatch, fresh_handles, case):
    """every kernel route that another input would take by default: the bytes and the PCM stay"""
    want = {coder: gpu_encode(A, case, coder) for coder in wc.CODERS}
    pcm = {coder: A.pacfile.decode_stream(data) for coder, data in want.items() if wc.decoded(case, coder)[1] is None}
    for name in SWITCHES:
        for k in SWITCHES + ("PACX_VQ_BFS", "PACX_VQ_FUSE_ALLOC"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv(name, "0")
        A.context.clear()                              # the overrides are read when a handle is created
        for coder in wc.CODERS:
            got = gpu_encode(A, case, coder)
            assert got == want[coder], (name, coder, first_difference(got, want[coder]))
            if coder in pcm:
                assert np.array_equal(A.pacfile.decode_stream(want[coder]), pcm[coder]), (name, coder)
                assert np.array_equal(A.pacfile.decode_stream(want[coder], chunk_bytes=2 * case[1] * 2196),
                                      pcm[coder]), (name, coder, "in chunks")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    A.context.clear()


def test_nine_channels_are_refused(A):
    rng = np.random.default_rng(9)
    pcm = rng.integers(-3000, 3001, (2 * 1024, 9)).astype(np.int16)
    with pytest.raises(A._lib.PacxError, match="at most 8 channels"):
        A.pacfile.encode_stream(pcm, 48000, 128, block_switching=True)


def test_zz_at_most_one_stream_needed_a_classifier():
    print(f"streams taken apart by the soak's classifiers: {[wc.stream_id(s) for s in CLASSIFIED]}")
    assert len(CLASSIFIED) <= 1


# ------------------------------------------------------------------------- 2. rate control at these shapes
_RATE = {}


def rate_setup(A, case):
    """the handle, view and flags of the block-switched stream with the cap rate as the handle's, the band curve and the
    rate curve of the GPU: once per case"""
    import torch
    if case in _RATE:
        return _RATE[case]
    pcm, _ = wc.material(case)
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, case[0], wc.CAP_KBPS, True, None)
    cap_bps = cp.targetBitsPerSample
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
    _RATE[case] = g
    return g


def body_of(g, out):
    body, total = g["enc"].gather_body(out["payload"], out["n_bytes"])
    return g["head"] + body[:int(total.item())].cpu().numpy().tobytes()


def layout_of(case):
    nbl, _, nbs, _ = wc.BANDS[case[0]]
    return nbl, nbs, max(nbl, wc.SUB * nbs)


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_nmr_report_against_the_model(A, case):
    pcm, _ = wc.material(case)
    data, rep = A.quality.encode_stream_report(pcm, case[0], 128, block_switching=True)
    assert data == gpu_encode(A, case, "bs")
    m = nm.model(pcm, data, True)
    nbl, nbs, stride = layout_of(case)
    assert m["nmr_db"].shape == (wc.N_BLOCKS, case[1], stride) and (np.array(m["record"]) < 0).any()
    compare_nmr(rep, m, 2e-12, 0.0, wc.tag_of(case))
    if case[0] >= 176400:                                   # a long block leaves the slots beyond its 9 bands unused
        long_blocks = [f for f, r in enumerate(m["record"]) if r >= 0 and not m["short"][f]]
        assert long_blocks and np.isnan(rep.nmr_db[long_blocks][:, :, nbl:]).all()
        assert not np.isnan(rep.nmr_db[long_blocks][:, :, :nbl]).any()


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_rate_curve_and_solve(A, case):
    a, model = wc.rate_analysis(case), wc.rate_curve(case)
    g = rate_setup(A, case)
    compare_rate_curve(wc.tag_of(case), a, wc.CAP_KBPS, model, g["rate_host"], g["flags"])
    host = g["rate_host"]
    small, big = am.total(host, 30 * GRID), am.total(host, -30 * GRID)
    sol, _ = check_rate_solve(A, g["enc"], g["rate_dev"], host, (small + big) // 2, -30, 30, "reachable")
    assert sol["met"]
    sol, _ = check_rate_solve(A, g["enc"], g["rate_dev"], host, small - 1, -30, 30, "unreachable")
    assert not sol["met"] and sol["target_nmr_db"] == 30.0 and sol["total_bytes"] == small


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_budget_search_equals_the_models(A, case):
    """encode_pack_nmr at -3 dB"""
    pcm, _ = wc.material(case)
    a = wc.rate_analysis(case)
    budget, capped, margin = (wc.stored(case, "search_" + k) for k in ("budget", "capped", "margin"))
    live = np.isfinite(margin)
    assert margin[live].min() >= wc.WINDOW                       # no unit inside the tie window: none is left out
    g = rate_setup(A, case)
    out = g["enc"].encode_pack_nmr(g["view"], g["flags"], wc.TARGETS[0], g["cap_bps"])
    got = out["budget"].cpu().numpy().reshape(budget.shape)
    assert np.array_equal(got[live], budget[live]) and not got[~live].any()
    got_cap = (out["status"].cpu().numpy().reshape(-1, case[1]) & A._lib.ST_RATE_CAP) != 0
    assert np.array_equal(got_cap, capped.any(axis=2))
    data = body_of(g, out)
    assert data == rm.encode(a, budget, len(pcm))
    check_stream(A, data, out["n_bytes"].cpu().numpy(), wc.tag_of(case))


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_band_curve_pick_and_second_pass(A, case):
    pcm, _ = wc.material(case)
    a, model = wc.rate_analysis(case), wc.band_curve(case)
    g = rate_setup(A, case)
    what = wc.tag_of(case)
    nbl, nbs, stride = layout_of(case)
    assert g["enc"].band_stride == stride == model["band_stride"] and g["host"]["nmr"].shape[1] == stride
    compare_curve(model, g, what)
    for target in wc.TARGETS:
        pick, ref, near = compare_pick(A, model, g, target, f"{what} {target:+.0f} dB")
        assert not near.any(), what                              # tests/test_wide_cases.py: the margins
        out = g["enc"].encode_pack_alloc(g["view"], g["flags"], np.ascontiguousarray(pick["bit_alloc"]))
        data = body_of(g, out)
        assert data == bm.encode(a, pick["bit_alloc"], len(pcm)), (what, target)
        assert np.array_equal(out["n_bytes"].cpu().numpy(), pick["n_bytes"]), (what, target)
        assert np.array_equal(out["bit_alloc"].cpu().numpy(), pick["bit_alloc"]), (what, target)
        check_stream(A, data, pick["n_bytes"], (what, target))
    own = bm.with_arrays(model, **g["host"])
    small, big = bm.total(own, 30 * GRID), bm.total(own, -30 * GRID)
    for limit, met in (((small + big) // 2, True), (small - 1, False)):
        sol, _ = check_solve(g, model, limit, -30, 30, f"{what} limit {limit}")
        assert bool(sol["met"]) == met


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_profiles_and_segment_rows(A, case):
    """band_profile, rate_profile over +-30 dB and band_profile_segments with one hop per segment, on the GPU's own
    curves: integers, every entry equal"""
    model = wc.band_curve(case)
    g = rate_setup(A, case)
    enc, what, n_ch = g["enc"], wc.tag_of(case), case[1]
    own = bm.with_arrays(model, **g["host"])
    t_lo, t_hi = -30 * GRID, 30 * GRID
    prof = enc.band_profile(g["dev"], -30, 30).cpu().numpy()
    assert np.array_equal(prof, pm.profile(own, t_lo, t_hi)), what
    assert np.array_equal(prof[::331], [bm.total(own, t) for t in range(t_lo, t_hi + 1, 331)]), what
    n_cf = len(model["cap"])
    rows = enc.band_profile_segments(g["dev"], n_ch, 0, -30, 30).cpu().numpy()
    first = sm.uniform_first(n_cf, n_ch, 0)
    assert len(first) == wc.N_BLOCKS + 1 and np.array_equal(rows, sm.rows(own, first, t_lo, t_hi)), what
    assert np.array_equal(rows.sum(axis=0), prof) and (rows.sum(axis=1) == 0).any(), what      # a dropped hop's row
    host = g["rate_host"]
    rprof = enc.rate_profile(g["rate_dev"], -30, 30).cpu().numpy()
    assert np.array_equal(rprof, rp.profile_steps(host, t_lo, t_hi)), what
    assert np.array_equal(rprof[::331], [am.total(host, t) for t in range(t_lo, t_hi + 1, 331)]), what
    rrows = enc.rate_profile_segments(g["rate_dev"], n_ch, 0, -30, 30).cpu().numpy()
    assert np.array_equal(rrows, rp.rows(host, first, t_lo, t_hi)) and np.array_equal(rrows.sum(axis=0), rprof), what


@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_kept_thresholds_and_picks(A, case):
    """band_thresholds / rate_thresholds of the GPU's own curves into outputs filled with 0xFF, and the picks on them,
    against tests/kept_model.py"""
    model = wc.band_curve(case)
    g = rate_setup(A, case)
    enc, what = g["enc"], wc.tag_of(case)
    own = bm.with_arrays(model, **g["host"])
    t_lo, t_hi = -30 * GRID, 30 * GRID
    nbl, nbs, stride = layout_of(case)
    bkept = check_band_thresholds(enc, own, t_lo, t_hi)
    assert sum(bkept[k].numel() * bkept[k].element_size() for k in ("e", "cap", "cap_alloc")) == \
        len(own["cap"]) * km.band_bytes_per_cf(stride)
    rkept = check_rate_thresholds(enc, g["rate_host"], t_lo, t_hi)
    kb, kr = km.band_thresholds(own, t_lo, t_hi), km.rate_thresholds(g["rate_host"], t_lo, t_hi)
    for target in wc.TARGETS + (-30.0, 30.0, 0.078125):
        t = int(target * GRID)
        got = enc.band_pick_thresholds(bkept, target)
        same(got, km.band_pick(kb, t), BAND_OUT, (what, target))
        same(got, enc.band_pick(g["dev"], target), BAND_OUT, (what, target))
        got = enc.rate_pick_thresholds(rkept, target)
        same(got, km.rate_pick(kr, t), RATE_OUT, (what, target))
        same(got, enc.rate_pick(g["rate_dev"], target), RATE_OUT, (what, target))


@functools.lru_cache(maxsize=None)
def abr_streams(A, case, allocation):
    """(the one-batch stream, its size in kb/s per channel) at a size half way between the totals of +30 and -30 dB"""
    g = rate_setup(A, case)
    if allocation == "band":
        own = bm.with_arrays(wc.band_curve(case), **g["host"])
        small, big = bm.total(own, 30 * GRID), bm.total(own, -30 * GRID)
    else:
        small, big = am.total(g["rate_host"], 30 * GRID), am.total(g["rate_host"], -30 * GRID)
    max_bytes = len(g["head"]) + (small + big) // 2
    data = A.pacfile.encode_stream_abr(wc.material(case)[0], case[0], max_bytes=max_bytes, block_switching=True,
                                       max_kbps_per_channel=wc.CAP_KBPS, allocation=allocation)
    assert len(g["head"]) + small < len(data) <= max_bytes
    return data, max_bytes


@pytest.mark.parametrize("allocation", ["band", "budget"])
@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_average_rate_streams_agree(A, case, allocation):
    """encode_stream_abr_kept = encode_stream_abr_chunked = encode_stream_abr, in chunks of two hops"""
    pcm, _ = wc.material(case)
    want, max_bytes = abr_streams(A, case, allocation)
    kw = dict(max_bytes=max_bytes, chunk_hops=2, max_kbps_per_channel=wc.CAP_KBPS, block_switching=True,
              allocation=allocation)
    got = A.pacfile.encode_stream_abr_chunked(pcm, case[0], **kw)
    assert got == want, "chunked: " + first_difference(got, want)
    got = A.pacfile.encode_stream_abr_kept(pcm, case[0], **kw)
    assert got == want, "kept: " + first_difference(got, want)
    check_stream(A, want, None, (wc.tag_of(case), allocation))


@pytest.mark.parametrize("case", wc.RATE_CONTROL[:1], ids=wc.case_id)
def test_average_rate_per_segment_streams_agree(A, case):
    """segments of three blocks, chunks of two: every chunk boundary but one falls inside a segment"""
    pcm, _ = wc.material(case)
    kw = dict(kbps_per_channel=96, max_kbps_per_channel=wc.CAP_KBPS, block_switching=True, allocation="band",
              segment_hops=3)
    want = A.pacfile.encode_stream_abr(pcm, case[0], **kw)
    got = A.pacfile.encode_stream_abr_chunked(pcm, case[0], chunk_hops=2, **kw)
    assert got == want, "chunked: " + first_difference(got, want)
    got = A.pacfile.encode_stream_abr_kept(pcm, case[0], chunk_hops=2, **kw)
    assert got == want, "kept: " + first_difference(got, want)
    check_stream(A, want, None, wc.tag_of(case))


# ------------------------------------------------------------------------- 3. the gain-shape band curve, two hops
@pytest.mark.parametrize("case", wc.RATE_CONTROL, ids=wc.case_id)
def test_vq_band_curve_pick_and_second_pass(A, case):
    pcm = np.ascontiguousarray(wc.material(case)[0][:wc.VQ_HOPS * 1024])
    sr, n_ch = case[:2]
    a, F = wc.vq_analysis(case), wc.vq_curve(case)
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, wc.CAP_KBPS, True, None, use_vq=True)
    sib = A.context.scalar_sibling(enc)
    assert flags.cpu().numpy().tolist() == [l * 1 + c * 2 + n * 4 for (l, c, n) in a["flags"]]
    dev = enc.vq_band_curve(view, flags, cp.targetBitsPerSample)
    host = {k: dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")}
    unit, _ = bm.layout(F)
    live = unit >= 0
    assert live.any() and host["nmr"].shape == F["nmr"].shape and np.array_equal(host["cap"], F["cap"])
    for test in (np.isposinf, np.isneginf, np.isnan, np.isfinite):
        assert np.array_equal(test(host["nmr"]), test(F["nmr"])), test.__name__
    fin = np.isfinite(F["nmr"])
    err = np.abs(host["nmr"][fin] - F["nmr"][fin]).max()
    print(f"gain-shape curve of {wc.tag_of(case)}: {int(live.sum())} bands, {int(fin.sum())} finite entries, "
          f"max |nmr - model| {err:.3g} dB")
    assert err <= 1e-5
    assert np.array_equal(host["cap_alloc"], F["cap_alloc"])
    head = A.pacfile.header_bytes(cp)
    for target in wc.TARGETS:
        t = int(target * GRID)
        assert bm.margins(F, target)[F["cap"] >= 0].min() >= wc.WINDOW, target        # no unit inside the tie window
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
