"""An average for the stream and a peak for every segment on the GPU (pacx_rate_solve_peak / pacx_band_solve_peak,
Encoder.rate_solve_peak / band_solve_peak, the peak_kbps_per_channel keyword of pacfile.encode_stream_abr and
quality.encode_stream_to_rate) against tests/peak_model.py, which states the definition over segment_model and the
plain models.

Bars.  The solve is integers and comparisons on given arrays, so every output equals the model's: floor, t, met, total
per segment; t*, met*, total* of the stream; bit_alloc / budget, n_bytes, capped per channel-frame.  No window anywhere.
A stream's segment is, record for record, the stream of encode_stream_nmr at that segment's target.
"""
import ctypes
import functools

import numpy as np
import pytest

import band_model as bm
import peak_model as pm
import segment_model as sm
from oracle import pac_oracle as po
from test_gpu_segments import EDGES, on_device, excerpt, records_of        # stateless helpers only

pytestmark = pytest.mark.gpu

KINDS = ("band", "rate")
HUGE = 10 ** 12


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


# ------------------------------------------------------------------------------------------------------ helpers
_ENC = {}
_OWN = {}


def encoder(A, kind):
    """a handle whose band tables are the synthetic curves' (band_model.synthetic: 44100 Hz), one per kind, kept by this
    module alone"""
    if kind not in _ENC:
        _ENC[kind] = A.engine.Encoder(44100, 128 / 44.1)
    return _ENC[kind]


def own_curves(A, name):
    """an excerpt's handle, view and flags, and for both kinds the device curve and the model's view of its arrays,
    kept by this module alone: the handle is the package's cached one, which other test modules close and make anew"""
    if name not in _OWN:
        pcm, sr = excerpt(name)
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
        band = enc.band_curve(view, flags, cp.targetBitsPerSample)
        rate = enc.rate_curve(view, flags, cp.targetBitsPerSample)
        tables = bm.tables(po.make_params(sr, pcm.shape[1], 320))
        host = {"band": bm.with_arrays(tables, *(band[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc"))),
                "rate": dict({k: rate[k].cpu().numpy() for k in ("worst", "bits", "steps")}, row=rate["row"],
                             sub_stride=rate["sub_stride"])}
        _OWN[name] = {"pcm": pcm, "sr": sr, "cp": cp, "enc": enc, "view": view, "flags": flags,
                      "dev": {"band": band, "rate": rate}, "host": host}
    return _OWN[name]


def gpu_peak(enc, kind, dev, first, peaks, limit, lo_db=-30, hi_db=30):
    fn = enc.band_solve_peak if kind == "band" else enc.rate_solve_peak
    return fn(dev, first, peaks, limit, lo_db, hi_db)


def grid(v):
    return np.round(np.asarray(v) * 64).astype(np.int64)


def check(enc, kind, dev, c, first, peaks, limit, lo_db=-30, hi_db=30, what="", u=None):
    """the peak solve against the model on the same arrays: everything equal"""
    sol = gpu_peak(enc, kind, dev, first, peaks, limit, lo_db, hi_db)
    ref = pm.solve_peak(kind, c, first, peaks, limit, int(lo_db * 64), int(hi_db * 64), u)
    assert sol["target_nmr_db"].dtype == np.float64 and sol["floor_nmr_db"].dtype == np.float64
    assert sol["met"].dtype == bool and sol["pinned"].dtype == bool and sol["total_bytes"].dtype == np.int64
    assert isinstance(sol["stream_target_nmr_db"], float) and isinstance(sol["stream_met"], bool) and \
        isinstance(sol["stream_total_bytes"], int)
    got = (int(grid(sol["stream_target_nmr_db"])), int(sol["stream_met"]), sol["stream_total_bytes"])
    want = (ref["t_stream"], ref["met_stream"], ref["total_stream"])
    t, u_gpu = grid(sol["target_nmr_db"]), grid(sol["floor_nmr_db"])
    bad = np.nonzero((t != ref["t"]) | (u_gpu != ref["floor"]) | (sol["met"] != (ref["met"] != 0)) |
                     (sol["total_bytes"] != ref["total"]))[0]
    print(f"{what} {kind}: stream gpu {got}, model {want}; {len(peaks)} segments, {int(sol['pinned'].sum())} pinned, "
          f"{int(sol['met'].sum())} met, {len(bad)} differ")
    for s in bad[:3]:
        print(f"  segment {s}: gpu {(u_gpu[s], t[s], sol['met'][s], sol['total_bytes'][s])}, model "
              f"{(ref['floor'][s], ref['t'][s], ref['met'][s], ref['total'][s])}")
    assert got == want and not len(bad), (what, kind)
    assert np.array_equal(sol["pinned"], ref["t"] > ref["t_stream"])
    for k in sm.PER_CF[kind]:
        assert np.array_equal(sol[k].cpu().numpy(), ref[k]), (what, kind, k)
    return sol, ref


@functools.lru_cache(maxsize=None)
def material(kind):
    """the shared pattern with its floors and the four stream limits of the model"""
    c, first, peaks = sm.material(kind)
    u = pm.floors(kind, c, first, peaks)
    return c, first, peaks, u, pm.stream_limits(kind, c, first, peaks, u=u)


def same_arrays(kind, got, want, what):
    for k in sm.PER_CF[kind]:
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), (what, k)


# ------------------------------------------------------------------ 1. synthetic curves against the model
@pytest.mark.parametrize("which", ["midpoint", "unreachable", "exact", "huge"])
@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_curves(A, kind, which):
    c, first, peaks, u, limits = material(kind)
    limit = limits[("midpoint", "unreachable", "exact", "huge").index(which)]
    enc = encoder(A, kind)
    sol, ref = check(enc, kind, on_device(enc, kind, c), c, first, peaks, limit, what=which, u=u)
    assert sol["stream_met"] == (which != "unreachable")
    if which == "midpoint":
        assert 0 < sol["pinned"].sum() < len(peaks) and -30 < sol["stream_target_nmr_db"] < 30


# ------------------------------------------------------------------ 2. the two reductions, on the same handle
@pytest.mark.parametrize("kind", KINDS)
def test_peaks_that_never_bind_give_the_plain_solve(A, kind):
    c, first, _, _, _ = material(kind)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    for limit in ((small + big) // 2, small - 1, small, HUGE):
        got = gpu_peak(enc, kind, dev, first, [HUGE] * (len(first) - 1), limit)
        one = enc.band_solve(dev, limit) if kind == "band" else enc.rate_solve(dev, None, limit)
        assert (got["stream_target_nmr_db"], got["stream_met"], got["stream_total_bytes"]) == \
            (one["target_nmr_db"], one["met"], one["total_bytes"]), limit
        assert (got["floor_nmr_db"] == -30.0).all() and not got["pinned"].any() and got["met"].all()
        assert (got["target_nmr_db"] == one["target_nmr_db"]).all() and got["total_bytes"].sum() == one["total_bytes"]
        same_arrays(kind, got, one, limit)


@pytest.mark.parametrize("kind", KINDS)
def test_a_limit_that_never_binds_gives_the_segmented_solve(A, kind):
    c, first, peaks, _, _ = material(kind)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    for part, limits in ((first, peaks), (EDGES, sm.limits_for(kind, c, EDGES))):
        got = gpu_peak(enc, kind, dev, part, limits, HUGE)
        seg = (enc.band_solve_segments if kind == "band" else enc.rate_solve_segments)(dev, part, limits)
        assert (got["stream_target_nmr_db"], got["stream_met"]) == (-30.0, True)
        assert got["stream_total_bytes"] == seg["total_bytes"].sum()
        for k in ("target_nmr_db", "met", "total_bytes"):
            assert np.array_equal(got[k], seg[k]), k
        assert np.array_equal(got["floor_nmr_db"], seg["target_nmr_db"])
        assert np.array_equal(got["pinned"], seg["target_nmr_db"] > -30.0)
        same_arrays(kind, got, seg, len(limits))


# ------------------------------------------------------------------ 3. edge shapes
@pytest.mark.parametrize("n_cf", [0, 1, 3, 4, 5, 255, 256, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_one_segment_at_the_workgroup_edges(A, kind, n_cf):
    """no, one and a few frames and one frame before, at and after the band pick's 4-frame and the rate pick's
    256-frame workgroup: the peak at the midpoint of the segment's sizes, the stream's limit below, at and above it"""
    c = sm.synthetic(kind, n_cf, 11)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    peak = (small + big) // 2
    for limit in sorted({(small + peak) // 2, peak, (peak + big) // 2, max(small - 1, 0), HUGE}):
        sol, _ = check(enc, kind, dev, c, [0, n_cf], [peak], limit, what=f"{n_cf} frames, limit {limit}")
    if n_cf == 0:
        assert (sol["stream_target_nmr_db"], sol["stream_met"], sol["stream_total_bytes"]) == (-30.0, True, 0)
        assert (sol["floor_nmr_db"][0], sol["met"][0], sol["total_bytes"][0]) == (-30.0, True, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_every_frame_its_own_segment(A, kind):
    """300 segments of one frame: more than one workgroup of the kernels that run a thread per segment, and no
    workgroup of a pick whose frames share a segment"""
    n = 300
    c = sm.synthetic(kind, n, 5)
    enc = encoder(A, kind)
    first = np.arange(n + 1, dtype=np.int64)
    peaks = sm.limits_for(kind, c, first)
    u = pm.floors(kind, c, first, peaks)
    sol, _ = check(enc, kind, on_device(enc, kind, c), c, first, peaks, pm.stream_limits(kind, c, first, peaks, u=u)[0],
                   what="300 of 1", u=u)
    assert 0 < sol["pinned"].sum() < n


@pytest.mark.parametrize("lo_db,hi_db", [(-8, 8)])
@pytest.mark.parametrize("kind", KINDS)
def test_another_range(A, kind, lo_db, hi_db):
    c, first, _, _, _ = material(kind)
    enc = encoder(A, kind)
    t_lo, t_hi = int(lo_db * 64), int(hi_db * 64)
    peaks = sm.limits_for(kind, c, first, t_lo, t_hi)
    u = pm.floors(kind, c, first, peaks, t_lo, t_hi)
    for limit in pm.stream_limits(kind, c, first, peaks, t_lo, t_hi, u=u)[:2]:
        check(enc, kind, on_device(enc, kind, c), c, first, peaks, limit, lo_db, hi_db, what=f"range {lo_db} .. {hi_db}", u=u)


# ------------------------------------------------------------------ 4. interleaved on one stream
@pytest.mark.parametrize("kind", KINDS)
def test_plain_peak_segmented_and_peak_solves_interleaved(A, kind):
    """a plain solve, a peak solve, a segmented one and a second peak solve with another partition and limit, queued
    on one handle and one stream through the C entry points and read back only after the fourth: they share the
    handle's states, the stream's state behind them and the segment table"""
    import torch
    c, first, peaks, u, limits = material(kind)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    n_cf = sm.n_cf_of(kind, c)
    edge_peaks = sm.limits_for(kind, c, EDGES)
    edge_u = pm.floors(kind, c, EDGES, edge_peaks)
    edge_limit = pm.stream_limits(kind, c, EDGES, edge_peaks, u=edge_u)[0]
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    plain_limit = small + (big - small) // 5
    gpu_peak(enc, kind, dev, first, peaks, limits[0])                # the handle's states are grown: no wait below
    ptr = A.engine._ptr
    arrays = [ptr(dev[k]) for k in (("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps"))]
    head = [] if kind == "band" else [int(dev["row"]), int(dev["sub_stride"])]
    width = enc.band_stride if kind == "band" else 8
    i64 = lambda v: np.ascontiguousarray(v, np.int64)                # noqa: E731
    keep = []

    def queue(suffix, seg_first=None, seg_limit=None, limit=None):
        n_seg = 1 if seg_first is None else len(seg_limit)
        out = [torch.zeros((n_cf, width), dtype=torch.int32, device=enc.device),
               torch.zeros((n_cf,), dtype=torch.int32, device=enc.device),
               torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device)]
        res = {k: torch.zeros(shape, dtype=torch.int32, device=enc.device)
               for k, shape in (("floor", (n_seg,)), ("result", (n_seg, 4)), ("stream", (1, 4)))}
        size = [] if seg_first is None else [ctypes.c_int64(n_seg), i64(seg_first), i64(seg_limit)]
        keep.extend(size[1:])
        size = [v if isinstance(v, ctypes.c_int64) else v.ctypes.data for v in size]
        if limit is not None:
            size.append(ctypes.c_int64(int(limit)))
        tail = [ptr(res["floor"]), ptr(res["result"]), ptr(res["stream"])] if suffix == "_peak" else [ptr(res["result"])]
        rc = getattr(enc.lib, f"pacx_{kind}_solve{suffix}")(
            enc.h, ctypes.c_int64(n_cf), *head, *arrays, *size, ctypes.c_double(-30.0), ctypes.c_double(30.0),
            *(ptr(t) for t in out), *tail, enc._stream())
        assert rc == 0, (suffix, enc.lib.pacx_last_error(enc.h))
        return out, res

    queued = [queue("", limit=plain_limit), queue("_peak", first, peaks, limits[0]), queue("_segments", EDGES, edge_peaks),
              queue("_peak", EDGES, edge_peaks, edge_limit)]
    torch.cuda.synchronize()

    def decode(t):
        r = t.cpu().numpy()
        return r[:, 0].astype(np.int64), r[:, 1].astype(np.int64), r[:, 2:].copy().view(np.int64)[:, 0]

    refs = [sm.solve_segments(kind, c, [0, n_cf], [plain_limit]), pm.solve_peak(kind, c, first, peaks, limits[0], u=u),
            sm.solve_segments(kind, c, EDGES, edge_peaks), pm.solve_peak(kind, c, EDGES, edge_peaks, edge_limit, u=edge_u)]
    assert refs[1]["t_stream"] != refs[3]["t_stream"]                # the two peak solves have answers of their own
    for i, ((out, res), ref) in enumerate(zip(queued, refs)):
        for g, k in zip(decode(res["result"]), ("t", "met", "total")):
            assert np.array_equal(g, ref[k]), (kind, i, k)
        if "floor" in ref:
            assert np.array_equal(res["floor"].cpu().numpy(), ref["floor"]), (kind, i)
            assert tuple(int(v[0]) for v in decode(res["stream"])) == \
                (ref["t_stream"], ref["met_stream"], ref["total_stream"]), (kind, i)
        for t, k in zip(out, sm.PER_CF[kind]):
            assert np.array_equal(t.cpu().numpy().astype(ref[k].dtype), ref[k]), (kind, i, k)


# ------------------------------------------------------------------ 5. the GPU's own curves
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["castanet", "harpsichord"])
def test_own_curves(A, name, kind):
    """segments of 8 blocks; the stream's limit is the whole-stream limit at 96 kb/s and every segment's peak the median
    of what the segments take under the plain solve at that limit: some segments bind, some do not"""
    g = own_curves(A, name)
    enc, view, flags, dev, host = g["enc"], g["view"], g["flags"], g["dev"][kind], g["host"][kind]
    n_ch, blocks, sr = g["cp"].nChannels, view.n_frames, g["sr"]
    allocation = "band" if kind == "band" else "budget"
    fb, count, _ = A.pacfile.segment_limits(96, n_ch, sr, blocks, 8)
    first = np.append(fb, blocks) * n_ch
    limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    one = enc.band_solve(dev, limit) if kind == "band" else enc.rate_solve(dev, None, limit)
    assert one["met"]
    nby = one["n_bytes"].cpu().numpy().astype(np.int64)
    per_seg = np.array([int(np.sum(nby[a:b][nby[a:b] > 0] + 4)) for a, b in zip(first, first[1:])])
    peak = int(np.median(per_seg))
    peaks = np.full(len(per_seg), peak, np.int64)
    sol, ref = check(enc, kind, dev, host, first, peaks, limit, what=name)
    pinned = sol["pinned"]
    print(f"{name} {kind}: plain {one['target_nmr_db']} dB, bytes {per_seg.tolist()}, peak {peak}; stream "
          f"{sol['stream_target_nmr_db']} dB, targets {sol['target_nmr_db'].tolist()}, bytes "
          f"{sol['total_bytes'].tolist()}, met {sol['met'].tolist()}")
    assert pinned.any() and not pinned.all()                        # some segments bind and some do not
    assert (sol["target_nmr_db"][~pinned] == sol["stream_target_nmr_db"]).all()
    assert (sol["target_nmr_db"][pinned] == sol["floor_nmr_db"][pinned]).all()
    assert sol["stream_met"] and sol["stream_total_bytes"] <= limit
    # the second pass writes the predicted record lengths
    out = enc.encode_pack_alloc(view, flags, sol["bit_alloc"]) if kind == "band" else \
        enc.encode_pack_budget(view, flags, sol["budget"])
    assert np.array_equal(out["n_bytes"].cpu().numpy(), sol["n_bytes"].cpu().numpy())
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    body = body[:int(total.item())].cpu().numpy().tobytes()
    assert len(body) == sol["stream_total_bytes"] <= limit           # the body is within the limit
    data = A.pacfile.header_bytes(g["cp"]) + body
    recs = records_of(A, data)
    written = sol["n_bytes"].cpu().numpy() > 0
    assert written.sum() == len(recs)
    at = np.concatenate(([0], np.cumsum(written)))
    whole = {}
    for s in range(len(peaks)):
        r0, r1 = int(at[first[s]]), int(at[first[s + 1]])
        mine = data[recs[r0][0]:recs[r1 - 1][1]] if r1 > r0 else b""
        assert len(mine) == sol["total_bytes"][s], s
        t = float(sol["target_nmr_db"][s])
        if t not in whole:
            whole[t] = A.pacfile.encode_stream_nmr(g["pcm"], sr, t, block_switching=True, allocation=allocation)
        theirs = records_of(A, whole[t])
        assert len(theirs) == len(recs), s
        assert mine == (whole[t][theirs[r0][0]:theirs[r1 - 1][1]] if r1 > r0 else b""), s
    # met is the comparison at the final target, recomputed from n_bytes
    n = sol["n_bytes"].cpu().numpy().astype(np.int64)
    again = np.array([int(np.sum(n[a:b][n[a:b] > 0] + 4)) for a, b in zip(first, first[1:])])
    assert np.array_equal(again, sol["total_bytes"]) and np.array_equal(sol["met"], again <= peaks)
    print(f"{name} {kind}: {int((~sol['met']).sum())} of {len(peaks)} segments above their peak at their final target")
    if kind == "band":
        assert sol["met"].all()                                      # every segment within its peak


# ------------------------------------------------------------------ 6. streams
@pytest.mark.parametrize("allocation", ["budget", "band"])
def test_stream_is_the_steps_composed_by_hand(A, allocation):
    pcm, sr = excerpt("castanet")
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    kw = dict(kbps_per_channel=96, block_switching=True, allocation=allocation, segment_hops=8, peak_kbps_per_channel=128)
    data = A.pacfile.encode_stream_abr(pcm, sr, **kw)
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None)
    fb, count, peaks = A.pacfile.segment_limits(128, n_ch, sr, blocks, 8)
    first = np.append(fb, blocks) * n_ch
    limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    if allocation == "band":
        sol = enc.band_solve_peak(enc.band_curve(view, flags, cp.targetBitsPerSample), first, peaks, limit)
        out = enc.encode_pack_alloc(view, flags, sol["bit_alloc"])
    else:
        sol = enc.rate_solve_peak(enc.rate_curve(view, flags, cp.targetBitsPerSample), first, peaks, limit)
        out = enc.encode_pack_budget(view, flags, sol["budget"])
    assert sol["stream_met"] and sol["met"].all()
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    assert data == A.pacfile.header_bytes(cp) + body[:int(total.item())].cpu().numpy().tobytes()
    assert np.array_equal(A.pacfile.decode_stream(data), po.decode_stream(data))
    # a file size instead of a rate: the same stream for the size that rate stands for
    head = len(A.pacfile.header_bytes(cp))
    kw2 = dict(kw, kbps_per_channel=None, max_bytes=head + limit)
    assert A.pacfile.encode_stream_abr(pcm, sr, **kw2) == data
    got, rep, info = A.quality.encode_stream_to_rate(pcm, sr, **kw)
    assert got == data
    seg = info["segments"]
    assert np.array_equal(seg["first_block"], fb) and np.array_equal(seg["blocks"], count)
    assert np.array_equal(seg["limit_bytes"], peaks)
    for k in ("target_nmr_db", "total_bytes", "floor_nmr_db", "pinned"):
        assert np.array_equal(seg[k], sol[k]), k
    assert info["stream_target_nmr_db"] == sol["stream_target_nmr_db"]
    assert info["target_nmr_db"].shape == (blocks,)
    assert np.array_equal(info["target_nmr_db"], np.repeat(sol["target_nmr_db"], count))
    assert info["limit_bytes"] == limit and info["total_bytes"] == sol["stream_total_bytes"] == len(data) - head
    print(f"{allocation}: stream {sol['stream_target_nmr_db']} dB, segments {sol['target_nmr_db'].tolist()}, floors "
          f"{sol['floor_nmr_db'].tolist()}, bytes {sol['total_bytes'].tolist()} of {peaks.tolist()}")


@pytest.mark.parametrize("kind", KINDS)
def test_a_segment_beyond_its_peak_is_named(A, kind):
    """a peak rate at which, by the model on the GPU's curve, the stream's limit is reached and some segment is not"""
    g = own_curves(A, "castanet")
    n_ch, blocks, sr = g["cp"].nChannels, g["view"].n_frames, g["sr"]
    limit = int(np.floor(96 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    found = None
    for kbps in np.arange(48.0, 0.0, -0.5):
        fb, count, peaks = A.pacfile.segment_limits(kbps, n_ch, sr, blocks, 8)
        ref = pm.solve_peak(kind, g["host"][kind], np.append(fb, blocks) * n_ch, peaks, limit)
        if (ref["met"] == 0).any():
            found = kbps, int(np.argmax(ref["met"] == 0)), fb, peaks, ref
            break
    assert found is not None
    kbps, s, fb, peaks, ref = found
    assert ref["met_stream"] == 1
    print(f"{kind}: peak {kbps} kb/s, met {ref['met'].tolist()}, floors {ref['floor'].tolist()}, first segment {s}")
    with pytest.raises(ValueError) as err:
        A.pacfile.encode_stream_abr(g["pcm"], sr, kbps_per_channel=96, block_switching=True, segment_hops=8,
                                    peak_kbps_per_channel=float(kbps), allocation="band" if kind == "band" else "budget")
    msg = str(err.value)
    assert f"segment {s} " in msg and f"from block {int(fb[s])}," in msg, msg
    assert f"{int(peaks[s])} bytes" in msg and f"{int(ref['total'][s])} bytes" in msg, msg
    assert ("cannot be reached at all" in msg) == (ref["floor"][s] == 30 * 64), msg
    assert ("fits at its own floor" in msg) == (ref["floor"][s] != 30 * 64), msg
    if kind == "band":                                               # and a stream that cannot be reached at all
        with pytest.raises(ValueError, match="cannot be reached: at the highest target"):
            A.pacfile.encode_stream_abr(g["pcm"], sr, kbps_per_channel=1, block_switching=True, segment_hops=8,
                                        peak_kbps_per_channel=128, allocation="band")


def test_arguments(A):
    import torch
    g = own_curves(A, "castanet")
    enc, band, rate = g["enc"], g["dev"]["band"], g["dev"]["rate"]
    ptr = A.engine._ptr
    n_cf = band["cap"].shape[0]
    alloc = torch.zeros((n_cf, enc.band_stride), dtype=torch.int32, device=enc.device)
    budget = torch.zeros((n_cf, 8), dtype=torch.int32, device=enc.device)
    nby = torch.zeros((n_cf,), dtype=torch.int32, device=enc.device)
    cpd = torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device)
    res = torch.zeros((3, 4), dtype=torch.int32, device=enc.device)
    floor = torch.zeros((2,), dtype=torch.int32, device=enc.device)
    i64 = lambda *v: np.array(v, np.int64)                                          # noqa: E731
    half = n_cf // 2

    def band_call(first, peaks, limit=10 ** 6, n_seg=2, floor=floor, stream=res[2:]):
        return enc.lib.pacx_band_solve_peak(
            enc.h, n_cf, ptr(band["nmr"]), ptr(band["cap"]), ptr(band["cap_alloc"]), n_seg,
            None if first is None else first.ctypes.data, None if peaks is None else peaks.ctypes.data, limit, -30.0,
            30.0, ptr(alloc), ptr(nby), ptr(cpd), ptr(floor), ptr(res), ptr(stream), None)

    def rate_call(first, peaks, limit=10 ** 6, n_seg=2, floor=floor, stream=res[2:]):
        return enc.lib.pacx_rate_solve_peak(
            enc.h, n_cf, int(rate["row"]), int(rate["sub_stride"]), ptr(rate["worst"]), ptr(rate["bits"]),
            ptr(rate["steps"]), n_seg, None if first is None else first.ctypes.data,
            None if peaks is None else peaks.ctypes.data, limit, -30.0, 30.0, ptr(budget), ptr(nby), ptr(cpd), ptr(floor),
            ptr(res), ptr(stream), None)

    good_first, good_peaks = i64(0, half, n_cf), i64(10 ** 6, 10 ** 6)
    for call in (band_call, rate_call):
        assert call(good_first, good_peaks) == 0
        assert call(good_first, good_peaks, n_seg=0) == A._lib.E_ARG
        assert call(None, good_peaks) == A._lib.E_ARG and call(good_first, None) == A._lib.E_ARG
        assert call(i64(0, n_cf, half), good_peaks) == A._lib.E_ARG
        assert call(good_first, i64(5, -1)) == A._lib.E_ARG and b"negative" in enc.lib.pacx_last_error(enc.h)
        assert call(good_first, good_peaks, limit=-1) == A._lib.E_ARG and b"negative" in enc.lib.pacx_last_error(enc.h)
        assert call(good_first, good_peaks, floor=None) == A._lib.E_ARG and b"null" in enc.lib.pacx_last_error(enc.h)
        assert call(good_first, good_peaks, stream=None) == A._lib.E_ARG
    torch.cuda.synchronize()
    for limit in (-1, 2.5):
        with pytest.raises(ValueError, match="limit_bytes"):
            enc.band_solve_peak(band, good_first, good_peaks, limit)
    with pytest.raises(ValueError):
        enc.rate_solve_peak(rate, [0, n_cf, half], [1, 2], 10)
    vq = A.engine.Encoder(g["sr"], 128 / (g["sr"] / 1000), use_vq=True)
    assert vq.lib.pacx_band_solve_peak(vq.h, 1, None, None, None, 1, None, None, 0, -30.0, 30.0, None, None, None, None,
                                       None, None, None) == A._lib.E_UNSUPPORTED
    vq.close()


# ------------------------------------------------------------------ 7. nothing else moves
def test_nothing_else_moves(A):
    """a peak solve grows the handle's solve state and leaves the stream's state behind the segments': the pick and the
    ordinary encode on that handle give what they gave before"""
    g = own_curves(A, "castanet")
    enc, band, view, flags = g["enc"], g["dev"]["band"], g["view"], g["flags"]

    def snapshot():
        out = {("band_pick", k): v.cpu().numpy() for k, v in enc.band_pick(band, -3.0).items()}
        e = enc.encode_pack(view, flags)
        body, total = enc.gather_body(e["payload"], e["n_bytes"])
        out["encode_pack", "body"] = body[:int(total.item())].cpu().numpy().tobytes()
        return out

    before = snapshot()
    n_cf = band["cap"].shape[0]
    first = np.linspace(0, n_cf, 62).astype(np.int64)
    for kind in KINDS:
        host = g["host"][kind]
        peaks = sm.limits_for(kind, host, first)
        u = pm.floors(kind, host, first, peaks)
        check(enc, kind, g["dev"][kind], host, first, peaks, pm.stream_limits(kind, host, first, peaks, u=u)[0],
              what="61 segments", u=u)
    after = snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
