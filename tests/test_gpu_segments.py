"""One noise-to-mask target per stretch of a stream on the GPU (pacx_rate_solve_segments / pacx_band_solve_segments,
Encoder.rate_solve_segments / band_solve_segments, the segment_hops keyword of pacfile.encode_stream_abr and
quality.encode_stream_to_rate) against tests/segment_model.py, which slices the arrays and calls the plain models.

Bars.  The solve is integers and comparisons on given arrays, so every output equals the model's: t, met, total per
segment; bit_alloc / budget, n_bytes, capped per channel-frame.  No window anywhere.  A stream's segment is, record
for record, the stream of encode_stream_nmr at that segment's target, and stays within its limit.
"""
import ctypes
import functools

import numpy as np
import pytest

import band_model as bm
import segment_model as sm
from conftest import load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

KINDS = ("band", "rate")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


# ------------------------------------------------------------------------------------------------------ helpers
_ENC = {}


def encoder(A, kind):
    """a handle whose band tables are the synthetic curves' (band_model.synthetic: 44100 Hz), one per kind, kept"""
    if kind not in _ENC:
        _ENC[kind] = A.engine.Encoder(44100, 128 / 44.1)
    return _ENC[kind]


def on_device(enc, kind, c):
    import torch
    keys = ("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps")
    dev = {k: torch.as_tensor(np.ascontiguousarray(c[k]), device=enc.device) for k in keys}
    if kind == "rate":
        dev["row"], dev["sub_stride"] = c["row"], c["sub_stride"]
    return dev


def gpu_solve(enc, kind, dev, first, limits, lo_db=-30, hi_db=30):
    fn = enc.band_solve_segments if kind == "band" else enc.rate_solve_segments
    return fn(dev, first, limits, lo_db, hi_db)


def check(enc, kind, dev, c, first, limits, lo_db=-30, hi_db=30, what=""):
    """the segmented solve against the model on the same arrays: everything equal"""
    sol = gpu_solve(enc, kind, dev, first, limits, lo_db, hi_db)
    ref = sm.solve_segments(kind, c, first, limits, int(lo_db * 64), int(hi_db * 64))
    t = np.round(sol["target_nmr_db"] * 64).astype(np.int64)
    assert sol["target_nmr_db"].dtype == np.float64 and sol["met"].dtype == bool and sol["total_bytes"].dtype == np.int64
    bad = np.nonzero((t != ref["t"]) | (sol["met"] != (ref["met"] != 0)) | (sol["total_bytes"] != ref["total"]))[0]
    print(f"{what} {kind}: {len(limits)} segments, {int(sol['met'].sum())} met, {len(set(t.tolist()))} targets, "
          f"{len(bad)} differ")
    for s in bad[:3]:
        print(f"  segment {s}: gpu {(t[s], sol['met'][s], sol['total_bytes'][s])}, model "
              f"{(ref['t'][s], ref['met'][s], ref['total'][s])}")
    assert not len(bad), (what, kind)
    for k in sm.PER_CF[kind]:
        assert np.array_equal(sol[k].cpu().numpy(), ref[k]), (what, kind, k)
    return sol, ref


@functools.lru_cache(maxsize=None)
def material(kind):
    return sm.material(kind)


# boundaries one frame before, at and after 64 and 256 (a wave and a workgroup of k_solve_pick; every one of them
# inside some 4-frame workgroup of k_band_pick_seg), with empty segments between
EDGES = np.array([0, 63, 64, 65, 65, 255, 256, 257, 257, 257, 511, 513, 1023, 1024, 1025, 1279, 1281, 1281, 2999, 3000],
                 np.int64)


# ------------------------------------------------------------------ 1. synthetic curves against the model
@pytest.mark.parametrize("partition", ["cycle", "edges"])
@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_curves(A, kind, partition):
    c, first, limits = material(kind)
    if partition == "edges":
        first, limits = EDGES, sm.limits_for(kind, c, EDGES)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    sol, ref = check(enc, kind, dev, c, first, limits, what=partition)
    assert 0 < sol["met"].sum() < len(limits)                       # both decisions are taken


@pytest.mark.parametrize("lo_db,hi_db", [(-2, 5.5), (0.078125, 0.078125)])
@pytest.mark.parametrize("kind", KINDS)
def test_other_ranges(A, kind, lo_db, hi_db):
    c, first, _ = material(kind)
    enc = encoder(A, kind)
    limits = sm.limits_for(kind, c, first, int(lo_db * 64), int(hi_db * 64))
    check(enc, kind, on_device(enc, kind, c), c, first, limits, lo_db, hi_db, what=f"range {lo_db} .. {hi_db}")


# ------------------------------------------------------------------ 2. one segment is the plain solve
def plain_solve(enc, kind, dev, limit, lo_db=-30, hi_db=30):
    return enc.band_solve(dev, limit, lo_db, hi_db) if kind == "band" else enc.rate_solve(dev, None, limit, lo_db, hi_db)


def assert_plain_equals_model(kind, one, ref, what):
    """a plain solve's dict against the model's one-segment result: everything equal"""
    assert isinstance(one["target_nmr_db"], float) and isinstance(one["met"], bool) and isinstance(one["total_bytes"], int)
    got = (round(one["target_nmr_db"] * 64), one["met"], one["total_bytes"])
    want = (int(ref["t"][0]), bool(ref["met"][0]), int(ref["total"][0]))
    print(f"{what} {kind}: gpu {got}, model {want}")
    assert one["target_nmr_db"] * 64 == got[0] and got == want, (what, kind)
    for k in sm.PER_CF[kind]:
        assert np.array_equal(one[k].cpu().numpy(), ref[k]), (what, kind, k)


@pytest.mark.parametrize("kind", KINDS)
def test_one_segment_equals_the_plain_solve(A, kind):
    """both routes to the one solve -- the plain entry point, whose table the init kernel writes, and the segmented
    one with an uploaded one-segment table -- against each other and against the model"""
    c, _, _ = material(kind)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    n_cf = sm.n_cf_of(kind, c)
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    for limit in ((small + big) // 2, small - 1, small, 10 ** 12):
        seg = gpu_solve(enc, kind, dev, [0, n_cf], [limit])
        one = plain_solve(enc, kind, dev, limit)
        assert (seg["target_nmr_db"][0], bool(seg["met"][0]), int(seg["total_bytes"][0])) == \
            (one["target_nmr_db"], one["met"], one["total_bytes"]), limit
        for k in sm.PER_CF[kind]:
            assert np.array_equal(seg[k].cpu().numpy(), one[k].cpu().numpy()), (limit, k)
        ref = sm.solve_segments(kind, c, [0, n_cf], [limit])
        assert_plain_equals_model(kind, one, ref, f"limit {limit}")
        assert (round(seg["target_nmr_db"][0] * 64), int(seg["met"][0]), int(seg["total_bytes"][0])) == \
            (ref["t"][0], ref["met"][0], ref["total"][0]), limit
        for k in sm.PER_CF[kind]:
            assert np.array_equal(seg[k].cpu().numpy(), ref[k]), (limit, k)


@pytest.mark.parametrize("n_cf", [0, 1, 3, 4, 5, 255, 256, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_plain_solves_at_the_workgroup_edges(A, kind, n_cf):
    """the plain solves with no, one and a few frames and one frame before, at and after the band pick's 4-frame and
    the rate pick's 256-frame workgroup, at four limits: one byte less than the highest target takes, exactly that,
    the midpoint of the smallest and the largest body, and more than anything takes.  Without frames the first of
    them is -1, which is no limit: the call refuses it, as every negative limit."""
    c = sm.synthetic(kind, n_cf, 11)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    for limit in (small - 1, small, (small + big) // 2, 10 ** 12):
        if limit < 0:
            assert n_cf == 0
            with pytest.raises(A._lib.PacxError, match="negative limit"):
                plain_solve(enc, kind, dev, limit)
            continue
        ref = sm.solve_segments(kind, c, [0, n_cf], [limit])
        assert_plain_equals_model(kind, plain_solve(enc, kind, dev, limit), ref, f"{n_cf} frames, limit {limit}")


@pytest.mark.parametrize("kind", KINDS)
def test_plain_and_segmented_solves_interleaved(A, kind):
    """a plain solve, a segmented one and a second plain one with another limit, queued on one handle and one stream
    through the C entry points and read back only after the third: they share the handle's states and its segment
    table, which the plain solves' init kernel writes and the segmented solve uploads"""
    import torch
    c, _, _ = material(kind)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    n_cf = sm.n_cf_of(kind, c)
    first, limits = EDGES, sm.limits_for(kind, c, EDGES)
    small, big = sm.total(kind, c, 30 * 64), sm.total(kind, c, -30 * 64)
    plain_limits = ((small + big) // 2, small + (big - small) // 5)
    check(enc, kind, dev, c, first, limits, what="before")          # the handle's states are grown: no wait below
    ptr = A.engine._ptr
    arrays = [ptr(dev[k]) for k in (("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps"))]
    head = [] if kind == "band" else [int(dev["row"]), int(dev["sub_stride"])]
    width = enc.band_stride if kind == "band" else 8
    seg_first, seg_limit = np.ascontiguousarray(first, np.int64), np.ascontiguousarray(limits, np.int64)

    def queue(n_seg):
        """one solve queued, nothing read: n_seg None is the plain entry point -> its outputs on the device"""
        out = [torch.zeros((n_cf, width), dtype=torch.int32, device=enc.device),
               torch.zeros((n_cf,), dtype=torch.int32, device=enc.device),
               torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device),
               torch.zeros((n_seg or 1, 4), dtype=torch.int32, device=enc.device)]
        name = f"pacx_{kind}_solve" + ("_segments" if n_seg else "")
        size = [ctypes.c_int64(n_seg), seg_first.ctypes.data, seg_limit.ctypes.data] if n_seg else \
            [ctypes.c_int64(int(plain_limits[len(queued) // 2]))]
        rc = getattr(enc.lib, name)(enc.h, ctypes.c_int64(n_cf), *head, *arrays, *size, ctypes.c_double(-30.0),
                                    ctypes.c_double(30.0), *(ptr(t) for t in out), enc._stream())
        assert rc == 0, (name, enc.lib.pacx_last_error(enc.h))
        queued.append(out)

    queued = []
    for n_seg in (None, len(limits), None):
        queue(n_seg)
    torch.cuda.synchronize()
    refs = [sm.solve_segments(kind, c, [0, n_cf], [plain_limits[0]]), sm.solve_segments(kind, c, first, limits),
            sm.solve_segments(kind, c, [0, n_cf], [plain_limits[1]])]
    assert refs[0]["t"][0] != refs[2]["t"][0]                        # the two plain solves have answers of their own
    for i, (out, ref) in enumerate(zip(queued, refs)):
        res = out[3].cpu().numpy()
        got = (res[:, 0].astype(np.int64), res[:, 1].astype(np.int64), res[:, 2:].copy().view(np.int64)[:, 0])
        print(f"{kind} solve {i}: {len(got[0])} segments, {int(got[1].sum())} met")
        for g, k in zip(got, ("t", "met", "total")):
            assert np.array_equal(g, ref[k]), (kind, i, k)
        for t, k in zip(out, sm.PER_CF[kind]):
            assert np.array_equal(t.cpu().numpy().astype(ref[k].dtype), ref[k]), (kind, i, k)


# ------------------------------------------------------------------ 3. as many segments as frames, and more
@pytest.mark.parametrize("kind", KINDS)
def test_every_frame_its_own_segment(A, kind):
    """600 segments: more than one workgroup of the init and step kernels; 1200 with every other one empty; no
    channel-frames at all with three empty segments"""
    n = 600
    c = sm.synthetic(kind, n, 5)
    enc = encoder(A, kind)
    dev = on_device(enc, kind, c)
    first = np.arange(n + 1, dtype=np.int64)
    check(enc, kind, dev, c, first, sm.limits_for(kind, c, first), what="600 of 1")
    first = np.repeat(np.arange(n + 1, dtype=np.int64), 2)[:-1]          # 0 0 1 1 2 ... : segments 0, 2, ... are empty
    assert len(first) == 2 * n + 1
    sol, _ = check(enc, kind, dev, c, first, sm.limits_for(kind, c, first), what="1200, every other empty")
    assert (sol["target_nmr_db"][0::2] == -30.0).all() and sol["met"][0::2].all() and not sol["total_bytes"][0::2].any()
    c0 = sm.slice_curve(kind, c, 0, 0)
    sol, _ = check(enc, kind, on_device(enc, kind, c0), c0, [0, 0, 0, 0], [0, 5, 10 ** 12], -2, 5.5, what="no frames")
    assert sol["target_nmr_db"].tolist() == [-2.0] * 3 and sol["met"].all() and not sol["total_bytes"].any()


# ------------------------------------------------------------------ 4. the GPU's own curves
def silence_and_drop():
    """tests/test_gpu_band.py's construction: digital silence, a short-coded hop the reference drops, ordinary hops"""
    rng = np.random.default_rng(5)
    pcm = np.zeros((6 * 1024, 2), np.int16)
    pcm[1024:2048] = rng.integers(-3000, 3000, (1024, 2))
    pcm[3 * 1024 + 900:4 * 1024] = rng.integers(-30000, 30000, (124, 2))
    pcm[4 * 1024:] = rng.integers(-3000, 3000, (2 * 1024, 2))
    return pcm, 48000


def excerpt(name, hops=24):
    ex = load_excerpt(name)
    return np.ascontiguousarray(ex["pcm"][:hops * 1024]), int(ex["sr"])


_OWN = {}


def own_curves(A, name):
    """the stream's handle, view and flags, and for both kinds the device curve and the model's view of its arrays"""
    if name not in _OWN:
        pcm, sr = silence_and_drop() if name == "silence_and_drop" else excerpt(name)
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["castanet", "silence_and_drop"])
def test_own_curves(A, name, kind):
    g = own_curves(A, name)
    n_ch, blocks = g["cp"].nChannels, g["view"].n_frames
    fb, count, limits = A.pacfile.segment_limits(96, n_ch, g["sr"], blocks, 5)
    first = np.append(fb, blocks) * n_ch
    host = g["host"][kind]
    if name == "silence_and_drop":
        dropped = (host["cap" if kind == "band" else "steps"] < 0).all(axis=1).reshape(blocks, n_ch).all(axis=1)
        assert dropped.sum() == 1                                    # the hop the reference drops
        at = int(np.argmax(dropped))                                 # and a segment that holds nothing else
        first = np.array(sorted(set(first.tolist()) | {at * n_ch, (at + 1) * n_ch}), np.int64)
        limits = np.array([A.pacfile.segment_limits(96, n_ch, g["sr"], int(b - a) // n_ch, 5)[2][0]
                           for a, b in zip(first, first[1:])], np.int64)
    sol, ref = check(g["enc"], kind, g["dev"][kind], host, first, limits, what=name)
    if name == "silence_and_drop":
        s = int(np.nonzero(first == at * n_ch)[0][0])
        assert (sol["target_nmr_db"][s], sol["met"][s], sol["total_bytes"][s]) == (-30.0, True, 0)


# ------------------------------------------------------------------ 5. streams
def records_of(A, data):
    """(offset of the length prefix, end) of every record of a .pac"""
    _, pos = A.pacfile.parse_header(data)
    offs, sizes = A.pacfile.record_chain(data, pos, bm.PAYLOAD_STRIDE)
    return [(o - 4, o + n) for o, n in zip(offs, sizes)]


@pytest.mark.parametrize("kbps", [96, 128])
@pytest.mark.parametrize("allocation", ["budget", "band"])
@pytest.mark.parametrize("name", ["harpsichord", "spmg"])
def test_streams(A, name, allocation, kbps):
    pcm, sr = excerpt(name)
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    kw = dict(kbps_per_channel=kbps, block_switching=True, allocation=allocation)
    data, rep, info = A.quality.encode_stream_to_rate(pcm, sr, segment_hops=8, **kw)
    assert data == A.pacfile.encode_stream_abr(pcm, sr, segment_hops=8, **kw)
    seg = info["segments"]
    fb, count, limits = A.pacfile.segment_limits(kbps, n_ch, sr, blocks, 8)
    assert np.array_equal(seg["first_block"], fb) and np.array_equal(seg["blocks"], count)
    assert np.array_equal(seg["limit_bytes"], limits) and len(limits) == 4
    assert info["target_nmr_db"].shape == (blocks,)
    assert np.array_equal(info["target_nmr_db"], np.repeat(seg["target_nmr_db"], count))
    recs = records_of(A, data)
    written = (info["n_bytes"] > 0).reshape(-1)                      # per channel-frame: has a record
    assert written.sum() == len(recs)
    at = np.concatenate(([0], np.cumsum(written)))                   # records before every channel-frame
    print(f"{name} {allocation} {kbps} kb/s: targets {seg['target_nmr_db'].tolist()}, bytes "
          f"{seg['total_bytes'].tolist()} of {limits.tolist()}")
    for s in range(len(limits)):
        r0, r1 = int(at[fb[s] * n_ch]), int(at[(fb[s] + count[s]) * n_ch])
        mine = data[recs[r0][0]:recs[r1 - 1][1]] if r1 > r0 else b""
        assert len(mine) == seg["total_bytes"][s] <= limits[s], s
        whole = A.pacfile.encode_stream_nmr(pcm, sr, float(seg["target_nmr_db"][s]), block_switching=True,
                                            allocation=allocation)
        theirs = records_of(A, whole)
        assert len(theirs) == len(recs), s                          # which hops are dropped does not depend on the target
        assert mine == (whole[theirs[r0][0]:theirs[r1 - 1][1]] if r1 > r0 else b""), s
    assert np.array_equal(A.pacfile.decode_stream(data), po.decode_stream(data))
    # one segment that holds every block: the whole-stream call, byte for byte
    assert A.pacfile.encode_stream_abr(pcm, sr, segment_hops=blocks, **kw) == A.pacfile.encode_stream_abr(pcm, sr, **kw)
    assert A.pacfile.encode_stream_abr(pcm, sr, segment_hops=1000, **kw) == A.pacfile.encode_stream_abr(pcm, sr, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_unreachable_segment_is_named(A, kind):
    """a rate at which, by the model on the GPU's curve, some segments can be reached and some cannot"""
    g = own_curves(A, "castanet")
    n_ch, blocks, sr = g["cp"].nChannels, g["view"].n_frames, g["sr"]
    found = None
    for kbps in np.arange(48.0, 0.0, -0.5):
        fb, count, limits = A.pacfile.segment_limits(kbps, n_ch, sr, blocks, 8)
        ref = sm.solve_segments(kind, g["host"][kind], np.append(fb, blocks) * n_ch, limits)
        if 0 < (ref["met"] == 0).sum() < len(limits):
            found = kbps, int(np.argmax(ref["met"] == 0)), fb, limits, ref
            break
    assert found is not None
    kbps, s, fb, limits, ref = found
    print(f"{kind}: {kbps} kb/s, met {ref['met'].tolist()}, first unreachable segment {s}")
    with pytest.raises(ValueError) as err:
        A.pacfile.encode_stream_abr(g["pcm"], sr, kbps_per_channel=float(kbps), block_switching=True, segment_hops=8,
                                    allocation="band" if kind == "band" else "budget")
    msg = str(err.value)
    assert f"segment {s} " in msg and f"from block {int(fb[s])}," in msg, msg
    assert f"{int(limits[s])} bytes" in msg and f"{int(ref['total'][s])} bytes" in msg, msg


# ------------------------------------------------------------------ 6. arguments
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
    res = torch.zeros((2, 4), dtype=torch.int32, device=enc.device)
    i64 = lambda *v: np.array(v, np.int64)                                          # noqa: E731
    half = n_cf // 2

    def band_call(n_seg, first, limits, lo=-30.0, hi=30.0, n=n_cf, result=res):
        return enc.lib.pacx_band_solve_segments(
            enc.h, n, ptr(band["nmr"]), ptr(band["cap"]), ptr(band["cap_alloc"]), n_seg,
            None if first is None else first.ctypes.data, None if limits is None else limits.ctypes.data, lo, hi,
            ptr(alloc), ptr(nby), ptr(cpd), ptr(result), None)

    def rate_call(n_seg, first, limits, lo=-30.0, hi=30.0, n=n_cf, result=res):
        return enc.lib.pacx_rate_solve_segments(
            enc.h, n, int(rate["row"]), int(rate["sub_stride"]), ptr(rate["worst"]), ptr(rate["bits"]),
            ptr(rate["steps"]), n_seg, None if first is None else first.ctypes.data,
            None if limits is None else limits.ctypes.data, lo, hi, ptr(budget), ptr(nby), ptr(cpd), ptr(result), None)

    good_first, good_limits = i64(0, half, n_cf), i64(10 ** 6, 10 ** 6)
    for call in (band_call, rate_call):
        assert call(2, good_first, good_limits) == 0
        for n_seg in (0, -1):
            assert call(n_seg, good_first, good_limits) == A._lib.E_ARG
        assert call(2, None, good_limits) == A._lib.E_ARG and b"null pointer" in enc.lib.pacx_last_error(enc.h)
        assert call(2, good_first, None) == A._lib.E_ARG
        for first in (i64(1, half, n_cf), i64(0, half, n_cf - 1), i64(0, half, n_cf + 1), i64(0, n_cf, half),
                      i64(0, -1, n_cf), i64(0, n_cf + 1, n_cf)):
            assert call(2, first, good_limits) == A._lib.E_ARG, first
        assert call(2, good_first, i64(5, -1)) == A._lib.E_ARG and b"negative" in enc.lib.pacx_last_error(enc.h)
        assert call(2, good_first, good_limits, result=None) == A._lib.E_ARG
        assert call(2, good_first, good_limits, n=-1) == A._lib.E_ARG
        for lo, hi in ((float("nan"), 3.0), (3.0, -3.0), (-30.01, 30.0), (-2e6, 0.0)):       # the plain solves' rules
            assert call(2, good_first, good_limits, lo, hi) == A._lib.E_ARG
    torch.cuda.synchronize()
    # the Python layer refuses the same before the call
    for first, limits in (([0, half], [1, 2]), ([1, half, n_cf], [1, 2]), ([0, n_cf, half], [1, 2]),
                          ([0, half, n_cf], [1, -2]), ([0], []), ([0.5, n_cf], [1])):
        with pytest.raises(ValueError):
            enc.band_solve_segments(band, first, limits)
        with pytest.raises(ValueError):
            enc.rate_solve_segments(rate, first, limits)
    with pytest.raises(ValueError):
        enc.band_solve_segments({"nmr": band["nmr"], "cap": band["cap"][:, :4], "cap_alloc": band["cap_alloc"]},
                                [0, n_cf], [1])
    assert enc.band_solve_segments(band, (0, half, n_cf), range(10 ** 6, 10 ** 6 + 2))["met"].all()   # any sequences
    vq = A.engine.Encoder(g["sr"], 128 / (g["sr"] / 1000), use_vq=True)
    assert vq.lib.pacx_band_solve_segments(vq.h, 1, None, None, None, 1, None, None, -30.0, 30.0, None, None, None, None,
                                           None) == A._lib.E_UNSUPPORTED
    assert vq.lib.pacx_rate_solve_segments(vq.h, 1, 8, 1, None, None, None, 1, None, None, -30.0, 30.0, None, None, None,
                                           None, None) == A._lib.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        vq.band_solve_segments(band, [0, n_cf], [1])
    vq.close()
    pcm, sr = g["pcm"], g["sr"]
    abr = A.pacfile.encode_stream_abr
    with pytest.raises(ValueError, match="max_bytes"):
        abr(pcm, sr, max_bytes=100000, segment_hops=8)
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="segment_hops"):
            abr(pcm, sr, kbps_per_channel=96, segment_hops=bad)
    with pytest.raises(ValueError, match="max_bytes"):
        A.quality.encode_stream_to_rate(pcm, sr, max_bytes=[100000], segment_hops=8)
    for kw in ({"n_lines": 512}, {"chunk_hops": 4}, {"use_vq": True}, {"use_sbr": True}):
        with pytest.raises(NotImplementedError):
            abr(pcm, sr, kbps_per_channel=96, segment_hops=8, **kw)


def test_a_list_of_rates(A):
    pcm, sr = excerpt("castanet")
    both = A.quality.encode_stream_to_rate(pcm, sr, kbps_per_channel=[96, 128], block_switching=True, segment_hops=8)
    assert len(both) == 2
    for (data, rep, info), kbps in zip(both, (96, 128)):
        assert data == A.pacfile.encode_stream_abr(pcm, sr, kbps_per_channel=kbps, block_switching=True, segment_hops=8)
        assert (info["segments"]["total_bytes"] <= info["segments"]["limit_bytes"]).all()
    assert (both[0][2]["segments"]["target_nmr_db"] >= both[1][2]["segments"]["target_nmr_db"]).all()


# ------------------------------------------------------------------ 7. nothing else moves
def test_nothing_else_moves(A):
    """a segmented solve grows the handle's solve state to 50 and leaves the boundaries beside it: the plain solves,
    the pick and the ordinary encode on that handle give what they gave before"""
    g = own_curves(A, "castanet")
    enc, band, rate, view, flags = g["enc"], g["dev"]["band"], g["dev"]["rate"], g["view"], g["flags"]
    host = g["host"]
    limit_b = (bm.total(host["band"], 30 * 64) + bm.total(host["band"], -30 * 64)) // 2
    limit_r = (sm.total("rate", host["rate"], 30 * 64) + sm.total("rate", host["rate"], -30 * 64)) // 2

    def snapshot():
        out = {}
        for name, sol in (("band_solve", enc.band_solve(band, limit_b)), ("rate_solve", enc.rate_solve(rate, flags, limit_r)),
                          ("band_pick", enc.band_pick(band, -3.0))):
            for k, v in sol.items():
                out[name, k] = v.cpu().numpy() if hasattr(v, "cpu") else v
        e = enc.encode_pack(view, flags)
        body, total = enc.gather_body(e["payload"], e["n_bytes"])
        out["encode_pack", "body"] = body[:int(total.item())].cpu().numpy().tobytes()
        return out

    before = snapshot()
    n_cf = band["cap"].shape[0]
    first = np.linspace(0, n_cf, 51).astype(np.int64)
    assert len(first) == 51 and first[0] == 0 and first[-1] == n_cf
    for kind in KINDS:
        limits = sm.limits_for(kind, host[kind], first)
        check(enc, kind, g["dev"][kind], host[kind], first, limits, what="50 segments")
    after = snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
