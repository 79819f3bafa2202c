"""CPU checks of the leaky bucket (include/pacx_bucket.h, pacx_bucket_scan / pacx_band_solve_bucket / pacx_rate_solve_bucket):
tests/bucket_model.py's hop-by-hop scan against a statement of every level without a recursion, exact in pieces, the
composition rule the kernel scans with against the hops applied one by one, the solve against the plain models where
the buffer cannot bind, pacfile.bucket's drain, the exports, what the Python layer refuses before it touches a GPU, and
the two messages of an unmet call."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import bucket_model as kb

Q = kb.Q
NAMES = ("pacx_bucket_scan", "pacx_band_solve_bucket", "pacx_rate_solve_bucket")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


def drawn(rng):
    """one case: hops of one to three channels, mostly small against a drain of the same order, sometimes empty, a
    fractional drain, a start level anywhere in the buffer"""
    n_ch, n_hops = int(rng.integers(1, 4)), int(rng.integers(0, 40))
    n_bytes = rng.integers(-3, 400, n_hops * n_ch) * (rng.random(n_hops * n_ch) < 0.7)
    drain = int(rng.integers(0, 500 << Q)) if rng.random() < 0.8 else int(rng.integers(0, 3)) * (1 << 50)
    size = int(rng.integers(0, 3000))
    start = int(rng.integers(0, (size << Q) + 1))
    return n_bytes, n_ch, (drain, size, start)


def test_scan_is_the_quadratic_statement():
    rng = np.random.default_rng(1)
    seen = {"over": 0, "emptied": 0, "start_peak": 0}
    for _ in range(300):
        n_bytes, n_ch, b = drawn(rng)
        s = kb.scan(n_bytes, n_ch, b)
        x = kb.hop_bytes(n_bytes, n_ch)
        level = kb.quadratic(x, b[0], b[2])
        assert s["level"] == level
        assert s["total"] == sum(x) == int(np.sum(np.where(n_bytes > 0, n_bytes + 4, 0)))
        assert s["peak_q16"] == max([b[2]] + level)
        assert s["peak_hop"] == (-1 if max([b[2]] + level) == b[2] else level.index(max(level)))
        over = [h for h, v in enumerate(level) if v > b[1] << Q]
        assert s["first_over"] == (over[0] if over else -1)
        assert s["end_q16"] == (max(0, level[-1] - b[0]) if level else b[2])
        seen["over"] += bool(over)
        seen["emptied"] += any(v - b[0] < 0 for v in level)
        seen["start_peak"] += s["peak_hop"] < 0 < len(level)
    assert min(seen.values()) > 5, seen                       # the draw reaches every branch


def test_scan_in_pieces_is_exact():
    rng = np.random.default_rng(2)
    for _ in range(100):
        n_bytes, n_ch, b = drawn(rng)
        whole = kb.scan(n_bytes, n_ch, b)
        n_hops = len(n_bytes) // n_ch
        cuts = sorted(int(c) for c in rng.integers(0, n_hops + 1, 3))
        level, total, start, peak, peak_hop, over = [], 0, b[2], b[2], -1, -1
        for a, e in zip([0] + cuts, cuts + [n_hops]):
            part = kb.scan(n_bytes[a * n_ch:e * n_ch], n_ch, (b[0], b[1], start))
            level += part["level"]
            total += part["total"]
            if part["peak_q16"] > peak:
                peak, peak_hop = part["peak_q16"], a + part["peak_hop"]
            if over < 0 and part["first_over"] >= 0:
                over = a + part["first_over"]
            start = part["end_q16"]
        assert (level, total, peak, peak_hop, over, start) == \
            (whole["level"], whole["total"], whole["peak_q16"], whole["peak_hop"], whole["first_over"], whole["end_q16"])


def test_composition_rule():
    """maps composed in any grouping, applied once, against the hops applied one by one -- and the levels of a scan
    as the exclusive prefix of the hops' maps applied to the start level"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        n_bytes, n_ch, b = drawn(rng)
        x = kb.hop_bytes(n_bytes, n_ch)
        maps = [kb.hop_map(v, b[0]) for v in x]
        f, seq = b[2], []
        for m in maps:
            seq.append(f)
            f = kb.apply(m, f)
        prefix, levels = None, []
        for m, v in zip(maps, x):
            levels.append((b[2] if prefix is None else kb.apply(prefix, b[2])) + (v << Q))
            prefix = m if prefix is None else kb.then(prefix, m)
        assert levels == kb.scan(n_bytes, n_ch, b)["level"]
        if len(maps) >= 3:                                   # (a b) c == a (b c), as maps and as pairs
            i, j = sorted(int(v) for v in rng.integers(1, len(maps), 2))
            fold = lambda ms: None if not ms else (ms[0] if len(ms) == 1 else kb.then(fold(ms[:-1]), ms[-1]))   # noqa: E731
            left, mid, right = fold(maps[:i]), fold(maps[i:j]), fold(maps[j:])
            parts = [p for p in (left, mid, right) if p is not None]
            one = fold(parts)
            other = parts[0] if len(parts) == 1 else kb.then(parts[0], fold(parts[1:]))
            assert one == other == fold(maps)
            assert kb.apply(one, b[2]) == f


def test_solve_is_the_plain_solve_where_the_buffer_cannot_bind():
    band, rate = bm.synthetic(60, 3), am.synthetic(60, 40, 12, 3)
    for c, model, evaluate, key in ((band, bm, bm.evaluate, "bit_alloc"), (rate, am, am.evaluate, "budget")):
        small, big = model.total(c, 30 * 64), model.total(c, -30 * 64)
        for limit in ((small + big) // 2, small - 1, small, 10 ** 12):
            plain = model.solve(c, limit)
            sol = kb.solve(lambda t: evaluate(c, t), 2, limit, (0, kb.SIZE_MAX, 0))
            assert (sol["t"], sol["met"], sol["total"]) == (plain["t"], plain["met"], plain["total"])
            assert np.array_equal(sol["per_cf"], plain[key]) and np.array_equal(sol["n_bytes"], plain["n_bytes"])
            assert [p[:2] for p in sol["path"]] == plain["path"]
        # only the buffer: a fifth of the way from the smallest peak to the largest, which binds
        peaks = [kb.scan(evaluate(c, t)[2], 2, (300 << Q, kb.SIZE_MAX, 0))["peak_q16"] for t in (30 * 64, -30 * 64)]
        size = (peaks[0] + (peaks[1] - peaks[0]) // 5) >> Q
        sol = kb.solve(lambda t: evaluate(c, t), 2, 1 << 62, (300 << Q, size, 0))
        assert sol["met"] and sol["bucket"]["peak_q16"] <= size << Q and sol["t"] > -30 * 64
        last_below = [p for p in sol["path"] if p[0] < sol["t"]][-1]
        assert not last_below[3] and last_below[2] > size << Q
        sol = kb.solve(lambda t: evaluate(c, t), 2, 1 << 62, (300 << Q, 0, 0))
        assert not sol["met"] and sol["t"] == 30 * 64 and len(sol["path"]) == 1


def test_pacfile_bucket(A):
    bucket = A.pacfile.bucket
    # 96 kb/s stereo at 48 kHz: 512 bytes a block exactly; at 192 kHz a quarter of that
    assert bucket(96, 2, 48000, 10000) == (512 << Q, 10000, 0) == A.pacfile.Bucket(512 << Q, 10000, 0)
    assert bucket(96, 2, 192000, 1, start_bytes=1) == (128 << Q, 1, 1 << Q)
    # at 44.1 kHz the drain is no whole number of bytes, nor of 1 / 65536: 96000 * 2 * 1024 / (8 * 44100) = 557.2789...
    d = bucket(96, 2, 44100, 0).drain_q16
    assert d == 36521830 and d * 8 * 44100 <= 96000 * 2 * 1024 * 65536 < (d + 1) * 8 * 44100
    for kbps, n_ch, sr, hop in ((Fraction(641, 10), 1, 44100, 1024), ("64.1", 3, 48000, 512), (0.1, 8, 192000, 1024),
                                (320, 6, 96000, 1024), (0, 2, 48000, 1024)):
        got = bucket(kbps, n_ch, sr, 5, hop=hop).drain_q16
        exact = Fraction(kbps) * 1000 * n_ch * hop * 65536 / (8 * sr)
        assert got == kb.drain_q16(kbps, n_ch, sr, hop) and got <= exact < got + 1, (kbps, n_ch, sr, hop)
    assert bucket(96, 2, 48000, 1 << 40, start_bytes=Fraction(3, 2)) == (512 << Q, 1 << 40, 3 << (Q - 1))
    for bad in (dict(kbps_per_channel=-1), dict(kbps_per_channel="x"), dict(kbps_per_channel=None), dict(n_channels=0),
                dict(n_channels=1.5), dict(sample_rate=0), dict(hop=0), dict(buffer_bytes=-1), dict(buffer_bytes=2.5),
                dict(buffer_bytes=(1 << 40) + 1), dict(start_bytes=-1), dict(start_bytes=1001), dict(start_bytes="y"),
                dict(kbps_per_channel=10 ** 30)):
        kw = dict(dict(kbps_per_channel=96, n_channels=2, sample_rate=48000, buffer_bytes=1000), **bad)
        with pytest.raises(ValueError):
            bucket(**kw)


def test_library_exports_the_bucket_calls(A):
    lib = A.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # declared in the companion header that pacx.h includes; the binding keeps its list beside pacx.h's own
    assert '#include "pacx_bucket.h"' in open(os.path.join(root, "include", "pacx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pacx_bucket.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header)) == set(NAMES) == set(A._lib.BUCKET_SIGNATURES)
    assert not set(NAMES) & set(A._lib.SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        args = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(A._lib.BUCKET_SIGNATURES[name][1]) == len(args.split(",")), name
        assert getattr(lib, name).argtypes == A._lib.BUCKET_SIGNATURES[name][1]
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7
    assert [f for f, _ in A._lib.PacxBucket._fields_] == ["drain_q16", "size_bytes", "start_q16"]
    assert A._lib.BUCKET_RESULT == kb.FIELDS and A._lib.BUCKET_Q == Q and A._lib.BUCKET_SIZE_MAX == kb.SIZE_MAX
    for name in ("bucket_scan", "band_solve_bucket", "rate_solve_bucket"):
        assert callable(getattr(A.engine.Encoder, name))
    assert list(inspect.signature(A.engine.Encoder.bucket_scan).parameters) == \
        ["self", "n_bytes", "n_channels", "bucket", "want_level"]
    assert list(inspect.signature(A.engine.Encoder.band_solve_bucket).parameters) == \
        ["self", "curve", "n_channels", "limit_bytes", "bucket", "nmr_lo_db", "nmr_hi_db"]
    assert list(inspect.signature(A.engine.Encoder.rate_solve_bucket).parameters) == \
        ["self", "curve", "flags", "n_channels", "limit_bytes", "bucket", "nmr_lo_db", "nmr_hi_db"]
    assert list(inspect.signature(A.pacfile.encode_stream_abr_buffered).parameters) == \
        ["pcm", "sample_rate", "kbps_per_channel", "buffer_bytes", "drain_kbps_per_channel", "start_bytes",
         "max_kbps_per_channel", "block_switching", "header_samples", "nmr_range_db", "allocation", "use_vq"]
    # a null handle is refused before anything is read
    assert lib.pacx_bucket_scan(None, 0, 1, None, None, None, None, None) == A._lib.E_ARG
    assert lib.pacx_band_solve_bucket(None, 0, 1, None, None, None, 0, None, -30.0, 30.0, None, None, None, None, None,
                                      None) == A._lib.E_ARG
    assert lib.pacx_rate_solve_bucket(None, 0, 1, 8, 1, None, None, None, 0, None, -30.0, 30.0, None, None, None, None,
                                      None, None) == A._lib.E_ARG


def test_refusals_before_gpu_work(A, monkeypatch):
    from audio_codec_amd import context, pacfile, quality
    Encoder = A.engine.Encoder

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    for call in (pacfile.encode_stream_abr_buffered, quality.encode_stream_to_buffer):
        for bad in ("bands", "", None):
            with pytest.raises(ValueError, match="allocation"):
                call(pcm, 44100, 96, 4000, allocation=bad)
        with pytest.raises(NotImplementedError, match="^gain-shape streams: allocation 'band' only$"):
            call(pcm, 44100, 96, 4000, use_vq=True)
        for kw in (dict(kbps_per_channel=0), dict(kbps_per_channel=-96), dict(buffer_bytes=-1), dict(buffer_bytes=0.5),
                   dict(buffer_bytes=(1 << 40) + 1), dict(start_bytes=4001), dict(start_bytes=-1),
                   dict(drain_kbps_per_channel=-1), dict(nmr_range_db=(3, -3)), dict(nmr_range_db=(0.01, 3))):
            with pytest.raises(ValueError):
                call(pcm, 44100, **dict(dict(kbps_per_channel=96, buffer_bytes=4000), **kw))
        for kw in (dict(), dict(allocation="band"), dict(allocation="band", use_vq=True), dict(drain_kbps_per_channel=0),
                   dict(start_bytes=4000)):
            with pytest.raises(AssertionError, match="an encoder was asked for"):
                call(pcm, 44100, 96, 4000, **kw)
    # the triple and the channels of a hop, as the Encoder's methods check them
    for bad in ((1, 2), (1, 2, 3, 4), (1.5, 2, 3), ("a", 2, 3), None, (1, 2, 1 << 63)):
        with pytest.raises(ValueError, match="three integers"):
            Encoder._bucket_struct("bucket_scan", bad)
    b = Encoder._bucket_struct("bucket_scan", np.array([1, 2, 3]))
    assert (b.drain_q16, b.size_bytes, b.start_q16) == (1, 2, 3)
    for n_ch, n_cf in ((0, 4), (-1, 4), (3, 4), (1.5, 3)):
        with pytest.raises(ValueError, match="n_channels"):
            Encoder._hop_channels("bucket_scan", n_ch, n_cf)
    assert Encoder._hop_channels("bucket_scan", 2, 0) == 2 and Encoder._hop_channels("bucket_scan", 3, 12) == 3


def test_the_two_messages(A):
    """an unmet call says which of the two conditions fails at the highest target: the size, in encode_stream_abr's
    words, or -- the size fitting -- the buffer, with the first block above it"""
    from audio_codec_amd import pacfile
    head = b"h" * 77
    n_bytes = np.array([100, 96, 0, 0, 700, 650, 50, 46], np.int32)         # hops of 204, 0, 1358, 104 bytes
    b = pacfile.Bucket(300 << Q, 1200, 150 << Q)
    at_hi = lambda t: n_bytes                                                # noqa: E731
    sol = kb.solve(at_hi, 2, 1665, b, 0, 64)
    assert not sol["met"] and sol["total"] == 1666 and sol["t"] == 64
    want = ("a body of 1665 bytes cannot be reached: at the highest target, 1 dB, it takes 1666 bytes (1743 with the "
            "header), the smallest size this range of targets gives")
    assert kb.refusal(sol, 1665, b, len(head), 1.0) == want == pacfile._unreachable(1665, 1666, 1.0, head)
    sol = kb.solve(at_hi, 2, 1666, b, 0, 64)
    s = sol["bucket"]
    # 150 + 204 = 354, drained to 54, to 0; 1358 arrives in an empty buffer
    assert not sol["met"] and [v >> Q for v in s["level"]] == [354, 54, 1358, 1162] and s["first_over"] == 2
    want = ("a buffer of 1200 bytes cannot be met: at the highest target, 1 dB, the body fits its limit (1666 of 1666 "
            "bytes) but block 2 brings the level to 1358 bytes, the first block above the buffer")
    assert kb.refusal(sol, 1666, b, len(head), 1.0) == want == \
        pacfile._buffer_overflows(b, 2, s["level"][2], 1666, 1666, 1.0)
    # a level that is no whole number of bytes is rounded up: it is above the buffer
    assert pacfile._buffer_overflows(b, 0, (1200 << Q) + 1, 5, 5, -2.5).count("to 1201 bytes") == 1
