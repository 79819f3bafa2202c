"""The leaky bucket on the GPU (pacx_bucket_scan, pacx_band_solve_bucket / pacx_rate_solve_bucket; Encoder.bucket_scan,
band_solve_bucket, rate_solve_bucket; pacfile.encode_stream_abr_buffered, quality.encode_stream_to_buffer and
buffer_report) against tests/bucket_model.py, which walks the hops one after the other in Python integers and runs
band_model's / abr_model's bisection with the bucket's peak as a second condition.

Bars.  Everything here is integers and comparisons on given arrays: every result field, every level, every output of
a solve equals the model's.  No window anywhere.  A buffered stream is, byte for byte, the stream of encode_stream_nmr
at the target found, and its level stays within the buffer.
"""
import ctypes
import functools

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import bucket_model as kb
import profile_model as pm
import rate_profile_model as rp
import segment_model as sm
import vq_band_model as vm
import widths_cases as wc
from conftest import load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

Q = kb.Q
KINDS = ("band", "rate")
HOPS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)      # a wave and the workgroup's 1024 hops, one off either way
CHANNELS = (1, 2, 3, 8)
T_LO, T_HI = -30 * 64, 30 * 64
TOP = (1 << 62) + (1 << 57)                                     # bucket_dev.h: the bound no level reaches


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


_ENC = {}


def encoder(A):
    """a handle whose band tables are the synthetic curves' (band_model.synthetic: 44100 Hz), kept"""
    if "enc" not in _ENC:
        _ENC["enc"] = A.engine.Encoder(44100, 128 / 44.1)
    return _ENC["enc"]


# ------------------------------------------------------------------------------------------------ 1. the scan
def c_scan(A, enc, n_bytes, n_ch, bucket, n_hops=None, want_level=True, n_bytes_null=False):
    """pacx_bucket_scan itself, its outputs prefilled with 0xFF and eight words longer than they need be
    -> (rc, level words, result words)"""
    import torch
    ptr = A.engine._ptr
    nb = torch.as_tensor(np.ascontiguousarray(n_bytes, np.int32), device=enc.device)
    n_hops = len(n_bytes) // n_ch if n_hops is None else n_hops
    level = torch.full((max(min(n_hops, 1 << 20), 0) + 8,), -1, dtype=torch.int64, device=enc.device)
    result = torch.full((len(kb.FIELDS) + 8,), -1, dtype=torch.int64, device=enc.device)
    b = None if bucket is None else A._lib.PacxBucket(*bucket)
    rc = enc.lib.pacx_bucket_scan(enc.h, n_hops, n_ch, None if n_bytes_null else ptr(nb),
                                  None if b is None else ctypes.byref(b), ptr(level) if want_level else None,
                                  ptr(result), enc._stream())
    torch.cuda.synchronize()
    return rc, level.cpu().numpy(), result.cpu().numpy()


def check_scan(A, enc, n_bytes, n_ch, bucket, what):
    ref = kb.scan(n_bytes, n_ch, bucket)
    rc, level, result = c_scan(A, enc, n_bytes, n_ch, bucket)
    assert rc == 0, (what, enc.lib.pacx_last_error(enc.h))
    n_hops = len(n_bytes) // n_ch
    got = dict(zip(kb.FIELDS, (int(v) for v in result)))
    assert got == {k: ref[k] for k in kb.FIELDS}, (what, got, {k: ref[k] for k in kb.FIELDS})
    assert (result[len(kb.FIELDS):] == -1).all() and (level[n_hops:] == -1).all(), what      # nothing behind the outputs
    assert np.array_equal(level[:n_hops], np.array(ref["level"], np.int64).reshape(-1)), what
    return ref


def burst(n_hops, n_ch, at, size=2000):
    nb = np.zeros(n_hops * n_ch, np.int32)
    nb[at * n_ch:(at + 1) * n_ch] = size
    return nb


def pattern(name, n_hops, n_ch):
    """-> list of (n_bytes, bucket) of one pattern at one shape"""
    n = n_hops * n_ch
    rng = np.random.default_rng(n_hops * 16 + n_ch)
    if name == "zero":
        return [(np.zeros(n, np.int32), (100 << Q, 1000, 500 << Q)), (np.zeros(n, np.int32), (0, 0, 0))]
    if name == "equal_drain":                               # x_h is the drain exactly: the level never moves
        x = n_ch * (37 + 4)
        return [(np.full(n, 37, np.int32), (x << Q, 5000, start)) for start in (0, 77 << Q)]
    if name == "lone_burst":
        at = sorted({k for k in (0, n_hops - 1, 63, 64, 1023, 1024) if 0 <= k < n_hops})
        return [(burst(n_hops, n_ch, k), ((300 << Q) + 5, 3000, 1000 << Q)) for k in at]
    if name == "empty_run":
        # the level runs out half a hop before hop k: the clamp engages inside a wave (37), at a wave's first hop
        # (64) and at a workgroup's (1024); the burst comes two hops later, into an empty buffer
        out, drain = [], (250 << Q) + 3
        for k in (37, 64, 1024):
            if k < n_hops:
                start = drain * (k - 1) + drain // 2
                out.append((burst(n_hops, n_ch, min(k + 2, n_hops - 1)), (drain, (start >> Q) + 1, start)))
        return out
    if name == "prefix_sum":                                # drain 0 from a full buffer: the largest values there are
        return [(np.full(n, 65535, np.int32), (0, 1 << 40, 1 << 56))]
    if name == "big_drain":                                 # larger than any hop, up to the largest int64
        nb = rng.integers(0, 3000, n).astype(np.int32)
        return [(nb, (d, 5000, 700 << Q)) for d in (10 ** 6 << Q, TOP - 1, TOP, TOP + 1, (1 << 63) - 1)] + \
            [(nb, (d, 1 << 40, 1 << 56)) for d in (TOP, 1 << 55, (1 << 56) - 5)]
    if name == "ones_and_max":                              # 1 gives 5 bytes, 65535 gives 65539
        nb = rng.choice(np.array([1, 65535, 0], np.int32), n, p=[0.6, 0.2, 0.2])
        return [(nb, ((30000 << Q) + 1, 100000, 0)), (np.ones(n, np.int32), (5 * n_ch << Q, 5 * n_ch, 0))]
    if name == "negative":                                  # a negative entry counts as 0
        nb = rng.integers(-70000, 3000, n).astype(np.int32)
        nb[::7] = -2 ** 31
        return [(nb, ((40 * n_ch) << Q, 3000, 10 << Q)), (-np.ones(n, np.int32), (1, 10, 10 << Q))]
    assert name == "random"
    out = []
    for seed in range(3):
        r = np.random.default_rng([seed, n_hops, n_ch])
        nb = (r.integers(0, 800, n) * (r.random(n) < 0.8)).astype(np.int32)
        mean = int(np.where(nb > 0, nb + 4, 0).sum() * 65536 // max(n_hops, 1))
        size = int(r.integers(0, 4000 * n_ch))
        out.append((nb, (mean + int(r.integers(0, mean // 4 + 1)) - mean // 8, size,
                         0 if seed == 0 else int(r.integers(0, (size << Q) + 1)))))
    return out


PATTERNS = ("zero", "equal_drain", "lone_burst", "empty_run", "prefix_sum", "big_drain", "ones_and_max", "negative",
            "random")


@pytest.mark.parametrize("name", PATTERNS)
def test_scan_equals_the_model(A, name):
    enc, seen = encoder(A), {"over": 0, "emptied": 0, "cases": 0}
    for n_hops in HOPS:
        for n_ch in CHANNELS:
            for i, (n_bytes, bucket) in enumerate(pattern(name, n_hops, n_ch)):
                ref = check_scan(A, enc, n_bytes, n_ch, bucket, (name, n_hops, n_ch, i))
                seen["cases"] += 1
                seen["over"] += ref["first_over"] >= 0
                seen["emptied"] += any(v < bucket[0] for v in ref["level"])
    print(f"{name}: {seen}")
    assert seen["cases"] >= len(CHANNELS) * 3
    if name == "empty_run":                                 # conditions on the pattern: the clamp does engage, at the border
        for k in (37, 64, 1024):
            n_bytes, b = pattern(name, 2049, 2)[(37, 64, 1024).index(k)]
            lv = kb.scan(n_bytes, 2, b)["level"]
            assert lv[k - 1] - b[0] < 0 <= lv[k - 2] - b[0] and lv[k] == 0 and lv[k + 2] == 4008 << Q
    if name == "prefix_sum":
        n_bytes, b = pattern(name, 4097, 8)[0]
        assert kb.scan(n_bytes, 8, b)["peak_q16"] == (1 << 56) + (4097 * 8 * 65539 << Q)


def test_scan_no_hops_and_the_python_call(A):
    enc = encoder(A)
    rc, _, result = c_scan(A, enc, [], 3, (5, 1 << 40, 1 << 56), n_bytes_null=True)
    assert rc == 0 and result[:5].tolist() == [0, 1 << 56, -1, -1, 1 << 56]
    rc, _, result = c_scan(A, enc, [7, 8, 9, 10], 2, (5 << Q, 20, 3 << Q), want_level=False)           # level may be NULL
    # hops of 23 and 27 bytes: 3 + 23 = 26, which is above 20; 21 + 27 = 48; 43 stay
    assert rc == 0 and result[:5].tolist() == [50, 48 << Q, 1, 0, 43 << Q]
    rng = np.random.default_rng(5)
    for n_hops, n_ch in ((0, 2), (1, 1), (1025, 3)):
        nb = rng.integers(-5, 900, n_hops * n_ch).astype(np.int32)
        b = A.pacfile.bucket(96, n_ch, 44100, 6000 * n_ch, start_bytes=100)
        ref = kb.scan(nb, n_ch, b)
        import torch
        for given in (nb, nb.tolist(), torch.as_tensor(nb, device=enc.device), nb.reshape(-1, n_ch)):
            got = enc.bucket_scan(given, n_ch, b, want_level=True)
            assert {k: got[k] for k in kb.FIELDS} == {k: ref[k] for k in kb.FIELDS}
            assert got["level"].dtype == torch.int64 and got["level"].cpu().numpy().tolist() == ref["level"]
            assert got["peak_bytes"] == ref["peak_q16"] / 65536 and got["end_bytes"] == ref["end_q16"] / 65536
        assert "level" not in enc.bucket_scan(nb, n_ch, b)
    with pytest.raises(ValueError, match="n_channels"):
        enc.bucket_scan([1, 2, 3], 2, (0, 0, 0))
    with pytest.raises(A._lib.PacxError, match="bucket"):
        enc.bucket_scan([1, 2], 2, (-1, 0, 0))
    vq = A.engine.Encoder(44100, 128 / 44.1, use_vq=True)                # defined on arrays alone: any handle
    assert vq.bucket_scan([10, 20, 0, 30], 2, (20 << Q, 30, 0))["peak_q16"] == 52 << Q          # 38, then 18 + 34
    vq.close()


def test_scan_in_pieces(A):
    enc = encoder(A)
    rng = np.random.default_rng(9)
    n_hops, n_ch = 2049, 2
    nb = (rng.integers(0, 900, n_hops * n_ch) * (rng.random(n_hops * n_ch) < 0.7)).astype(np.int32)
    b = ((780 << Q) + 777, 2500, 100 << Q)
    whole = check_scan(A, enc, nb, n_ch, b, "whole")
    # it overflows in the second piece, runs empty and peaks in the third; at the cuts the level is back inside the
    # buffer, where a piece has to start (the domain of include/pacx.h)
    assert 1 <= whole["first_over"] < 64 and any(v < b[0] for v in whole["level"]) and 64 <= whole["peak_hop"] < 1000
    assert all(whole["level"][c - 1] - b[0] <= b[1] << Q for c in (1, 64, 1000))
    level, total, start, peak, peak_hop, over = [], 0, b[2], b[2], -1, -1
    for a, e in zip((0, 1, 64, 1000), (1, 64, 1000, n_hops)):
        part = enc.bucket_scan(nb[a * n_ch:e * n_ch], n_ch, (b[0], b[1], start), want_level=True)
        level += part["level"].cpu().numpy().tolist()
        total += part["total"]
        if part["peak_q16"] > peak:
            peak, peak_hop = part["peak_q16"], a + part["peak_hop"]
        if over < 0 and part["first_over"] >= 0:
            over = a + part["first_over"]
        start = part["end_q16"]
    assert (level, total, peak, peak_hop, over, start) == \
        (whole["level"], whole["total"], whole["peak_q16"], whole["peak_hop"], whole["first_over"], whole["end_q16"])


def test_scan_arguments(A):
    enc, E = encoder(A), A._lib.E_ARG
    nb, good = [10, 20, 30, 40], (5, 100, 7)
    assert c_scan(A, enc, nb, 2, good)[0] == 0
    for n_ch in (0, -1):
        assert c_scan(A, enc, nb, n_ch, good, n_hops=2)[0] == E
    for n_hops, n_ch in ((-1, 2), ((1 << 30) + 1, 1), (1 << 30, 2), ((1 << 29) + 1, 2), (1 << 62, 4), (3, 1 << 30)):
        assert c_scan(A, enc, nb, n_ch, good, n_hops=n_hops)[0] == E, (n_hops, n_ch)
        assert b"2^30" in enc.lib.pacx_last_error(enc.h)
    for bad in ((-1, 100, 7), (5, -1, 0), (5, (1 << 40) + 1, 7), (5, 100, -1), (5, 100, (100 << Q) + 1), (5, 0, 1),
                (-(1 << 63), 100, 7)):
        assert c_scan(A, enc, nb, 2, bad)[0] == E, bad
        assert b"bucket" in enc.lib.pacx_last_error(enc.h)
    assert c_scan(A, enc, nb, 2, None)[0] == E and b"null pointer" in enc.lib.pacx_last_error(enc.h)
    assert c_scan(A, enc, nb, 2, good, n_bytes_null=True)[0] == E
    b = A._lib.PacxBucket(*good)
    assert enc.lib.pacx_bucket_scan(enc.h, 0, 1, None, ctypes.byref(b), None, None, None) == E       # no result
    # the ends of the domain are inside it
    for ok in ((0, 0, 0), (5, 1 << 40, 1 << 56), ((1 << 63) - 1, 100, 100 << Q)):
        assert c_scan(A, enc, nb, 2, ok)[0] == 0, ok


# ------------------------------------------------------------------------------------------------ 2. the solves
def on_device(enc, kind, c):
    import torch
    keys = ("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps")
    dev = {k: torch.as_tensor(np.ascontiguousarray(c[k]), device=enc.device) for k in keys}
    if kind == "rate":
        dev["row"], dev["sub_stride"] = c["row"], c["sub_stride"]
    return dev


def evaluator(kind, c):
    """evaluate(t) of the model, every target taken once"""
    return functools.lru_cache(maxsize=None)((lambda t: bm.evaluate(c, t)) if kind == "band" else
                                             (lambda t: am.evaluate(c, t)))


def gpu_solve(enc, kind, dev, n_ch, limit, bucket, lo_db=-30, hi_db=30):
    if kind == "band":
        return enc.band_solve_bucket(dev, n_ch, limit, bucket, lo_db, hi_db)
    return enc.rate_solve_bucket(dev, None, n_ch, limit, bucket, lo_db, hi_db)


def same_solve(kind, sol, ref, what):
    """a buffered solve's dict against the model's: everything equal"""
    assert isinstance(sol["target_nmr_db"], float) and isinstance(sol["met"], bool) and isinstance(sol["total_bytes"], int)
    got = (sol["target_nmr_db"] * 64, sol["met"], sol["total_bytes"])
    assert got == (ref["t"], bool(ref["met"]), ref["total"]), (what, got, (ref["t"], ref["met"], ref["total"]))
    assert np.array_equal(sol["bit_alloc" if kind == "band" else "budget"].cpu().numpy(), ref["per_cf"]), what
    assert np.array_equal(sol["n_bytes"].cpu().numpy(), ref["n_bytes"]), what
    assert np.array_equal(sol["capped"].cpu().numpy(), ref["capped"]), what
    assert {k: sol["bucket"][k] for k in kb.FIELDS} == {k: ref["bucket"][k] for k in kb.FIELDS}, what


def hop_peaks(ev, n_ch, drain, t):
    """(the largest hop, the peak level from an empty buffer) in bytes at target t, rounded up"""
    s = kb.scan(ev(t)[2], n_ch, (drain, kb.SIZE_MAX, 0))
    return max(kb.hop_bytes(ev(t)[2], n_ch), default=0), -(-s["peak_q16"] >> Q)


def material(kind, source, n_cf):
    if source == "synthetic":
        return sm.synthetic(kind, n_cf, 11)
    return pm.planted(n_cf, 13, T_LO, T_HI) if kind == "band" else rp.planted(n_cf, 13, T_LO, T_HI)


def grid_of(ev, n_cf, n_ch):
    """four limits crossed with four buffers -> list of (limit, bucket): one byte less than the highest target takes
    (none without records), exactly that, the midpoint of the smallest and the largest body, more than anything takes;
    a buffer one byte below the largest hop at the highest target (never met), exactly the peak there, half way to
    the peak at the lowest target from a third full, and one nothing reaches.  The drain: a little above the mean
    hop at 0 dB, no whole number of bytes"""
    small, big = ev(T_HI)[0], ev(T_LO)[0]
    n_hops = n_cf // n_ch
    drain = (ev(0)[0] << Q) // max(n_hops, 1) + 12345
    hop_hi, peak_hi = hop_peaks(ev, n_ch, drain, T_HI)
    _, peak_lo = hop_peaks(ev, n_ch, drain, T_LO)
    mid = (peak_hi + peak_lo) // 2
    buckets = [(drain, max(hop_hi - 1, 0), 0), (drain, peak_hi, 0), (drain, mid, (mid // 3) << Q), (drain, 1 << 40, 1 << 50)]
    limits = [v for v in (small - 1, small, (small + big) // 2, 10 ** 12) if v >= 0]
    return [(limit, b) for limit in limits for b in buckets]


CH_OF = {0: 2, 1: 1, 3: 3, 4: 2, 5: 1, 255: 1, 256: 2, 257: 1, 2050: 2}     # 2050 stereo: two trips of the scan


@pytest.mark.parametrize("n_cf", sorted(CH_OF))
@pytest.mark.parametrize("source", ["synthetic", "planted"])
@pytest.mark.parametrize("kind", KINDS)
def test_solves_equal_the_model(A, kind, source, n_cf):
    c, n_ch = material(kind, source, n_cf), CH_OF[n_cf]
    enc = encoder(A)
    dev, ev = on_device(enc, kind, c), evaluator(kind, c)
    met, bound = 0, 0
    for limit, b in grid_of(ev, n_cf, n_ch):
        ref = kb.solve(ev, n_ch, limit, b, T_LO, T_HI)
        same_solve(kind, gpu_solve(enc, kind, dev, n_ch, limit, b), ref, (limit, b))
        met += ref["met"]
        bound += ref["met"] and any(total <= limit and not ok for _, total, _, ok in ref["path"])
    print(f"{kind} {source} {n_cf}: {met} met, the buffer decided a probe in {bound}")
    if n_cf >= 255:
        assert 0 < met < 16 and bound > 0                   # both answers, and probes only the buffer refused
    # another range, one target wide and off zero
    limit, b = grid_of(ev, n_cf, n_ch)[-2]
    for lo_db, hi_db in ((-2, 5.5), (0.078125, 0.078125)):
        ref = kb.solve(ev, n_ch, limit, b, int(lo_db * 64), int(hi_db * 64))
        same_solve(kind, gpu_solve(enc, kind, dev, n_ch, limit, b, lo_db, hi_db), ref, (lo_db, hi_db))


@pytest.mark.parametrize("kind", KINDS)
def test_reductions(A, kind):
    n_cf, n_ch = 2050, 2
    c = sm.synthetic(kind, n_cf, 7)
    enc = encoder(A)
    dev, ev = on_device(enc, kind, c), evaluator(kind, c)
    small, big = ev(T_HI)[0], ev(T_LO)[0]
    drain = (ev(0)[0] << Q) // (n_cf // n_ch) + 999
    # a buffer nothing reaches: every array and the result are the plain solve's of the same handle
    for limit in ((small + big) // 2, small - 1, small, 10 ** 12):
        sol = gpu_solve(enc, kind, dev, n_ch, limit, (drain, 1 << 40, 0))
        plain = enc.band_solve(dev, limit) if kind == "band" else enc.rate_solve(dev, None, limit)
        assert set(plain) | {"bucket"} == set(sol)
        for k, v in plain.items():
            assert np.array_equal(sol[k].cpu().numpy(), v.cpu().numpy()) if hasattr(v, "cpu") else sol[k] == v, (limit, k)
        assert sol["bucket"]["total"] == sol["total_bytes"] and sol["bucket"]["first_over"] == -1
    # a limit nothing reaches: only the buffer binds
    hop_hi, peak_hi = hop_peaks(ev, n_ch, drain, T_HI)
    _, peak_lo = hop_peaks(ev, n_ch, drain, T_LO)
    assert hop_hi <= peak_hi < peak_lo
    size = peak_hi + (peak_lo - peak_hi) // 4
    sol = gpu_solve(enc, kind, dev, n_ch, 1 << 62, (drain, size, 0))
    ref = kb.solve(ev, n_ch, 1 << 62, (drain, size, 0), T_LO, T_HI)
    same_solve(kind, sol, ref, "limit 2^62")
    assert sol["met"] and -30 < sol["target_nmr_db"] < 30 and sol["bucket"]["peak_q16"] <= size << Q
    below = [p for p in ref["path"] if p[0] < ref["t"]][-1]
    assert not below[3] and below[2] > size << Q              # fits failed at the last target tried below, on the peak
    # a buffer below the largest hop at the highest target: met = 0 there
    sol = gpu_solve(enc, kind, dev, n_ch, 1 << 62, (drain, hop_hi - 1, 0))
    same_solve(kind, sol, kb.solve(ev, n_ch, 1 << 62, (drain, hop_hi - 1, 0), T_LO, T_HI), "too small")
    assert not sol["met"] and sol["target_nmr_db"] == 30.0 and sol["bucket"]["first_over"] >= 0


def rising_curve():
    """A rate curve on which the bytes, and with them the peak, RISE with the target: four stereo hops of one long
    unit per channel-frame with three steps.  In the hops 1 and 2 the step in the middle is the large one and passes
    from -5 dB on, the small first step from +5 dB on: 42 bytes a frame below -5 dB, 755 in [-5, 5) dB, 30 from 5 dB."""
    n_cf, row, sub = 8, 24, 3
    worst, bits = np.full((n_cf, row), np.nan), np.zeros((n_cf, row), np.int32)
    steps = np.full((n_cf, 8), -1, np.int32)
    steps[:, 0] = 2
    for cf in range(n_cf):
        odd = cf // 2 in (1, 2)
        worst[cf, :3] = (5.0, -5.0, -40.0) if odd else (20.0, 0.0, -20.0)
        bits[cf, :3] = (200, 6000, 300) if odd else (100, 180, 300)
    return {"worst": worst, "bits": bits, "steps": steps, "row": row, "sub_stride": sub}


def test_the_bisections_path_is_pinned(A):
    c, n_ch = rising_curve(), 2
    ev = evaluator("rate", c)
    b = (100 << Q, 500, 0)
    peak = lambda t: kb.scan(ev(t)[2], n_ch, b)["peak_q16"]                  # noqa: E731
    # conditions on the input: the peak rises with the target at -5 dB, the buffer holds below -5 dB and from 5 dB on
    assert peak(-321) < peak(-320) and peak(-321) <= 500 << Q < peak(-320)
    assert all(peak(t) <= 500 << Q for t in (T_LO, -640, -321, 320, T_HI)) and peak(319) > 500 << Q
    ref = kb.solve(ev, n_ch, 1 << 62, b, T_LO, T_HI)
    assert [p[0] for p in ref["path"][:6]] == [1920, -1, 959, 479, 239, 359]
    assert ref["t"] == 320 and ref["met"]                   # the bisection's answer, 35 dB above the lowest that fits
    enc = encoder(A)
    sol = gpu_solve(enc, "rate", on_device(enc, "rate", c), n_ch, 1 << 62, b)
    same_solve("rate", sol, ref, "rising")
    assert sol["target_nmr_db"] == 5.0 and sol["n_bytes"].cpu().numpy().tolist() == [23, 23, 26, 26, 26, 26, 23, 23]


@pytest.mark.parametrize("kind", KINDS)
def test_solves_queued_without_a_wait(A, kind):
    """two buffered solves with a plain one between them, queued on one handle and one stream through the C entry
    points and read back only after the third: they share the handle's workspace table"""
    import torch
    n_cf, n_ch = 2050, 2
    c = sm.synthetic(kind, n_cf, 7)
    enc = encoder(A)
    dev, ev = on_device(enc, kind, c), evaluator(kind, c)
    small, big = ev(T_HI)[0], ev(T_LO)[0]
    drain = (ev(0)[0] << Q) // (n_cf // n_ch) + 999
    hop_hi, peak_hi = hop_peaks(ev, n_ch, drain, T_HI)
    _, peak_lo = hop_peaks(ev, n_ch, drain, T_LO)
    jobs = [((small + big) // 2, (drain, peak_hi + (peak_lo - peak_hi) // 4, 0)), (small + (big - small) // 5, None),
            (1 << 62, (drain, peak_hi + (peak_lo - peak_hi) // 2, 100 << Q))]
    gpu_solve(enc, kind, dev, n_ch, jobs[0][0], jobs[0][1])         # the handle's state is allocated: no wait below
    ptr = A.engine._ptr
    arrays = [ptr(dev[k]) for k in (("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps"))]
    head = [] if kind == "band" else [int(dev["row"]), int(dev["sub_stride"])]
    width = enc.band_stride if kind == "band" else 8
    queued = []
    for limit, b in jobs:
        out = [torch.zeros((n_cf, width), dtype=torch.int32, device=enc.device),
               torch.zeros((n_cf,), dtype=torch.int32, device=enc.device),
               torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device),
               torch.full((4, 4), -1, dtype=torch.int32, device=enc.device)]
        if b is None:
            rc = getattr(enc.lib, f"pacx_{kind}_solve")(
                enc.h, n_cf, *head, *arrays, limit, -30.0, 30.0, *(ptr(t) for t in out), enc._stream())
        else:
            rc = getattr(enc.lib, f"pacx_{kind}_solve_bucket")(
                enc.h, n_cf, n_ch, *head, *arrays, limit, ctypes.byref(A._lib.PacxBucket(*b)), -30.0, 30.0,
                *(ptr(t) for t in out[:3]), ptr(out[3]), ptr(out[3][1:]), enc._stream())
        assert rc == 0, enc.lib.pacx_last_error(enc.h)
        queued.append(out)
    torch.cuda.synchronize()
    targets = []
    for (limit, b), out in zip(jobs, queued):
        ref = kb.solve(ev, n_ch, limit, b or (0, 1 << 40, 0), T_LO, T_HI)
        res = out[3].cpu().numpy()
        assert (int(res[0, 0]), int(res[0, 1]), int(res[:1, 2:].copy().view(np.int64)[0, 0])) == \
            (ref["t"], ref["met"], ref["total"]), (limit, b)
        if b is not None:
            words = res[1:].reshape(-1).view(np.int64)
            assert dict(zip(kb.FIELDS, words.tolist())) == {k: ref["bucket"][k] for k in kb.FIELDS} and words[5] == -1
        else:
            assert (res[1:] == -1).all()
        for t, want in zip(out, (ref["per_cf"], ref["n_bytes"], ref["capped"])):
            assert np.array_equal(t.cpu().numpy().astype(np.asarray(want).dtype), want), (limit, b)
        targets.append(ref["t"])
    assert len(set(targets)) == 3                           # three answers of their own


def test_solve_arguments(A):
    import torch
    enc, E = encoder(A), A._lib.E_ARG
    ptr = A.engine._ptr
    n_cf = 6
    band, rate = on_device(enc, "band", sm.synthetic("band", n_cf, 3)), on_device(enc, "rate", sm.synthetic("rate", n_cf, 3))
    alloc = torch.zeros((n_cf, enc.band_stride), dtype=torch.int32, device=enc.device)
    budget = torch.zeros((n_cf, 8), dtype=torch.int32, device=enc.device)
    nby = torch.zeros((n_cf,), dtype=torch.int32, device=enc.device)
    cpd = torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device)
    res = torch.zeros((4, 4), dtype=torch.int32, device=enc.device)
    good = (100 << Q, 5000, 0)

    def band_call(n=n_cf, n_ch=2, limit=10 ** 6, b=good, lo=-30.0, hi=30.0, result=res, bres=res[1:], h=enc):
        return h.lib.pacx_band_solve_bucket(
            h.h, n, n_ch, ptr(band["nmr"]), ptr(band["cap"]), ptr(band["cap_alloc"]), limit,
            None if b is None else ctypes.byref(A._lib.PacxBucket(*b)), lo, hi, ptr(alloc), ptr(nby), ptr(cpd),
            ptr(result), ptr(bres), None)

    def rate_call(n=n_cf, n_ch=2, limit=10 ** 6, b=good, lo=-30.0, hi=30.0, result=res, bres=res[1:], h=enc, row=None):
        return h.lib.pacx_rate_solve_bucket(
            h.h, n, n_ch, int(rate["row"]) if row is None else row, int(rate["sub_stride"]), ptr(rate["worst"]),
            ptr(rate["bits"]), ptr(rate["steps"]), limit, None if b is None else ctypes.byref(A._lib.PacxBucket(*b)),
            lo, hi, ptr(budget), ptr(nby), ptr(cpd), ptr(result), ptr(bres), None)

    for call in (band_call, rate_call):
        assert call() == 0
        for n_ch in (0, -1, 4, 5):                          # n_cf is no multiple of it, or it is no count
            assert call(n_ch=n_ch) == E and b"multiple" in enc.lib.pacx_last_error(enc.h), n_ch
        assert call(n_ch=1) == 0 and call(n_ch=3) == 0 and call(n_ch=6) == 0
        assert call(n=-2) == E
        assert call(limit=-1) == E and b"negative" in enc.lib.pacx_last_error(enc.h)
        assert call(b=None) == E and b"null pointer" in enc.lib.pacx_last_error(enc.h)
        assert call(result=None) == E and call(bres=None) == E
        for bad in ((-1, 100, 7), (5, -1, 0), (5, (1 << 40) + 1, 7), (5, 100, -1), (5, 100, (100 << Q) + 1)):
            assert call(b=bad) == E and b"bucket" in enc.lib.pacx_last_error(enc.h), bad
        for lo, hi in ((float("nan"), 3.0), (3.0, -3.0), (-30.01, 30.0), (-2e6, 0.0)):           # the plain solves' rules
            assert call(lo=lo, hi=hi) == E
    assert rate_call(row=7 * int(rate["sub_stride"])) == E
    torch.cuda.synchronize()
    vq = A.engine.Encoder(44100, 128 / 44.1, use_vq=True)
    assert band_call(h=vq) == A._lib.E_UNSUPPORTED and rate_call(h=vq) == A._lib.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        vq.band_solve_bucket(band, 2, 10 ** 6, good)
    vq.close()
    # the Python layer: the channels and the triple before the call, the bucket's numbers by the library
    for n_ch in (0, 4, 1.5):
        with pytest.raises(ValueError, match="n_channels"):
            enc.band_solve_bucket(band, n_ch, 10 ** 6, good)
    with pytest.raises(ValueError, match="three integers"):
        enc.rate_solve_bucket(rate, None, 2, 10 ** 6, (1, 2))
    for limit in (-1, 2.5):
        with pytest.raises(ValueError, match="limit_bytes"):
            enc.band_solve_bucket(band, 2, limit, good)
    with pytest.raises(A._lib.PacxError, match="bucket"):
        enc.band_solve_bucket(band, 2, 10 ** 6, (5, 100, (100 << Q) + 1))
    assert enc.band_solve_bucket(band, 2, 10 ** 6, A.pacfile.bucket(96, 2, 44100, 5000))["met"]


# ------------------------------------------------------------------------------------------------ 3. streams
def excerpt(name, hops=24):
    ex = load_excerpt(name)
    return np.ascontiguousarray(ex["pcm"][:hops * 1024]), int(ex["sr"])


STREAMS = {"castanet6": wc.stream, "harpsichord24": lambda: excerpt("harpsichord"), "vq12": vm.fixture_stream}
KBPS = 96
_OWN = {}


def own(A, name, allocation):
    """the stream's handle, its curve on the device and the model's evaluate on the curve's arrays"""
    key = name, allocation
    if key not in _OWN:
        pcm, sr = STREAMS[name]()
        use_vq = name == "vq12"
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None, use_vq)
        tables = bm.tables(po.make_params(sr, pcm.shape[1], 320))
        if allocation == "band":
            dev = (enc.vq_band_curve if use_vq else enc.band_curve)(view, flags, cp.targetBitsPerSample)
            host = bm.with_arrays(tables, *(dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")))
        else:
            dev = enc.rate_curve(view, flags, cp.targetBitsPerSample)
            host = dict({k: dev[k].cpu().numpy() for k in ("worst", "bits", "steps")}, row=dev["row"],
                        sub_stride=dev["sub_stride"])
        _OWN[key] = {"pcm": pcm, "sr": sr, "use_vq": use_vq, "cp": cp, "enc": enc, "view": view, "flags": flags,
                     "dev": dev, "ev": evaluator("band" if allocation == "band" else "rate", host),
                     "head": A.pacfile.header_bytes(cp)}
    return _OWN[key]


def record_sizes(A, data):
    _, pos = A.pacfile.parse_header(data)
    return A.pacfile.record_chain(data, pos, bm.PAYLOAD_STRIDE)[1]


CASES = [("castanet6", "budget"), ("castanet6", "band"), ("harpsichord24", "budget"), ("harpsichord24", "band"),
         ("vq12", "band")]


@pytest.mark.parametrize("name,allocation", CASES)
def test_streams(A, name, allocation):
    g = own(A, name, allocation)
    pcm, sr, use_vq, ev = g["pcm"], g["sr"], g["use_vq"], g["ev"]
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    limit = int(np.floor(KBPS * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    kw = dict(block_switching=True, allocation=allocation, use_vq=use_vq)
    buffered, to_buffer = A.pacfile.encode_stream_abr_buffered, A.quality.encode_stream_to_buffer
    drain = kb.drain_q16(KBPS, n_ch, sr)
    # a buffer nothing reaches: the average-rate stream
    plain = A.pacfile.encode_stream_vq_abr(pcm, sr, KBPS, block_switching=True) if use_vq else \
        A.pacfile.encode_stream_abr(pcm, sr, KBPS, block_switching=True, allocation=allocation)
    assert buffered(pcm, sr, KBPS, 1 << 40, **kw) == plain
    whole = kb.solve(ev, n_ch, limit, (drain, 1 << 40, 0), T_LO, T_HI)
    assert whole["met"]
    # a buffer that binds: a fraction of the peak level at the whole-stream target, not below the largest hop at 30 dB
    hop_hi = max(kb.hop_bytes(ev(T_HI)[2], n_ch))
    found = None
    for share in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4):
        size = max(int(share * (whole["bucket"]["peak_q16"] >> Q)), hop_hi)
        ref = kb.solve(ev, n_ch, limit, (drain, size, 0), T_LO, T_HI)
        if ref["met"] and ref["t"] > whole["t"]:
            found = share, size, ref
            break
    assert found is not None                                # conditions on the input: the buffer binds and is met
    share, size, ref = found
    data, info = to_buffer(pcm, sr, KBPS, size, **kw)
    print(f"{name} {allocation}: whole stream {whole['t'] / 64:g} dB with a peak of {whole['bucket']['peak_q16'] >> Q} "
          f"bytes; a buffer of {size} ({share:g} of it): {info['target_nmr_db']:g} dB, peak {info['peak_bytes']:.1f} at "
          f"block {info['peak_block']}, {info['mean_kbps_per_channel']:.1f} kb/s, at most "
          f"{info['max_kbps_per_channel_seen']:.1f}")
    assert data == buffered(pcm, sr, KBPS, size, **kw)
    assert info["target_nmr_db"] * 64 == ref["t"] and info["limit_bytes"] == limit and info["bucket"] == (drain, size, 0)
    at = A.pacfile.encode_stream_vq_nmr(pcm, sr, info["target_nmr_db"], block_switching=True) if use_vq else \
        A.pacfile.encode_stream_nmr(pcm, sr, info["target_nmr_db"], block_switching=True, allocation=allocation)
    assert data == at
    predicted = info["n_bytes"].reshape(-1)
    assert np.array_equal(predicted, ref["n_bytes"])
    assert record_sizes(A, data) == predicted[predicted > 0].tolist()          # the second pass wrote what was predicted
    s = kb.scan(predicted, n_ch, (drain, size, 0))
    assert info["total_bytes"] == s["total"] == ref["total"] <= limit
    assert (info["level_bytes"] * 65536).astype(np.int64).tolist() == s["level"] and len(s["level"]) == blocks
    assert info["peak_bytes"] * 65536 == s["peak_q16"] <= size << Q and info["peak_block"] == s["peak_hop"]
    assert info["end_bytes"] * 65536 == s["end_q16"]
    below = [p for p in ref["path"] if p[0] < ref["t"]][-1]
    assert not below[3]                                     # fits fails at the last target the bisection tried below
    if name == "harpsichord24":                             # no hop dropped: the finished bytes give the same levels
        assert (predicted > 0).all()
        rep = A.quality.buffer_report(data, KBPS, size)
        assert rep["bucket"] == info["bucket"] and rep["blocks"] == blocks and rep["fits"] and rep["first_over"] == -1
        assert np.array_equal(rep["level_bytes"], info["level_bytes"]) and rep["total_bytes"] == info["total_bytes"]
        assert (rep["peak_bytes"], rep["peak_block"], rep["end_bytes"]) == \
            (info["peak_bytes"], info["peak_block"], info["end_bytes"])
        assert rep["mean_kbps_per_channel"] == info["mean_kbps_per_channel"]
        tight = A.quality.buffer_report(plain, KBPS, size)  # the average-rate stream does not play through it
        assert not tight["fits"] and tight["first_over"] == kb.scan(whole["n_bytes"], n_ch, (drain, size, 0))["first_over"]
    # a buffer below the largest hop at the highest target, and a size below the smallest body: the model's messages
    small = (drain, hop_hi - 1, 0)
    with pytest.raises(ValueError) as err:
        buffered(pcm, sr, KBPS, hop_hi - 1, **kw)
    unmet = kb.solve(ev, n_ch, limit, small, T_LO, T_HI)
    assert not unmet["met"] and unmet["total"] <= limit
    assert str(err.value) == kb.refusal(unmet, limit, small, len(g["head"]), 30.0)
    low = 4.0
    low_limit = int(np.floor(low * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    low_bucket = (kb.drain_q16(low, n_ch, sr), 1 << 40, 0)
    unmet = kb.solve(ev, n_ch, low_limit, low_bucket, T_LO, T_HI)
    assert not unmet["met"] and unmet["total"] > low_limit
    with pytest.raises(ValueError) as err:
        buffered(pcm, sr, low, 1 << 40, **kw)
    assert str(err.value) == kb.refusal(unmet, low_limit, low_bucket, len(g["head"]), 30.0)


def test_nothing_else_moves(A):
    """buffered solves use a state of their own in the handle's workspace table: encode_pack, band_solve and band_pick
    on the same handle give what they gave before"""
    g = own(A, "castanet6", "band")
    enc, band, view, flags, ev = g["enc"], g["dev"], g["view"], g["flags"], g["ev"]
    limit = (ev(T_HI)[0] + ev(T_LO)[0]) // 2

    def snapshot():
        out = {}
        for name, sol in (("band_solve", enc.band_solve(band, limit)), ("band_pick", enc.band_pick(band, -3.0))):
            for k, v in sol.items():
                out[name, k] = v.cpu().numpy() if hasattr(v, "cpu") else v
        e = enc.encode_pack(view, flags)
        body, total = enc.gather_body(e["payload"], e["n_bytes"])
        out["encode_pack", "body"] = body[:int(total.item())].cpu().numpy().tobytes()
        return out

    before = snapshot()
    n_ch = g["pcm"].shape[1]
    for b in ((300 << Q, 1 << 40, 0), (300 << Q, 2000, 0), (0, 0, 0)):
        same_solve("band", enc.band_solve_bucket(band, n_ch, limit, b), kb.solve(ev, n_ch, limit, b, T_LO, T_HI), b)
    after = snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
