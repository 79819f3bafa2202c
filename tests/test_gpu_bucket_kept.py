"""GPU checks of the buffered solve for a stream in chunks (include/pacx_bucket_kept.h).  No tolerance anywhere; outputs
are prefilled with 0xFF bytes.

1. the bytes kernels: row m of pacx_*_bytes_thresholds equals the n_bytes of the single-target pick on the same kept
   curve at target_t[m] -- 0-5 and 255-257 channel-frames (the band kernel holds four a workgroup, the rate kernel
   one), 1, 2, 15 and 31 targets with repeats, targets outside the range and its two ends, G = 1, 2, 257, 3841, 8193, a
   handle with fewer sizes, a rate row at and above the layout's;
2. pacx_bucket_scan_targets: every field equals bucket_model.scan per row, whole and in pieces of 1, 64 and 1000 hops,
   for 1 and 31 targets, on the patterns of tests/test_gpu_bucket.py (restated here);
3. the tree on scans made up on the host: equal to tests/bucket_kept_model.py step by step for levels 1 ... 5;
4. HostStreamRateEncoder.solve_bucket on kept synthetic curves: equal to band_solve_bucket / rate_solve_bucket of the same
   handle on the one-batch curve for chunks of 1, 5, all and more blocks, levels 1, 2, 4, 5, four limits by four
   buffers, and on the curve whose peak rises with the target;
5. streams: encode_stream_abr_buffered_kept equals encode_stream_abr_buffered byte for byte, its two refusals word for
   word; a memmap store; the iterator's pieces;
6. nothing else moves.
"""
import functools

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import bucket_kept_model as bt
import bucket_model as kb
import profile_model as pm
import rate_profile_model as rp
import vq_band_model as vm
import widths_cases as wc
from conftest import load_excerpt

pytestmark = pytest.mark.gpu

GRID, Q = bm.GRID, kb.Q
NARROW, WIDE = (-2 * GRID, 2 * GRID), (-30 * GRID, 30 * GRID)
GRIDS = [(-3 * GRID, -3 * GRID), (17, 18), NARROW, WIDE, (-64 * GRID, 64 * GRID)]      # G = 1, 2, 257, 3841, 8193
T_LO, T_HI = WIDE
FRAMES = [0, 1, 2, 3, 4, 5, 255, 256, 257]       # k_band_bytes_kept: four frames a workgroup; k_rate_bytes_kept: one
TOP = (1 << 62) + (1 << 57)                      # bucket_dev.h: the bound no level reaches


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


def solver(A, nm_bits=12):
    """a scalar encoder on the band tables of band_model.synthetic"""
    return A.context.encoder(44100, 128 / 44.1, 4, nm_bits)


def on_device(enc, kind, c):
    import torch
    keys = ("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps")
    dev = {k: torch.as_tensor(np.ascontiguousarray(c[k]), device=enc.device) for k in keys}
    if kind == "rate":
        dev["row"], dev["sub_stride"] = c["row"], c["sub_stride"]
    return dev


def keep(enc, kind, c, t_lo, t_hi):
    """the curve kept as thresholds, on the device"""
    op = enc.band_thresholds if kind == "band" else enc.rate_thresholds
    return op(on_device(enc, kind, c), t_lo / GRID, t_hi / GRID)


@functools.lru_cache(maxsize=None)
def band_curve(n_cf, seed, t_lo, t_hi, n_cand=16):
    c = pm.planted(n_cf, seed, t_lo, t_hi, cap_scale=0.6)
    if n_cand != 16:                                        # a handle with fewer sizes: the entries beyond hold anything
        c["n_cand"], c["n_mant_size_bits"] = n_cand, {8: 3}[n_cand]
        c["cap_alloc"] = np.minimum(c["cap_alloc"], n_cand)
    return c


@functools.lru_cache(maxsize=None)
def rate_curve(n_cf, seed, t_lo, t_hi, extra=0):
    c = rp.planted(n_cf, seed, t_lo, t_hi)
    if extra:                                               # a row above the layout's: the tail belongs to no unit
        rng = np.random.default_rng(seed)
        c["worst"] = np.concatenate((c["worst"], rng.uniform(-40, 40, (n_cf, extra))), axis=1)
        c["bits"] = np.concatenate((c["bits"], rng.integers(1, 999, (n_cf, extra)).astype(np.int32)), axis=1)
        c["row"] += extra
    return c


# ------------------------------------------------------------------------------------------------ 1. the bytes kernels
def targets_for(n, t_lo, t_hi, seed):
    """n targets: the two ends, one below and one far above the range, a repeat, the rest drawn"""
    rng = np.random.default_rng(seed)
    t = rng.integers(t_lo, t_hi + 1, n)
    fixed = [t_hi, t_lo, t_lo - 1, t_hi + 70000, t_hi]
    t[:min(n, len(fixed))] = fixed[:n]
    if n >= 15:
        t[n - 1] = t[7]                                     # a repeat among the drawn ones
    return t.astype(np.int32)


def check_bytes(enc, kind, kept, t_lo, t_hi, targets, what, picks):
    """the call's rows against the single-target pick at every target (picks: a cache of those per target)"""
    import torch
    n_cf, n = kept["e"].shape[0], len(targets)
    op, pick = (enc.band_bytes_thresholds, enc.band_pick_thresholds) if kind == "band" else \
        (enc.rate_bytes_thresholds, enc.rate_pick_thresholds)
    guard = torch.full((n + 1, n_cf), -1, dtype=torch.int32, device=enc.device)
    out = guard[:n]
    t_dev = torch.as_tensor(targets, device=enc.device)
    assert op(kept, t_dev, out=out) is out
    got = guard.cpu().numpy()
    assert (got[n] == -1).all(), what                       # nothing behind the rows
    for m, t in enumerate(targets):
        at = int(min(max(int(t), t_lo), t_hi))
        if at not in picks:
            picks[at] = pick(kept, at / GRID)["n_bytes"].cpu().numpy()
        assert np.array_equal(got[m], picks[at]), (what, m, int(t))
    # a sequence from the host and a tensor made by the call: the same rows
    again = op(kept, [int(t) for t in targets])
    assert tuple(again.shape) == (n, n_cf) and np.array_equal(again.cpu().numpy(), got[:n]), what


@pytest.mark.parametrize("n_cf", FRAMES)
@pytest.mark.parametrize("kind", ["band", "rate"])
def test_bytes_frame_counts(A, kind, n_cf):
    enc = solver(A)
    t_lo, t_hi = NARROW
    c = band_curve(n_cf, 40 + n_cf, t_lo, t_hi) if kind == "band" else rate_curve(n_cf, 60 + n_cf, t_lo, t_hi)
    kept, picks = keep(enc, kind, c, t_lo, t_hi), {}
    for n in (1, 2, 15, 31):
        check_bytes(enc, kind, kept, t_lo, t_hi, targets_for(n, t_lo, t_hi, n_cf * 32 + n), (kind, n_cf, n), picks)
    if n_cf >= 255:
        assert any(v.any() for v in picks.values())         # conditions on the input: there are records


@pytest.mark.parametrize("t_lo,t_hi", GRIDS)
@pytest.mark.parametrize("kind", ["band", "rate"])
def test_bytes_grids(A, kind, t_lo, t_hi):
    enc = solver(A)
    for n_cf in (5, 257):
        c = band_curve(n_cf, 7, t_lo, t_hi) if kind == "band" else rate_curve(n_cf, 9, t_lo, t_hi)
        kept, picks = keep(enc, kind, c, t_lo, t_hi), {}
        for n in (1, 31):
            check_bytes(enc, kind, kept, t_lo, t_hi, targets_for(n, t_lo, t_hi, n), (kind, n_cf, t_lo, t_hi, n), picks)
        if t_hi - t_lo > 100 and n_cf == 257:
            sizes = {int(v.sum()) for v in picks.values()}
            assert len(sizes) > 3                           # conditions on the input: the targets give different bytes


def test_bytes_with_fewer_sizes_and_rows_above_the_layout(A):
    t_lo, t_hi = NARROW
    enc = solver(A, 3)                                      # eight sizes: the indices 8 ... 15 of a slot count for nothing
    kept = keep(enc, "band", band_curve(37, 5, t_lo, t_hi, n_cand=8), t_lo, t_hi)
    check_bytes(enc, "band", kept, t_lo, t_hi, targets_for(31, t_lo, t_hi, 3), "eight sizes", {})
    enc = solver(A)
    for extra in (0, 1, 77):
        kept = keep(enc, "rate", rate_curve(37, 6, t_lo, t_hi, extra), t_lo, t_hi)
        check_bytes(enc, "rate", kept, t_lo, t_hi, targets_for(31, t_lo, t_hi, extra), ("row + ", extra), {})
    # refusals of the Python layer: no target, too many, a tensor of another type, an out of another shape
    import torch
    for bad in ([], list(range(32)), [0.5], torch.zeros(3, dtype=torch.int64, device=enc.device)):
        with pytest.raises(ValueError, match="rate_bytes_thresholds"):
            enc.rate_bytes_thresholds(kept, bad)
    with pytest.raises(ValueError, match="out is a contiguous int32"):
        enc.rate_bytes_thresholds(kept, [0, 1], out=torch.zeros((2, 36), dtype=torch.int32, device=enc.device))
    # and of the C entry point: n_targets outside [1, 31], before any launch
    ptr = A.engine._ptr
    t = torch.zeros(40, dtype=torch.int32, device=enc.device)
    out = torch.zeros((40, 37), dtype=torch.int32, device=enc.device)
    for n in (0, 32, -1):
        rc = enc.lib.pacx_rate_bytes_thresholds(enc.h, 37, kept["row"], kept["sub_stride"], ptr(kept["e"]),
                                                ptr(kept["bits"]), ptr(kept["steps"]), -2.0, 2.0, n, ptr(t), ptr(out),
                                                enc._stream())
        assert rc == A._lib.E_ARG and b"n_targets" in enc.lib.pacx_last_error(enc.h)


# ------------------------------------------------------------------------------------------------ 2. the scans
HOPS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
CHANNELS = (1, 2, 3, 8)


def burst(n_hops, n_ch, at, size=2000):
    nb = np.zeros(n_hops * n_ch, np.int32)
    nb[at * n_ch:(at + 1) * n_ch] = size
    return nb


def pattern(name, n_hops, n_ch):
    """the patterns of tests/test_gpu_bucket.py, restated -> list of (n_bytes, bucket) of one pattern at one shape"""
    n = n_hops * n_ch
    rng = np.random.default_rng(n_hops * 16 + n_ch)
    if name == "zero":
        return [(np.zeros(n, np.int32), (100 << Q, 1000, 500 << Q)), (np.zeros(n, np.int32), (0, 0, 0))]
    if name == "equal_drain":                               # x_h is the drain exactly: the level never moves
        x = n_ch * (37 + 4)
        return [(np.full(n, 37, np.int32), (x << Q, 5000, 77 << Q))]
    if name == "lone_burst":
        at = sorted({k for k in (0, n_hops - 1, 63, 64, 1023, 1024) if 0 <= k < n_hops})
        return [(burst(n_hops, n_ch, k), ((300 << Q) + 5, 3000, 1000 << Q)) for k in at]
    if name == "empty_run":
        # the level runs out half a hop before hop k: the clamp engages inside a wave (37), at a wave's first hop (64)
        # and at the workgroup's (1024); the burst comes two hops later, into an empty buffer
        out, drain = [], (250 << Q) + 3
        for k in (37, 64, 1024):
            if k < n_hops:
                start = drain * (k - 1) + drain // 2
                out.append((burst(n_hops, n_ch, min(k + 2, n_hops - 1)), (drain, (start >> Q) + 1, start)))
        return out
    if name == "prefix_sum":                                # drain 0 from a full buffer: the largest values there are
        return [(np.full(n, 65535, np.int32), (0, 1 << 40, 1 << 56))]
    if name == "big_drain":                                 # the largest drain: above any hop, up to the largest int64
        nb = rng.integers(0, 3000, n).astype(np.int32)
        return [(nb, (d, 5000, 700 << Q)) for d in (TOP - 1, TOP, (1 << 63) - 1)] + [(nb, ((1 << 56) - 5, 1 << 40, 1 << 56))]
    if name == "ones_and_max":                              # 1 gives 5 bytes, 65535 gives 65539
        nb = rng.choice(np.array([1, 65535, 0], np.int32), n, p=[0.6, 0.2, 0.2])
        return [(nb, ((30000 << Q) + 1, 100000, 0))]
    if name == "negative":                                  # a negative entry counts as 0
        nb = rng.integers(-70000, 3000, n).astype(np.int32)
        nb[::7] = -2 ** 31
        return [(nb, ((40 * n_ch) << Q, 3000, 10 << Q))]
    if name == "twin_peaks":                                # equal peaks in two pieces: the earlier hop stands
        out = []
        for a, b in ((0, 1), (10, 70), (63, 1030), (999, 1000)):
            if b < n_hops:
                nb = burst(n_hops, n_ch, a, 4000)
                nb[b * n_ch:(b + 1) * n_ch] = 4000
                out.append((nb, (1 << 60, 4004 * n_ch, 0)))
        return out
    assert name == "random"
    out = []
    for seed in range(2):
        r = np.random.default_rng([seed, n_hops, n_ch])
        nb = (r.integers(0, 800, n) * (r.random(n) < 0.8)).astype(np.int32)
        mean = int(np.where(nb > 0, nb + 4, 0).sum() * 65536 // max(n_hops, 1))
        size = int(r.integers(0, 4000 * n_ch))
        out.append((nb, (mean + int(r.integers(0, mean // 4 + 1)) - mean // 8, size,
                         0 if seed == 0 else int(r.integers(0, (size << Q) + 1)))))
    return out


PATTERNS = ("zero", "equal_drain", "lone_burst", "empty_run", "prefix_sum", "big_drain", "ones_and_max", "negative",
            "twin_peaks", "random")


def rows_of(n_bytes, n_ch, n):
    """row 0 the pattern, the others the pattern turned by three hops more each: other levels under the same bucket"""
    return np.stack([np.roll(n_bytes, 3 * n_ch * m) for m in range(n)]).astype(np.int32)


def scan_rows(enc, rows, n_ch, bucket, piece):
    """-> int64 [n + 1, 5]: every row's acc after the pieces of `piece` hops in order, and the guard row behind them"""
    import torch
    n, n_cf = rows.shape
    n_hops = n_cf // n_ch
    dev = torch.as_tensor(rows, device=enc.device)
    guard = torch.full((n + 1, 5), -1, dtype=torch.int64, device=enc.device)
    guard[:n] = torch.as_tensor(enc.bucket_no_hop(bucket, n), device=enc.device)
    acc = guard[:n]
    for a in range(0, max(n_hops, 1), piece):
        b = min(a + piece, n_hops)
        assert enc.bucket_scan_targets(dev[:, a * n_ch:b * n_ch], n_ch, bucket[0], bucket[1], a, acc) is acc
    return guard.cpu().numpy()


@pytest.mark.parametrize("name", PATTERNS)
def test_scan_targets_equal_the_model(A, name):
    enc, seen = solver(A), {"cases": 0, "over": 0, "pieces": 0}
    for n_hops in HOPS:
        for n_ch in CHANNELS:
            if n_hops > 1025 and n_ch in (3, 8) and name != "random":
                continue                                    # the model walks every hop in Python
            for i, (n_bytes, bucket) in enumerate(pattern(name, n_hops, n_ch)):
                n = 31 if n_hops in (1, 65, 1025) and n_ch <= 2 else 1
                rows = rows_of(n_bytes, n_ch, n)
                want = np.array([[kb.scan(r, n_ch, bucket)[k] for k in kb.FIELDS] for r in rows], np.int64)
                pieces = [p for p in (1, 64, 1000, 1 << 30) if p >= 64 or n_hops <= 65]
                for piece in pieces:
                    got = scan_rows(enc, rows, n_ch, bucket, piece)
                    assert (got[n] == -1).all() and np.array_equal(got[:n], want), (name, n_hops, n_ch, i, piece)
                    seen["pieces"] += -(-n_hops // piece) > 1
                seen["cases"] += 1
                seen["over"] += int((want[:, 3] >= 0).any())
    print(f"{name}: {seen}")
    assert seen["cases"] >= len(CHANNELS) * 3 and seen["pieces"] > 0
    if name == "twin_peaks":                                # conditions on the pattern: two hops reach the peak
        nb, bucket = pattern(name, 1025, 2)[1]
        s = kb.scan(nb, 2, bucket)
        assert s["peak_hop"] == 10 and s["level"].count(s["peak_q16"]) == 2 and s["level"][70] == s["peak_q16"]


def test_scan_targets_arguments(A):
    import torch
    enc = solver(A)
    ptr = A.engine._ptr
    nb = torch.zeros((31, 8), dtype=torch.int32, device=enc.device)
    acc = torch.as_tensor(enc.bucket_no_hop((0, 10, 0), 31), device=enc.device)

    def rc(n_hops=4, n_ch=2, n=31, rows=nb, stride=8, drain=0, size=10, off=0, a=acc):
        return enc.lib.pacx_bucket_scan_targets(enc.h, n_hops, n_ch, n, ptr(rows) if rows is not None else None, stride,
                                                drain, size, off, ptr(a) if a is not None else None, enc._stream())
    assert rc() == 0 and rc(n_hops=0, rows=None) == 0
    for kw in (dict(n=0), dict(n=32), dict(n_ch=0), dict(n_hops=-1), dict(stride=7), dict(drain=-1), dict(size=-1),
               dict(size=(1 << 40) + 1), dict(off=-1), dict(off=1 << 30), dict(rows=None), dict(a=None)):
        assert rc(**kw) == A._lib.E_ARG, kw
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), enc.bucket_no_hop((0, 10, 0), 31))     # silence from an empty buffer
    with pytest.raises(ValueError, match="bucket_scan_targets: acc"):
        enc.bucket_scan_targets(nb, 2, 0, 10, 0, acc[:30])
    with pytest.raises(ValueError, match="bucket_scan_targets: n_channels"):
        enc.bucket_scan_targets(nb, 3, 0, 10, 0, acc)


# ------------------------------------------------------------------------------------------------ 3. the tree
def made_up(t, seed, size):
    """a scan for target t that no stream gave: whether it fits goes up and down with t"""
    r = np.random.default_rng([seed, t + 100000])
    return {"total": int(r.integers(0, 2000)), "peak_q16": int(r.integers(0, 2 * size << Q)), "peak_hop": int(r.integers(-1, 50)),
            "first_over": int(r.integers(-1, 50)), "end_q16": int(r.integers(0, size << Q))}


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_tree_steps_equal_the_model(A, levels):
    import torch
    enc = solver(A)
    n = (1 << levels) - 1
    tree = None
    for (t_lo, t_hi) in [(-7, -7), (0, 1), (-1, 1), (-128, 128), WIDE, (-4096, 4096)]:
        for seed, limit, size in ((1, 1000, 1000), (2, 1500, 400), (3, 10, 1000), (4, 1 << 40, 1 << 30)):
            bucket = (5 << Q, size, 3 << Q)
            tree = enc.bucket_tree_begin(bucket, t_lo / GRID, t_hi / GRID, levels, tree=tree)
            s, held = bt.begin(t_lo, t_hi), bt.no_hop(bucket[2])
            steps = enc.bucket_tree_passes(t_lo / GRID, t_hi / GRID, levels)
            assert steps == bt.passes(t_lo, t_hi, levels)
            for p in range(steps + 1):                      # one more: a step on an ended solve changes nothing
                tt = tree["target_t"].cpu().numpy().tolist()
                want = bt.targets(s, levels)
                assert tt[:n] == want and tt[n:] == [s["mid"]] * (31 - n), (t_lo, t_hi, seed, p)
                assert np.array_equal(tree["acc"].cpu().numpy(), enc.bucket_no_hop(bucket, 31))
                acc = [made_up(t, seed, size) for t in want]
                tree["acc"][:n] = torch.as_tensor(np.array([[a[k] for k in kb.FIELDS] for a in acc], np.int64),
                                                  device=enc.device)
                s, held, _ = bt.step(s, held, acc, limit, size, levels)
                assert enc.bucket_tree_step(limit, bucket, levels, tree) is tree
                got = enc.bucket_tree_result(tree)
                assert (got["target_nmr_db"] * GRID, got["met"], got["total_bytes"]) == \
                    (s["mid"], bool(s["met"]), held["total"]), (t_lo, t_hi, seed, p)
                assert {k: got["bucket"][k] for k in kb.FIELDS} == held, (t_lo, t_hi, seed, p)
                if p == steps - 1:
                    assert s["done"]
                    final = dict(got)
            assert got == final
    # refusals: levels, the limit, the bucket
    for bad in (0, 6, 2.5, None):
        with pytest.raises(ValueError, match="levels"):
            enc.bucket_tree_begin((0, 10, 0), levels=bad)
    with pytest.raises(ValueError, match="limit_bytes"):
        enc.bucket_tree_step(-1, (0, 10, 0), levels, tree)
    with pytest.raises(A._lib.PacxError, match="a bucket has"):
        enc.bucket_tree_begin((0, 10, 11 << Q), levels=levels)
    b = A._lib.PacxBucket(0, 10, 0)
    import ctypes
    for lv in (0, 6):
        assert enc.lib.pacx_bucket_tree_begin(enc.h, ctypes.byref(b), -30.0, 30.0, lv, A.engine._ptr(tree["state"]),
                                              A.engine._ptr(tree["target_t"]), A.engine._ptr(tree["acc"]),
                                              enc._stream()) == A._lib.E_ARG
    assert enc.lib.pacx_bucket_tree_begin(enc.h, ctypes.byref(b), -30.0, 30.0, 4, None, A.engine._ptr(tree["target_t"]),
                                          A.engine._ptr(tree["acc"]), enc._stream()) == A._lib.E_ARG


# ------------------------------------------------------------------------------------------------ 4. the solve in chunks
def evaluator(kind, c):
    return functools.lru_cache(maxsize=None)((lambda t: bm.evaluate(c, t)) if kind == "band" else
                                             (lambda t: am.evaluate(c, t)))


def hop_peaks(ev, n_ch, drain, t):
    s = kb.scan(ev(t)[2], n_ch, (drain, kb.SIZE_MAX, 0))
    return max(kb.hop_bytes(ev(t)[2], n_ch), default=0), -(-s["peak_q16"] >> Q)


def grid_of(ev, n_cf, n_ch):
    """four limits crossed with four buffers, as tests/test_gpu_bucket.py draws them -> list of (limit, bucket)"""
    small, big = ev(T_HI)[0], ev(T_LO)[0]
    drain = (ev(0)[0] << Q) // max(n_cf // n_ch, 1) + 12345
    hop_hi, peak_hi = hop_peaks(ev, n_ch, drain, T_HI)
    _, peak_lo = hop_peaks(ev, n_ch, drain, T_LO)
    mid = (peak_hi + peak_lo) // 2
    buckets = [(drain, max(hop_hi - 1, 0), 0), (drain, peak_hi, 0), (drain, mid, (mid // 3) << Q), (drain, 1 << 40, 1 << 50)]
    limits = [v for v in (small - 1, small, (small + big) // 2, 10 ** 12) if v >= 0]
    return [(limit, b) for limit in limits for b in buckets]


def chunked_on(A, enc, kind, c, n_ch, chunk_hops, t_lo=T_LO, t_hi=T_HI):
    """a HostStreamRateEncoder whose store holds the curve c, kept chunk by chunk as analyse() lays a stream's curves
    out: the blocks in chunks of chunk_hops, the last two a chunk of their own"""
    import torch
    from audio_codec_amd import pacfile, streaming
    n_cf = len(c["cap"] if kind == "band" else c["steps"])
    blocks = n_cf // n_ch
    assert blocks >= 2 and n_cf % n_ch == 0
    hr = streaming.HostStreamRateEncoder(enc, n_ch, chunk_hops, 128 / 44.1, nmr_lo_db=t_lo / GRID, nmr_hi_db=t_hi / GRID,
                                         allocation="band" if kind == "band" else "budget")
    if kind == "rate":                                      # the synthetic curve's row, not the cap rate's
        row, sub = c["row"], c["sub_stride"]

        class Path(pacfile._BudgetPath):
            def layout(self, max_bits_per_sample):
                return row, {"row": row, "sub_stride": sub}
        hr.path = Path(enc)
    kept = keep(enc, kind, c, t_lo, t_hi)
    hr.keep_curves()
    hr._kept_buffers()
    per_block = n_ch * hr.path.kept_bytes_per_cf(hr.max_bps)
    hr.kept = {"store": np.zeros(blocks * per_block, np.uint8), "hops": blocks - 2, "per_block": per_block}
    for before, n in hr._kept_pieces():
        buf = torch.zeros(n * per_block, dtype=torch.uint8, device=enc.device)
        views = hr.path.kept_views(buf, n * n_ch, hr.max_bps)
        for a in hr.path.kind.kept:
            views[a.key].copy_(kept[a.key][before * n_ch:(before + n) * n_ch])
        hr.kept["store"][before * per_block:(before + n) * per_block] = buf.cpu().numpy()
    return hr


def one_batch(enc, kind, dev, n_ch, limit, bucket, lo_db=-30, hi_db=30):
    if kind == "band":
        return enc.band_solve_bucket(dev, n_ch, limit, bucket, lo_db, hi_db)
    return enc.rate_solve_bucket(dev, None, n_ch, limit, bucket, lo_db, hi_db)


def same_answer(got, ref, what):
    assert set(got) == {"target_nmr_db", "met", "total_bytes", "bucket"}
    assert (got["target_nmr_db"], got["met"], got["total_bytes"]) == \
        (ref["target_nmr_db"], ref["met"], ref["total_bytes"]), (what, got, {k: ref[k] for k in got})
    assert got["bucket"] == ref["bucket"], (what, got["bucket"], ref["bucket"])


N_CH, BLOCKS = 2, 13                                        # 11 blocks and the tail's two: chunks of 5 leave one over
LEVELS = (1, 2, 4, 5)


@pytest.mark.parametrize("chunk_hops", [1, 5, 11, 40])      # 1, 5, all and more blocks
@pytest.mark.parametrize("kind", ["band", "rate"])
def test_solve_bucket_equals_the_one_batch_solve(A, kind, chunk_hops):
    enc = solver(A)
    n_cf = BLOCKS * N_CH
    c = pm.planted(n_cf, 13, T_LO, T_HI) if kind == "band" else rp.planted(n_cf, 13, T_LO, T_HI)
    dev, ev = on_device(enc, kind, c), evaluator(kind, c)
    hr = chunked_on(A, enc, kind, c, N_CH, chunk_hops)
    turn = [1, 5, 11, 40].index(chunk_hops)
    met, bound = 0, 0
    for i, (limit, b) in enumerate(grid_of(ev, n_cf, N_CH)):
        levels = LEVELS[(i + i // 4 + turn) % 4]            # every depth meets every limit, every buffer and every chunking
        ref = one_batch(enc, kind, dev, N_CH, limit, b)
        same_answer(hr.solve_bucket(limit, b, levels), ref, (kind, chunk_hops, levels, limit, b))
        met += ref["met"]
        bound += ref["met"] and ref["bucket"]["total"] <= limit and \
            ref["target_nmr_db"] > one_batch(enc, kind, dev, N_CH, limit, (b[0], 1 << 40, 0))["target_nmr_db"]
    print(f"{kind} chunks of {chunk_hops}: {met} of 16 met, the buffer moved the target in {bound}")
    assert 0 < met < 16 and bound > 0                       # conditions on the input
    limit, b = grid_of(ev, n_cf, N_CH)[9]
    assert hr.solve_bucket(limit, b) == hr.solve_bucket(limit, b, 4)                # the default depth; the object is reusable
    # another range, narrower than the thresholds are kept for, is not what the object solves: its own range, off zero
    hr = chunked_on(A, enc, kind, c, N_CH, chunk_hops, -2 * GRID, 352)
    for levels in LEVELS:
        same_answer(hr.solve_bucket(limit, b, levels), one_batch(enc, kind, dev, N_CH, limit, b, -2, 5.5), (levels, "narrow"))


def rising_curve():
    """The curve of tests/test_gpu_bucket.py's test_the_bisections_path_is_pinned, restated: the bytes, and with them the
    peak, RISE with the target.  Four stereo hops of one long unit per channel-frame with three steps; in the hops 1 and
    2 the step in the middle is the large one and passes from -5 dB on, the small first step from +5 dB on."""
    n_cf, row, sub = 8, 24, 3
    worst, bits = np.full((n_cf, row), np.nan), np.zeros((n_cf, row), np.int32)
    steps = np.full((n_cf, 8), -1, np.int32)
    steps[:, 0] = 2
    for cf in range(n_cf):
        odd = cf // 2 in (1, 2)
        worst[cf, :3] = (5.0, -5.0, -40.0) if odd else (20.0, 0.0, -20.0)
        bits[cf, :3] = (200, 6000, 300) if odd else (100, 180, 300)
    return {"worst": worst, "bits": bits, "steps": steps, "row": row, "sub_stride": sub}


@pytest.mark.parametrize("levels", LEVELS)
def test_the_bisections_path_is_pinned_in_chunks(A, levels):
    c, n_ch, b = rising_curve(), 2, (100 << Q, 500, 0)
    ev = evaluator("rate", c)
    peak = lambda t: kb.scan(ev(t)[2], n_ch, b)["peak_q16"]                  # noqa: E731
    assert peak(-321) <= 500 << Q < peak(-320) and peak(319) > 500 << Q >= peak(320) and peak(T_LO) <= 500 << Q
    ref = kb.solve(ev, n_ch, 1 << 62, b, T_LO, T_HI)
    assert [p[0] for p in ref["path"][:6]] == [1920, -1, 959, 479, 239, 359] and ref["t"] == 320
    enc = solver(A)
    for chunk_hops in (1, 2):
        got = chunked_on(A, enc, "rate", c, n_ch, chunk_hops).solve_bucket(1 << 62, b, levels)
        same_answer(got, one_batch(enc, "rate", on_device(enc, "rate", c), n_ch, 1 << 62, b), (levels, chunk_hops))
        assert got["target_nmr_db"] == 5.0 and got["met"]
        # the answer lies above the lowest target that fits: the lowest of all fits, and so does every one below -5 dB
        fits = lambda t: kb.scan(ev(t)[2], n_ch, b)["peak_q16"] <= 500 << Q      # noqa: E731
        assert fits(T_LO) and fits(-321) and T_LO < -321 < got["target_nmr_db"] * GRID


# ------------------------------------------------------------------------------------------------ 5. streams
def excerpt(name, hops=24):
    ex = load_excerpt(name)
    return np.ascontiguousarray(ex["pcm"][:hops * 1024]), int(ex["sr"])


STREAMS = {"castanet6": wc.stream, "harpsichord24": lambda: excerpt("harpsichord"), "vq12": vm.fixture_stream}
KBPS = 96
CASES = [("harpsichord24", "budget", 5), ("harpsichord24", "band", 4096), ("castanet6", "band", 1), ("castanet6", "budget", 4),
         ("vq12", "band", 3)]


@functools.lru_cache(maxsize=None)
def binding(A, name, allocation):
    """a buffer that binds on the stream and is met, found with the one-batch call -> (pcm, sample rate, keywords, the
    buffer, its one-batch bytes and target, the average-rate target)"""
    pcm, sr = STREAMS[name]()
    use_vq = name == "vq12"
    kw = dict(block_switching=True, allocation=allocation, use_vq=use_vq)
    one = lambda size: A.pacfile._encode_stream_buffered(pcm, sr, KBPS, size, None, 0, 320, True, None, (-30, 30),   # noqa: E731
                                                         allocation, use_vq)
    _, whole, _, limit, _, _ = one(1 << 40)
    for share in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3):
        size = int(share * (whole["bucket"]["peak_q16"] >> Q))
        try:
            data, sol, _, _, _, _ = one(size)
        except ValueError:
            break
        if sol["target_nmr_db"] > whole["target_nmr_db"]:
            return pcm, sr, kw, size, data, sol["target_nmr_db"], whole["target_nmr_db"]
    raise AssertionError("conditions on the input: no buffer binds and is met")


@pytest.mark.parametrize("name,allocation,chunk_hops", CASES)
def test_streams(A, name, allocation, chunk_hops):
    pcm, sr, kw, size, want, target, plain_target = binding(A, name, allocation)
    kept, buffered = A.pacfile.encode_stream_abr_buffered_kept, A.pacfile.encode_stream_abr_buffered
    assert target > plain_target                            # the buffer binds: not encode_stream_abr_kept's target
    got = kept(pcm, sr, KBPS, size, chunk_hops=chunk_hops, **kw)
    assert got == want == buffered(pcm, sr, KBPS, size, **kw)
    plain = A.pacfile.encode_stream_abr_kept(pcm, sr, KBPS, chunk_hops=chunk_hops, block_switching=True,
                                             use_vq=kw["use_vq"], allocation=allocation)
    assert plain != got and kept(pcm, sr, KBPS, 1 << 40, chunk_hops=chunk_hops, **kw) == plain
    for levels in (1, 5):
        assert kept(pcm, sr, KBPS, size, chunk_hops=chunk_hops, levels=levels, **kw) == want
    # a start level and a drain of its own
    more = dict(drain_kbps_per_channel=80, start_bytes=size // 4)
    try:
        ref = buffered(pcm, sr, KBPS, size, **more, **kw)
    except ValueError as e:
        with pytest.raises(ValueError) as err:
            kept(pcm, sr, KBPS, size, chunk_hops=chunk_hops, **more, **kw)
        assert str(err.value) == str(e)
    else:
        assert kept(pcm, sr, KBPS, size, chunk_hops=chunk_hops, **more, **kw) == ref
    # the size fails at the highest target; the buffer fails there although the size fits: the one-batch call's words
    for args, what in (((4.0, 1 << 40), "a body of"), ((KBPS, 8), "a buffer of 8 bytes cannot be met")):
        with pytest.raises(ValueError, match="^" + what) as ours:
            kept(pcm, sr, *args, chunk_hops=chunk_hops, **kw)
        with pytest.raises(ValueError) as theirs:
            buffered(pcm, sr, *args, **kw)
        assert str(ours.value) == str(theirs.value)
    assert "fits its limit" in str(ours.value)              # the second message: the size fits at 30 dB


@pytest.mark.parametrize("allocation", ["band", "budget"])
def test_a_memmap_store_and_the_iterators_pieces(A, tmp_path, allocation):
    from audio_codec_amd import streaming
    pcm, sr, kw, size, want, _, _ = binding(A, "harpsichord24", allocation)
    cp = A.pacfile._rate_coding_params(pcm, sr, 320, None)
    head = A.pacfile.header_bytes(cp)                      # once: it fills in the params it is given
    need = (len(pcm) // 1024 + 2) * pcm.shape[1] * A.pacfile._kept_bytes_per_cf(cp, allocation)
    store = np.memmap(tmp_path / "curves.bin", dtype=np.uint8, mode="w+", shape=(need + 5,))
    store[:] = 0xFF
    src = np.memmap(tmp_path / "pcm.bin", dtype=np.int16, mode="w+", shape=pcm.shape)
    src[:] = pcm
    pieces = list(A.pacfile.iter_encode_abr_buffered_kept(src, sr, KBPS, size, chunk_hops=7, curve_store=store, **kw))
    assert len(pieces) == 1 + 4 + 1 and all(isinstance(p, bytes) for p in pieces)   # header, 7 + 7 + 7 + 3 blocks, tail
    assert b"".join(pieces) == want and pieces[0] == head == want[:len(head)]
    assert (np.asarray(store[need:]) == 0xFF).all() and (np.asarray(store[:need]) != 0xFF).any()
    with pytest.raises(ValueError, match="curve_store.*it holds %d" % (need - 1)):
        A.pacfile.encode_stream_abr_buffered_kept(src, sr, KBPS, size, chunk_hops=7, curve_store=store[:need - 1], **kw)
    assert callable(streaming.HostStreamRateEncoder.solve_bucket)


# ------------------------------------------------------------------------------------------------ 6. nothing else moves
def test_nothing_else_moves(A):
    """a buffered solve on an object between two average-rate encodes of the same object, and beside the handle's other
    calls: encode_stream_abr_kept's bytes, encode_pack and band_solve_bucket give what they gave before"""
    from audio_codec_amd import streaming
    pcm, sr, kw, size, want, target, plain_target = binding(A, "harpsichord24", "band")
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None, False)
    head = A.pacfile.header_bytes(cp)
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    limit = int(np.floor(KBPS * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    b = A.pacfile.bucket(KBPS, n_ch, sr, size)
    curve = enc.band_curve(view, flags, cp.targetBitsPerSample)
    hr = streaming.HostStreamRateEncoder(enc, n_ch, 5, cp.targetBitsPerSample, block_switching=True)
    hr.keep_curves().analyse(pcm)

    def snapshot():
        out = {}
        sol = hr.solve(limit)
        out["abr_kept"] = head + b"".join(bytes(p) for p in hr.encode(pcm, sol["target_nmr_db"]))
        for k, v in enc.band_solve_bucket(curve, n_ch, limit, tuple(b)).items():
            out["band_solve_bucket", k] = v.cpu().numpy() if hasattr(v, "cpu") else v
        e = enc.encode_pack(view, flags)
        body, total = enc.gather_body(e["payload"], e["n_bytes"])
        out["encode_pack"] = body[:int(total.item())].cpu().numpy().tobytes()
        return out

    before = snapshot()
    assert before["abr_kept"] == A.pacfile.encode_stream_abr_kept(pcm, sr, KBPS, chunk_hops=5, block_switching=True)
    sol = hr.solve_bucket(limit, b)
    assert sol["target_nmr_db"] == target == before["band_solve_bucket", "target_nmr_db"] and sol["met"]
    assert sol["bucket"] == before["band_solve_bucket", "bucket"]
    assert head + b"".join(bytes(p) for p in hr.encode(pcm, sol["target_nmr_db"])) == want
    after = snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
