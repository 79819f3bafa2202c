"""Per-block targets under a leaky bucket on the GPU (pacx_bucket_through, pacx_band_solve_bucket_pinned /
pacx_rate_solve_bucket_pinned; Encoder.bucket_through, band_solve_bucket_pinned, rate_solve_bucket_pinned;
pacfile.encode_stream_abr_pinned, quality.encode_stream_to_buffer_pinned) against tests/pin_model.py, which walks the
recursion and the phases in Python integers over bucket_model.scan.

Bars.  Everything here is integers and comparisons on given arrays: every level through a hop, every result field, every
output of a solve equals the model's.  No window anywhere.  A pinned stream holds, block for block, the records of
encode_stream_nmr at that block's target, and its level stays within the buffer.
"""
import ctypes
import functools

import numpy as np
import pytest

import band_model as bm
import bucket_model as kb
import pin_model as pn
import segment_model as sm
import test_gpu_bucket as tb
from conftest import load_excerpt
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

Q = kb.Q
KINDS = tb.KINDS
T_LO, T_HI = tb.T_LO, tb.T_HI
STEPS = (1, 64, T_HI - T_LO)                                    # the full grid, a dB, the whole range
PHASES = (1, 2, 8, 16)


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


# ------------------------------------------------------------------------------------------------ 1. the level through a hop
def c_through(A, enc, n_bytes, n_ch, bucket, want_level=True):
    """pacx_bucket_through itself, its outputs prefilled with 0xFF and eight words longer than they need be
    -> (rc, level words, through words, result words)"""
    import torch
    ptr = A.engine._ptr
    nb = torch.as_tensor(np.ascontiguousarray(n_bytes, np.int32), device=enc.device)
    n_hops = len(n_bytes) // n_ch
    level = torch.full((n_hops + 8,), -1, dtype=torch.int64, device=enc.device)
    through = torch.full((n_hops + 8,), -1, dtype=torch.int64, device=enc.device)
    result = torch.full((len(kb.FIELDS) + 8,), -1, dtype=torch.int64, device=enc.device)
    b = A._lib.PacxBucket(*bucket)
    rc = enc.lib.pacx_bucket_through(enc.h, n_hops, n_ch, ptr(nb) if len(n_bytes) else None, ctypes.byref(b),
                                     ptr(level) if want_level else None, ptr(through), ptr(result), enc._stream())
    torch.cuda.synchronize()
    return rc, level.cpu().numpy(), through.cpu().numpy(), result.cpu().numpy()


def check_through(A, enc, n_bytes, n_ch, bucket, what):
    thr, ref = pn.through(n_bytes, n_ch, bucket)
    rc, level, through, result = c_through(A, enc, n_bytes, n_ch, bucket)
    assert rc == 0, (what, enc.lib.pacx_last_error(enc.h))
    n_hops = len(n_bytes) // n_ch
    got = dict(zip(kb.FIELDS, (int(v) for v in result)))
    assert got == {k: ref[k] for k in kb.FIELDS}, (what, got, {k: ref[k] for k in kb.FIELDS})
    assert (result[len(kb.FIELDS):] == -1).all() and (level[n_hops:] == -1).all() and (through[n_hops:] == -1).all(), what
    assert np.array_equal(level[:n_hops], np.array(ref["level"], np.int64).reshape(-1)), what
    assert np.array_equal(through[:n_hops], np.array(thr, np.int64).reshape(-1)), what
    return thr, ref


def mirrored(n_bytes, n_ch):
    """the hops in reverse order: what engages at a wave's or the workgroup's first hop forwards does so at the last
    one backwards"""
    return np.ascontiguousarray(np.asarray(n_bytes).reshape(-1, n_ch)[::-1]).reshape(-1)


@pytest.mark.parametrize("name", tb.PATTERNS)
def test_through_equals_the_model(A, name):
    enc, seen = tb.encoder(A), {"over": 0, "emptied_backwards": 0, "cases": 0}
    for n_hops in tb.HOPS:
        for n_ch in tb.CHANNELS:
            for i, (n_bytes, bucket) in enumerate(tb.pattern(name, n_hops, n_ch)):
                for nb in (n_bytes, mirrored(n_bytes, n_ch)):
                    thr, ref = check_through(A, enc, nb, n_ch, bucket, (name, n_hops, n_ch, i))
                    X = [x << Q for x in kb.hop_bytes(nb, n_ch)]
                    seen["cases"] += 1
                    seen["over"] += any(t > bucket[1] << Q for t in thr)
                    # R_h = X_h: what lies behind the hop has drained away before it counts
                    seen["emptied_backwards"] += any(t - lv == 0 and x > 0 for t, lv, x in zip(thr[:-1], ref["level"], X))
    print(f"{name}: {seen}")
    assert seen["cases"] >= len(tb.CHANNELS) * 6
    if name == "random":                                    # conditions on the pattern: backwards too, the clamp engages
        assert seen["emptied_backwards"] > 0 and seen["over"] > 0      # at some hops and not at others
    if name == "lone_burst":
        n_bytes, b = tb.pattern(name, 2049, 2)[-2]                                  # the burst at hop 1024
        thr = pn.through(n_bytes, 2, b)[0]
        # the start level of 1000 bytes counts for the hops it has not drained away from (1000 / 300 of them); the hop
        # before the burst lies in the stretch that ends with it
        assert thr[1024] == 4008 << Q and thr[0] == 1000 << Q and thr[5] == 0 and thr[1023] == (4008 << Q) - b[0]
        back = pn.through(mirrored(n_bytes, 2), 2, b)[0]
        assert back[1024] == 4008 << Q and back[1023] == (4008 << Q) - b[0] and back[1022] == (4008 << Q) - 2 * b[0]


def test_through_no_hops_and_the_python_call(A):
    import torch
    enc = tb.encoder(A)
    rc, _, _, result = c_through(A, enc, [], 3, (5, 1 << 40, 1 << 56))
    assert rc == 0 and result[:5].tolist() == [0, 1 << 56, -1, -1, 1 << 56]
    # hops of 23 and 27 bytes from 3: F = 3, 21; R = 23 + (27 - 5), 27: through = 48, 48; level may be NULL
    rc, _, through, result = c_through(A, enc, [7, 8, 9, 10], 2, (5 << Q, 20, 3 << Q), want_level=False)
    assert rc == 0 and result[:5].tolist() == [50, 48 << Q, 1, 0, 43 << Q] and through[:2].tolist() == [48 << Q, 48 << Q]
    rng = np.random.default_rng(5)
    for n_hops, n_ch in ((0, 2), (1, 1), (1025, 3)):
        nb = rng.integers(-5, 900, n_hops * n_ch).astype(np.int32)
        b = A.pacfile.bucket(96, n_ch, 44100, 6000 * n_ch, start_bytes=100)
        thr, ref = pn.through(nb, n_ch, b)
        for given in (nb, nb.tolist(), torch.as_tensor(nb, device=enc.device), nb.reshape(-1, n_ch)):
            got = enc.bucket_through(given, n_ch, b, want_level=True)
            assert {k: got[k] for k in kb.FIELDS} == {k: ref[k] for k in kb.FIELDS}
            assert got["through"].dtype == torch.int64 and got["through"].cpu().numpy().tolist() == thr
            assert got["level"].cpu().numpy().tolist() == ref["level"]
            assert got == dict(enc.bucket_scan(given, n_ch, b), through=got["through"], level=got["level"])
        assert "level" not in enc.bucket_through(nb, n_ch, b)
    with pytest.raises(ValueError, match="n_channels"):
        enc.bucket_through([1, 2, 3], 2, (0, 0, 0))
    with pytest.raises(A._lib.PacxError, match="bucket"):
        enc.bucket_through([1, 2], 2, (-1, 0, 0))
    E, good = A._lib.E_ARG, A._lib.PacxBucket(5, 100, 7)
    nb = torch.as_tensor(np.array([1, 2], np.int32), device=enc.device)
    out = torch.zeros((8,), dtype=torch.int64, device=enc.device)
    ptr = A.engine._ptr
    assert enc.lib.pacx_bucket_through(enc.h, 2, 1, ptr(nb), ctypes.byref(good), None, None, ptr(out), None) == E
    assert b"null pointer" in enc.lib.pacx_last_error(enc.h)                           # no through
    assert enc.lib.pacx_bucket_through(enc.h, 2, 1, ptr(nb), ctypes.byref(good), None, ptr(out), None, None) == E
    assert enc.lib.pacx_bucket_through(enc.h, 2, 1, ptr(nb), None, None, ptr(out), ptr(out[2:]), None) == E
    assert enc.lib.pacx_bucket_through(enc.h, (1 << 30) + 1, 1, ptr(nb), ctypes.byref(good), None, ptr(out), ptr(out[2:]),
                                       None) == E and b"2^30" in enc.lib.pacx_last_error(enc.h)
    vq = A.engine.Encoder(44100, 128 / 44.1, use_vq=True)                # defined on arrays alone: any handle
    assert vq.bucket_through([10, 20, 0, 30], 2, (20 << Q, 30, 0))["through"].cpu().tolist() == [52 << Q, 52 << Q]
    vq.close()


# ------------------------------------------------------------------------------------------------ 2. the solves
def gpu_solve(enc, kind, dev, n_ch, limit, bucket, step, phases, lo_db=-30, hi_db=30):
    if kind == "band":
        return enc.band_solve_bucket_pinned(dev, n_ch, limit, bucket, lo_db, hi_db, step / 64, phases)
    return enc.rate_solve_bucket_pinned(dev, None, n_ch, limit, bucket, lo_db, hi_db, step / 64, phases)


def same_solve(kind, sol, ref, what):
    """a pinned solve's dict against the model's: everything equal"""
    assert isinstance(sol["target_nmr_db"], float) and isinstance(sol["met"], bool) and isinstance(sol["total_bytes"], int)
    got = (sol["target_nmr_db"] * 64, sol["met"], sol["total_bytes"], sol["phases"], sol["open"])
    want = (ref["t"], bool(ref["met"]), ref["total"], ref["phases"], bool(ref["open"]))
    assert got == want, (what, got, want)
    assert sol["target_t"].cpu().numpy().tolist() == ref["target_t"], what
    assert sol["phase_of"].cpu().numpy().tolist() == ref["phase_of"], what
    assert np.array_equal(sol["bit_alloc" if kind == "band" else "budget"].cpu().numpy(), ref["per_cf"]), what
    assert np.array_equal(sol["n_bytes"].cpu().numpy(), ref["n_bytes"]), what
    assert np.array_equal(sol["capped"].cpu().numpy(), ref["capped"]), what
    assert {k: sol["bucket"][k] for k in kb.FIELDS} == {k: ref["bucket"][k] for k in kb.FIELDS}, what


def solve_cases(kind, source, n_cf):
    """test_gpu_bucket's four limits by four buffers, the three steps and the four phase counts spread over them so
    that every step meets every count -> (n_ch, the curve, list of (limit, bucket, step, phases, the model's solve))"""
    c, n_ch = tb.material(kind, source, n_cf), tb.CH_OF[n_cf]
    one = tb.evaluator(kind, c)
    ev = pn.per_hop(one, n_ch)
    out = []
    for i, (limit, b) in enumerate(tb.grid_of(one, n_cf, n_ch)):
        step, phases = STEPS[i % 3], PHASES[i % 4]
        out.append((limit, b, step, phases, pn.solve(ev, n_ch, n_cf // n_ch, limit, b, T_LO, T_HI, step, phases)))
    return n_ch, c, out


@pytest.mark.parametrize("n_cf", sorted(tb.CH_OF))
@pytest.mark.parametrize("source", ["synthetic", "planted"])
@pytest.mark.parametrize("kind", KINDS)
def test_solves_equal_the_model(A, kind, source, n_cf):
    n_ch, c, cases = solve_cases(kind, source, n_cf)
    enc = tb.encoder(A)
    dev = tb.on_device(enc, kind, c)
    seen = {"met": 0, "pinned": 0, "two_levels": 0, "open": 0, "combos": set()}
    for limit, b, step, phases, ref in cases:
        same_solve(kind, gpu_solve(enc, kind, dev, n_ch, limit, b, step, phases), ref, (limit, b, step, phases))
        seen["met"] += ref["met"]
        seen["pinned"] += max(ref["phase_of"], default=-1) >= 0
        seen["two_levels"] += max(ref["phase_of"], default=-1) >= 1
        seen["open"] += ref["open"]
        seen["combos"].add((step, phases))
    print(f"{kind} {source} {n_cf}: { {k: v for k, v in seen.items() if k != 'combos'} }")
    assert len(seen["combos"]) == len(STEPS) * len(PHASES) or len(cases) < 16
    if n_cf >= 255:
        # both answers, hops pinned, on more than one level, and phases that ran out
        assert 0 < seen["met"] < 16 and seen["pinned"] > 0
    # another range, one target wide and off zero
    limit, b = cases[-2][:2]
    one = tb.evaluator(kind, c)
    for lo_db, hi_db in ((-2, 5.5), (0.078125, 0.078125)):
        ref = pn.solve(pn.per_hop(one, n_ch), n_ch, n_cf // n_ch, limit, b, int(lo_db * 64), int(hi_db * 64), 16, 8)
        same_solve(kind, gpu_solve(enc, kind, dev, n_ch, limit, b, 16, 8, lo_db, hi_db), ref, (lo_db, hi_db))


def loud_runs(kind, n_cf, n_ch):
    """synthetic material with three loud stretches of hops in a quiet stream -- the curve's noise-to-mask entries
    lowered by 16 dB everywhere else, by 4 and 8 dB in the second and third stretch, so that a frame there takes fewer
    bytes at every target -- a limit half way between the smallest and the largest body and a buffer half way from the
    peak at the highest target to the one at the whole stream's: the stretches bind one after the other, the rest never"""
    c = dict(sm.synthetic(kind, n_cf, 7))
    key = "nmr" if kind == "band" else "worst"
    shift = np.full(n_cf // n_ch, 16.0)
    for (a, e), db in (((100, 130), 0.0), ((400, 420), 4.0), ((700, 790), 8.0)):
        shift[a:e] = db
    c[key] = c[key] - np.repeat(shift, n_ch).reshape((-1,) + (1,) * (c[key].ndim - 1))
    one = tb.evaluator(kind, c)
    small, big = one(T_HI)[0], one(T_LO)[0]
    limit = (small + big) // 2
    drain = 5 * (limit << Q) // (4 * (n_cf // n_ch))         # above the mean hop: the quiet stream never fills the buffer
    hop_hi, peak_hi = tb.hop_peaks(one, n_ch, drain, T_HI)
    whole = kb.solve(one, n_ch, limit, (drain, 1 << 40, 0), T_LO, T_HI)
    peak_at = -(-whole["bucket"]["peak_q16"] >> Q)
    return c, one, limit, (drain, peak_hi + (peak_at - peak_hi) // 2, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_reductions(A, kind):
    n_cf, n_ch = 2050, 2
    c, one, limit, b = loud_runs(kind, n_cf, n_ch)
    enc = tb.encoder(A)
    dev = tb.on_device(enc, kind, c)
    small = one(T_HI)[0]
    # max_phases = 1: every shared output is the buffered solve's of the same handle, array for array
    for lim, bucket in ((limit, b), (small - 1, b), (10 ** 12, b), (limit, (b[0], 0, 0))):
        sol = gpu_solve(enc, kind, dev, n_ch, lim, bucket, 64, 1)
        buffered = tb.gpu_solve(enc, kind, dev, n_ch, lim, bucket)
        assert set(buffered) | {"target_t", "phase_of", "phases", "open"} == set(sol)
        for k, v in buffered.items():
            assert np.array_equal(sol[k].cpu().numpy(), v.cpu().numpy()) if hasattr(v, "cpu") else sol[k] == v, (lim, k)
        assert sol["phases"] == int(sol["met"]) and (sol["target_t"] == int(sol["target_nmr_db"] * 64)).all()
    sol = gpu_solve(enc, kind, dev, n_ch, limit, b, 64, 1)
    assert sol["met"] and sol["open"] and (sol["phase_of"] == 0).any() and (sol["phase_of"] == -1).any()
    # a buffer nothing reaches: every array and the result are the plain solve's, one bisection, no hop pinned
    for lim in (limit, small - 1, small, 10 ** 12):
        sol = gpu_solve(enc, kind, dev, n_ch, lim, (b[0], 1 << 40, 0), 64, 8)
        plain = enc.band_solve(dev, lim) if kind == "band" else enc.rate_solve(dev, None, lim)
        for k, v in plain.items():
            assert np.array_equal(sol[k].cpu().numpy(), v.cpu().numpy()) if hasattr(v, "cpu") else sol[k] == v, (lim, k)
        assert sol["phases"] == int(sol["met"]) and not sol["open"] and (sol["phase_of"] == -1).all()
        assert (sol["target_t"] == int(sol["target_nmr_db"] * 64)).all()
    # with phases to spare: the model's solve; more than one level pinned, hops left free below the one target, the
    # bytes the one target leaves unspent are spent, and the buffer holds
    ref = pn.solve(pn.per_hop(one, n_ch), n_ch, n_cf // n_ch, limit, b, T_LO, T_HI, 64, 8)
    sol = gpu_solve(enc, kind, dev, n_ch, limit, b, 64, 8)
    same_solve(kind, sol, ref, "phases to spare")
    buffered = tb.gpu_solve(enc, kind, dev, n_ch, limit, b)
    print(f"{kind}: one target {buffered['target_nmr_db']:g} dB with {buffered['total_bytes']} of {limit} bytes; pinned: "
          f"levels {[v / 64 for v in ref['levels']]} dB, {int((sol['phase_of'] >= 0).sum())} of {n_cf // n_ch} hops "
          f"pinned, {sol['total_bytes']} bytes, open {sol['open']}")
    assert sol["met"] and max(ref["phase_of"]) >= 1 and -1 in ref["phase_of"]
    assert sol["target_nmr_db"] < buffered["target_nmr_db"] == max(ref["target_t"]) / 64
    assert buffered["total_bytes"] < sol["total_bytes"] <= limit and sol["bucket"]["peak_q16"] <= b[1] << Q


@pytest.mark.parametrize("kind", KINDS)
def test_solves_queued_without_a_wait(A, kind):
    """a pinned solve, a buffered one and a pinned one with other parameters, queued on one handle and one stream through
    the C entry points and read back only after the third: they share the handle's workspace table"""
    import torch
    n_cf, n_ch = 2050, 2
    c, one, limit, b = loud_runs(kind, n_cf, n_ch)
    enc = tb.encoder(A)
    dev = tb.on_device(enc, kind, c)
    jobs = [(limit, b, 64, 8), (limit, b, None, None), (1 << 62, (b[0], b[1] * 2, 100 << Q), 1, 2)]
    gpu_solve(enc, kind, dev, n_ch, limit, b, 64, 1)                  # the handle's state is allocated: no wait below
    ptr = A.engine._ptr
    arrays = [ptr(dev[k]) for k in (("nmr", "cap", "cap_alloc") if kind == "band" else ("worst", "bits", "steps"))]
    head = [] if kind == "band" else [int(dev["row"]), int(dev["sub_stride"])]
    width = enc.band_stride if kind == "band" else 8
    queued = []
    for lim, bucket, step, phases in jobs:
        out = [torch.full((n_cf, width), -1, dtype=torch.int32, device=enc.device),
               torch.full((n_cf,), -1, dtype=torch.int32, device=enc.device),
               torch.full((n_cf,), 255, dtype=torch.uint8, device=enc.device),
               torch.full((6, 4), -1, dtype=torch.int32, device=enc.device),
               torch.full((2, n_cf // n_ch + 8), -1, dtype=torch.int32, device=enc.device)]
        if step is None:
            rc = getattr(enc.lib, f"pacx_{kind}_solve_bucket")(
                enc.h, n_cf, n_ch, *head, *arrays, lim, ctypes.byref(A._lib.PacxBucket(*bucket)), -30.0, 30.0,
                *(ptr(t) for t in out[:3]), ptr(out[3]), ptr(out[3][1:]), enc._stream())
        else:
            rc = getattr(enc.lib, f"pacx_{kind}_solve_bucket_pinned")(
                enc.h, n_cf, n_ch, *head, *arrays, lim, ctypes.byref(A._lib.PacxBucket(*bucket)), -30.0, 30.0, step,
                phases, *(ptr(t) for t in out[:3]), ptr(out[4][0]), ptr(out[4][1]), ptr(out[3]), ptr(out[3][1:]),
                ptr(out[3][4:]), enc._stream())
        assert rc == 0, enc.lib.pacx_last_error(enc.h)
        queued.append(out)
    torch.cuda.synchronize()
    ev, answers = pn.per_hop(one, n_ch), []
    for (lim, bucket, step, phases), out in zip(jobs, queued):
        ref = kb.solve(one, n_ch, lim, bucket, T_LO, T_HI) if step is None else \
            pn.solve(ev, n_ch, n_cf // n_ch, lim, bucket, T_LO, T_HI, step, phases)
        res = out[3].cpu().numpy()
        assert (int(res[0, 0]), int(res[0, 1]), int(res[:1, 2:].copy().view(np.int64)[0, 0])) == \
            (ref["t"], ref["met"], ref["total"]), (lim, bucket)
        words = res[1:4].reshape(-1).view(np.int64)
        assert dict(zip(kb.FIELDS, words.tolist())) == {k: ref["bucket"][k] for k in kb.FIELDS} and words[5] == -1
        per_hop = out[4].cpu().numpy()
        if step is None:
            assert (res[4:] == -1).all() and (per_hop == -1).all()
        else:
            assert res[4].tolist() == [ref["phases"], ref["open"], -1, -1] and (res[5] == -1).all()
            assert per_hop[0, :-8].tolist() == ref["target_t"] and per_hop[1, :-8].tolist() == ref["phase_of"]
            assert (per_hop[:, -8:] == -1).all()                               # nothing behind the outputs
        for t, want in zip(out, (ref["per_cf"], ref["n_bytes"], ref["capped"])):
            assert np.array_equal(t.cpu().numpy().astype(np.asarray(want).dtype), want), (lim, bucket)
        answers.append((ref["t"], ref["total"]))
    assert len(set(answers)) == 3                           # three answers of their own


def test_solve_arguments(A):
    import torch
    enc, E = tb.encoder(A), A._lib.E_ARG
    ptr = A.engine._ptr
    n_cf = 6
    band = tb.on_device(enc, "band", sm.synthetic("band", n_cf, 3))
    rate = tb.on_device(enc, "rate", sm.synthetic("rate", n_cf, 3))
    alloc = torch.zeros((n_cf, enc.band_stride), dtype=torch.int32, device=enc.device)
    budget = torch.zeros((n_cf, 8), dtype=torch.int32, device=enc.device)
    nby = torch.zeros((n_cf,), dtype=torch.int32, device=enc.device)
    cpd = torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device)
    hops = torch.zeros((2, n_cf), dtype=torch.int32, device=enc.device)
    res = torch.zeros((6, 4), dtype=torch.int32, device=enc.device)
    good = (100 << Q, 5000, 0)
    base = dict(n=n_cf, n_ch=2, limit=10 ** 6, b=good, lo=-30.0, hi=30.0, step=64, phases=8, target=hops[0],
                phase_of=hops[1], result=res, bres=res[1:], pres=res[4:], h=enc, row=None)

    def band_call(**kw):
        a = dict(base, **kw)
        return a["h"].lib.pacx_band_solve_bucket_pinned(
            a["h"].h, a["n"], a["n_ch"], ptr(band["nmr"]), ptr(band["cap"]), ptr(band["cap_alloc"]), a["limit"],
            None if a["b"] is None else ctypes.byref(A._lib.PacxBucket(*a["b"])), a["lo"], a["hi"], a["step"],
            a["phases"], ptr(alloc), ptr(nby), ptr(cpd), ptr(a["target"]), ptr(a["phase_of"]), ptr(a["result"]),
            ptr(a["bres"]), ptr(a["pres"]), None)

    def rate_call(**kw):
        a = dict(base, **kw)
        return a["h"].lib.pacx_rate_solve_bucket_pinned(
            a["h"].h, a["n"], a["n_ch"], int(rate["row"]) if a["row"] is None else a["row"], int(rate["sub_stride"]),
            ptr(rate["worst"]), ptr(rate["bits"]), ptr(rate["steps"]), a["limit"],
            None if a["b"] is None else ctypes.byref(A._lib.PacxBucket(*a["b"])), a["lo"], a["hi"], a["step"],
            a["phases"], ptr(budget), ptr(nby), ptr(cpd), ptr(a["target"]), ptr(a["phase_of"]), ptr(a["result"]),
            ptr(a["bres"]), ptr(a["pres"]), None)

    for call in (band_call, rate_call):
        assert call() == 0
        for step in (0, -1, -(1 << 31)):
            assert call(step=step) == E and b"pin_step_t" in enc.lib.pacx_last_error(enc.h), step
        for phases in (0, -1, 17, 1 << 30):
            assert call(phases=phases) == E and b"max_phases" in enc.lib.pacx_last_error(enc.h), phases
        assert call(step=1, phases=1) == 0 and call(step=(1 << 31) - 1, phases=16) == 0
        for n_ch in (0, -1, 4, 5):
            assert call(n_ch=n_ch) == E and b"multiple" in enc.lib.pacx_last_error(enc.h), n_ch
        assert call(n_ch=1) == 0 and call(n_ch=3) == 0 and call(n_ch=6) == 0
        assert call(n=-2) == E
        assert call(limit=-1) == E and b"negative" in enc.lib.pacx_last_error(enc.h)
        assert call(b=None) == E and b"null pointer" in enc.lib.pacx_last_error(enc.h)
        for missing in ("result", "bres", "pres", "target", "phase_of"):
            assert call(**{missing: None}) == E and b"null pointer" in enc.lib.pacx_last_error(enc.h), missing
        assert call(n=0, target=None, phase_of=None) == 0                    # no hops: nothing to write per hop
        for bad in ((-1, 100, 7), (5, -1, 0), (5, (1 << 40) + 1, 7), (5, 100, -1), (5, 100, (100 << Q) + 1)):
            assert call(b=bad) == E and b"bucket" in enc.lib.pacx_last_error(enc.h), bad
        for lo, hi in ((float("nan"), 3.0), (3.0, -3.0), (-30.01, 30.0), (-2e6, 0.0)):
            assert call(lo=lo, hi=hi) == E
    assert rate_call(row=7 * int(rate["sub_stride"])) == E
    torch.cuda.synchronize()
    # no frames: t_lo, met, one bisection, the scan of no hop
    assert band_call(n=0) == 0
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert r[0].tolist() == [T_LO, 1, 0, 0] and r[4, :2].tolist() == [1, 0]
    vq = A.engine.Encoder(44100, 128 / 44.1, use_vq=True)
    assert band_call(h=vq) == A._lib.E_UNSUPPORTED and rate_call(h=vq) == A._lib.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        vq.band_solve_bucket_pinned(band, 2, 10 ** 6, good)
    vq.close()
    # the Python layer: the step, the phases, the channels and the triple before the call
    for step in (0, 0.01, -1, None):
        with pytest.raises(ValueError, match="pin_step_db"):
            enc.band_solve_bucket_pinned(band, 2, 10 ** 6, good, pin_step_db=step)
    for phases in (0, 17, 2.5):
        with pytest.raises(ValueError, match="max_phases"):
            enc.rate_solve_bucket_pinned(rate, None, 2, 10 ** 6, good, max_phases=phases)
    for n_ch in (0, 4, 1.5):
        with pytest.raises(ValueError, match="n_channels"):
            enc.band_solve_bucket_pinned(band, n_ch, 10 ** 6, good)
    with pytest.raises(ValueError, match="three integers"):
        enc.rate_solve_bucket_pinned(rate, None, 2, 10 ** 6, (1, 2))
    for limit in (-1, 2.5):
        with pytest.raises(ValueError, match="limit_bytes"):
            enc.band_solve_bucket_pinned(band, 2, limit, good)
    with pytest.raises(A._lib.PacxError, match="bucket"):
        enc.band_solve_bucket_pinned(band, 2, 10 ** 6, (5, 100, (100 << Q) + 1))
    sol = enc.band_solve_bucket_pinned(band, 2, 10 ** 6, A.pacfile.bucket(96, 2, 44100, 5000))
    assert sol["met"] and sol["phases"] >= 1 and tuple(sol["target_t"].shape) == (3,)


# ------------------------------------------------------------------------------------------------ 3. the GPU's own curves
@pytest.mark.parametrize("curve", ["band", "rate", "gain-shape"])
def test_own_curves_of_the_castanet_stream(A, curve):
    """the six-hop block-switched castanet stream: the curve is the GPU's, the solve runs where the stream's would (for
    the gain-shape curve on the scalar sibling), the model works on the arrays read back"""
    from audio_codec_amd import context
    pcm, sr = tb.STREAMS["castanet6"]()
    # the handle is asked for here: one kept from an earlier module may have been closed since
    cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None, curve == "gain-shape")
    if curve == "rate":
        dev, solver, kind = enc.rate_curve(view, flags, cp.targetBitsPerSample), enc, "rate"
        one = tb.evaluator("rate", dict({k: dev[k].cpu().numpy() for k in ("worst", "bits", "steps")}, row=dev["row"],
                                        sub_stride=dev["sub_stride"]))
    else:
        dev = (enc.vq_band_curve if curve == "gain-shape" else enc.band_curve)(view, flags, cp.targetBitsPerSample)
        tables = bm.tables(po.make_params(sr, pcm.shape[1], 320))
        one = tb.evaluator("band", bm.with_arrays(tables, *(dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc"))))
        solver, kind = context.scalar_sibling(enc) if curve == "gain-shape" else enc, "band"
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    ev = pn.per_hop(one, n_ch)
    drain = kb.drain_q16(tb.KBPS, n_ch, 44100)
    limit = (one(T_HI)[0] + one(0)[0]) // 2
    whole = kb.solve(one, n_ch, limit, (drain, 1 << 40, 0), T_LO, T_HI)
    hop_hi = max(kb.hop_bytes(one(T_HI)[2], n_ch))
    pinned = 0
    for share in (2.0, 0.8, 0.6, 0.4):
        size = max(int(share * (whole["bucket"]["peak_q16"] >> Q)), hop_hi)
        for step, phases in ((1, 16), (16, 8), (64, 2)):
            ref = pn.solve(ev, n_ch, blocks, limit, (drain, size, 0), T_LO, T_HI, step, phases)
            same_solve(kind, gpu_solve(solver, kind, dev, n_ch, limit, (drain, size, 0), step, phases), ref,
                       (curve, share, step, phases))
            pinned += max(ref["phase_of"]) >= 0
    print(f"{curve}: whole stream {whole['t'] / 64:g} dB, hops pinned in {pinned} of 12 solves")
    assert pinned > 0


# ------------------------------------------------------------------------------------------------ 4. streams
# Chosen on the CPU with band_model on the golden excerpt (rate_model.analysis, band_model.curve, pin_model.solve): the
# castanet hops 24 ... 47 hold the excerpt's first five strokes.  At 96 kb/s the whole-stream solve gives 2.17 dB with
# a peak of 2022 bytes.  Under a buffer of 1200 bytes the one-target solve gives 4.22 dB and leaves 1782 of 14489
# bytes unspent; with a step of 0.25 dB the pinned solve finds the levels 4.22, 0.77 and -0.125 dB: 13 blocks pinned at
# the first, 2 at the second, 11 free at the third, 9 bytes unspent.
PIN_HOPS, PIN_BUFFER, PIN_STEP_DB = (24, 48), 1200, 0.25
_STREAM = {}


def pin_stream(A, allocation, use_vq=False):
    key = allocation, use_vq
    if key not in _STREAM:
        ex = load_excerpt("castanet")
        pcm, sr = np.ascontiguousarray(ex["pcm"][PIN_HOPS[0] * 1024:PIN_HOPS[1] * 1024]), int(ex["sr"])
        cp, enc, view, flags = A.pacfile._rate_stream_setup(pcm, sr, 320, True, None, use_vq)
        tables = bm.tables(po.make_params(sr, pcm.shape[1], 320))
        if allocation == "band":
            dev = (enc.vq_band_curve if use_vq else enc.band_curve)(view, flags, cp.targetBitsPerSample)
            host = bm.with_arrays(tables, *(dev[k].cpu().numpy() for k in ("nmr", "cap", "cap_alloc")))
        else:
            dev = enc.rate_curve(view, flags, cp.targetBitsPerSample)
            host = dict({k: dev[k].cpu().numpy() for k in ("worst", "bits", "steps")}, row=dev["row"],
                        sub_stride=dev["sub_stride"])
        _STREAM[key] = {"pcm": pcm, "sr": sr, "one": tb.evaluator("band" if allocation == "band" else "rate", host),
                        "head": A.pacfile.header_bytes(cp)}
    return _STREAM[key]


def block_records(A, data, n_ch):
    """the records of a .pac stream block by block, found on the device (Encoder.index_body) -> list of bytes"""
    import torch
    from audio_codec_amd import context
    cp, pos = A.pacfile.parse_header(data)
    enc = context.encoder_for_params(cp)
    raw = np.frombuffer(data, np.uint8)[pos:].copy()
    offsets, sizes, result = enc.index_body(torch.as_tensor(raw, device=enc.device), n_ch)
    records, used, broke = (int(v) for v in result.cpu().numpy())
    assert broke == -1 and used == len(raw) and records % n_ch == 0
    offsets, sizes = offsets[:records].cpu().numpy(), sizes[:records].cpu().numpy()
    return [b"".join(raw[offsets[r] - 4:offsets[r] + sizes[r]].tobytes() for r in range(h * n_ch, (h + 1) * n_ch))
            for h in range(records // n_ch)]


CASES = [("band", False), ("budget", False), ("band", True)]


@pytest.mark.parametrize("allocation,use_vq", CASES)
def test_streams(A, allocation, use_vq):
    g = pin_stream(A, allocation, use_vq)
    pcm, sr, one = g["pcm"], g["sr"], g["one"]
    n_ch, blocks = pcm.shape[1], len(pcm) // 1024 + 2
    limit = int(np.floor(tb.KBPS * 1000.0 * n_ch * blocks * 1024 / sr / 8.0))
    kw = dict(block_switching=True, allocation=allocation, use_vq=use_vq)
    pinned, to_buffer = A.pacfile.encode_stream_abr_pinned, A.quality.encode_stream_to_buffer_pinned
    at_target = A.pacfile.encode_stream_vq_nmr if use_vq else \
        functools.partial(A.pacfile.encode_stream_nmr, allocation=allocation)
    drain = kb.drain_q16(tb.KBPS, n_ch, sr)
    # a buffer nothing reaches: the average-rate stream, byte for byte
    plain = A.pacfile.encode_stream_vq_abr(pcm, sr, tb.KBPS, block_switching=True) if use_vq else \
        A.pacfile.encode_stream_abr(pcm, sr, tb.KBPS, block_switching=True, allocation=allocation)
    assert pinned(pcm, sr, tb.KBPS, 1 << 40, **kw) == plain
    # one phase: the buffered stream
    assert pinned(pcm, sr, tb.KBPS, PIN_BUFFER, max_phases=1, **kw) == \
        A.pacfile.encode_stream_abr_buffered(pcm, sr, tb.KBPS, PIN_BUFFER, **kw)
    # the buffer that binds
    b = (drain, PIN_BUFFER, 0)
    ref = pn.solve(pn.per_hop(one, n_ch), n_ch, blocks, limit, b, T_LO, T_HI, int(PIN_STEP_DB * 64), 8)
    uniform = kb.solve(one, n_ch, limit, b, T_LO, T_HI)
    data, info = to_buffer(pcm, sr, tb.KBPS, PIN_BUFFER, pin_step_db=PIN_STEP_DB, **kw)
    frozen = sorted({int(k) for k in ref["phase_of"] if k >= 0})
    print(f"{allocation}{' gain-shape' if use_vq else ''}: one target {uniform['t'] / 64:g} dB with {uniform['total']} of "
          f"{limit} bytes; pinned: levels {[v / 64 for v in ref['levels']]} dB, blocks per phase "
          f"{[ref['phase_of'].count(k) for k in frozen]}, {ref['phase_of'].count(-1)} free, {ref['total']} bytes, "
          f"peak {info['peak_bytes']:.1f} of {PIN_BUFFER}")
    if (allocation, use_vq) == ("band", False):
        # the premise, as chosen on the CPU: two phases pinned blocks and blocks stayed free, well below the one target
        assert len(frozen) >= 2 and ref["phase_of"].count(-1) >= 1 and not ref["open"]
        assert ref["t"] <= uniform["t"] - 64 and ref["total"] > uniform["total"]
    assert ref["met"] and uniform["met"] and max(ref["phase_of"]) >= 0
    assert data == pinned(pcm, sr, tb.KBPS, PIN_BUFFER, pin_step_db=PIN_STEP_DB, **kw)
    assert (info["target_nmr_db"] * 64, info["phases"], info["open"]) == (ref["t"], ref["phases"], bool(ref["open"]))
    assert (info["block_target_nmr_db"] * 64).tolist() == ref["target_t"] and info["phase_of"].tolist() == ref["phase_of"]
    assert info["limit_bytes"] == limit and info["bucket"] == b
    predicted = info["n_bytes"].reshape(-1)
    assert np.array_equal(predicted, ref["n_bytes"]) and (predicted > 0).all()          # no hop dropped
    assert tb.record_sizes(A, data) == predicted.tolist()                                # the second pass wrote it
    thr, s = pn.through(predicted, n_ch, b)
    assert info["total_bytes"] == s["total"] == ref["total"] <= limit
    assert (info["level_bytes"] * 65536).astype(np.int64).tolist() == s["level"] and len(s["level"]) == blocks
    assert (info["through_bytes"] * 65536).astype(np.int64).tolist() == thr and max(thr) <= PIN_BUFFER << Q
    assert info["peak_bytes"] * 65536 == s["peak_q16"] <= PIN_BUFFER << Q and info["peak_block"] == s["peak_hop"]
    # no block above the one target; every block holds the records of encode_stream_nmr at its own target
    assert max(ref["target_t"]) <= uniform["t"]
    mine = block_records(A, data, n_ch)
    assert len(mine) == blocks
    for t in sorted(set(ref["target_t"])):
        theirs = block_records(A, at_target(pcm, sr, t / 64, block_switching=True), n_ch)
        assert len(theirs) == blocks
        for h in range(blocks):
            if ref["target_t"][h] == t:
                assert mine[h] == theirs[h], (t, h)
    # the finished bytes play through the buffer; the average-rate stream does not
    rep = A.quality.buffer_report(data, tb.KBPS, PIN_BUFFER)
    assert rep["fits"] and rep["first_over"] == -1 and rep["blocks"] == blocks and rep["total_bytes"] == info["total_bytes"]
    assert np.array_equal(rep["level_bytes"], info["level_bytes"]) and rep["peak_bytes"] <= PIN_BUFFER
    assert not A.quality.buffer_report(plain, tb.KBPS, PIN_BUFFER)["fits"]
    # the two messages are the buffered call's, character for character
    hop_hi = max(kb.hop_bytes(one(T_HI)[2], n_ch))
    for args, bucket, lim in (((tb.KBPS, hop_hi - 1), (drain, hop_hi - 1, 0), limit),
                              ((4.0, 1 << 40), (kb.drain_q16(4.0, n_ch, sr), 1 << 40, 0),
                               int(np.floor(4.0 * 1000.0 * n_ch * blocks * 1024 / sr / 8.0)))):
        unmet = kb.solve(one, n_ch, lim, bucket, T_LO, T_HI)
        assert not unmet["met"]
        with pytest.raises(ValueError) as err:
            pinned(pcm, sr, *args, **kw)
        with pytest.raises(ValueError) as theirs:
            A.pacfile.encode_stream_abr_buffered(pcm, sr, *args, **kw)
        assert str(err.value) == str(theirs.value) == kb.refusal(unmet, lim, bucket, len(g["head"]), 30.0)
