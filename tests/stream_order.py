"""The stream contract of include/pacx.h under a schedule that can see it fail (test infrastructure).

Nearly every GPU test calls an entry point on the default stream with finished inputs and reads the outputs through
.cpu(), which waits for the whole device: a kernel on the wrong stream, an internal stream that does not wait for its
fork event, a chain that does not join back before the call returns -- none of them shows.  run_delayed() is the
schedule that shows them.  Every case has a REAL input set and a DECOY of the same shapes and types, both valid
material for the entry point, so that a kernel which reads the wrong one reads valid memory and gives a wrong answer,
nothing worse.  On the caller's stream, with no host wait anywhere:

    producer (holds the stream) | real inputs over the decoy | the call(s) | outputs to keep-buffers |
    decoy over the inputs again, poison over the outputs

and then, on the host, the producer must still be running (`released.query()` is False): the whole sequence was
queued while its stream was held, which is also what "asynchronous" means.  A kernel that did not wait for the
caller's stream read the decoy; one that is not joined back ran after the keep-copy (stale outputs) or after the
overwrite (decoy inputs).  Truth is the same call made synchronously on the default stream, and the reference's own
bytes and PCM from tests/golden wherever a fixture exists; both comparisons are plain equality.

The decoy of an excerpt is the OTHER excerpt of tests/golden (castanet <-> harpsichord: same length, channels and
sample rate), so both sides have the reference's bytes; for curves it is the synthetic curve of another seed, for a
limit one from the other end of the range.  tests/test_stream_order.py checks on the CPU that every pair differs in
every output row.

The material functions are NumPy only; everything that touches torch imports it inside the function.
"""
import functools
import os
import struct
import time

import numpy as np

import mixed_batches as mb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HOP = 1024
SR = 44100                                # both excerpts
N_CALLER_STREAMS = 4
# The delay is DELAY_MULTIPLE times the host time of a timed dry pass of the very sequence (inputs, calls, keep-copies,
# overwrites) made right before, and DELAY_MIN_MS at least.  Measured on an MI355X ("stream
# contract"): dry passes of 0.06 to 0.82 ms, so the floor decides; the host needed 0.83 to 1.03 ms at most (2.87 ms
# once, on a first launch) to queue a sequence behind the producer -- 40 ms leaves a factor of 14 over the worst seen.
DELAY_MULTIPLE = 8
DELAY_MIN_MS = 40.0
DELAY_MAX_MS = 400.0
POISON = 0xA5

# Calls that may wait for the host, each with the sentence of include/pacx.h it rests on.  run_delayed() checks validity
# BEFORE such a call (job.checkpoint(name)) and not after it.  A row needs header text.
MAY_BLOCK = (
    ("the second of two segmented or peak solves queued back to back on one handle",
     ("pacx_rate_solve_segments", "pacx_band_solve_segments", "pacx_rate_solve_peak", "pacx_band_solve_peak"),
     "a call waits for the upload of the segmented solve before it on the same handle, and for nothing else"),
    ("any call that has to grow a workspace of the handle",
     ("*",),
     "a call that has to grow a workspace waits for the whole device first, then frees and allocates"),
)
BLOCKING_CALLS = frozenset(n for _, names, _ in MAY_BLOCK for n in names if n != "*")

PAIRS = {"long": ("harpsichord", "castanet"), "bs": ("castanet", "harpsichord")}        # variant -> (real, decoy)

LOG = []                                  # one dict per delayed run: what the summary test reports


# ------------------------------------------------------------------------------------------------- material (NumPy)
@functools.lru_cache(maxsize=None)
def excerpt(name):
    return dict(np.load(os.path.join(GOLDEN, f"excerpt_{name}.npz")))


def planar_stream(pcm):
    """pacfile.device_stream's layout on the host: int16 [nCh, (n_hops + 3) * 1024] -- zeros, the hops, the last hop
    again, zeros"""
    n, n_ch = pcm.shape
    buf = np.zeros((n_ch, n + 3 * HOP), np.int16)
    buf[:, HOP:HOP + n] = pcm.T
    buf[:, HOP + n:2 * HOP + n] = pcm[n - HOP:].T
    return buf


def packed_flags(rows, n_frames):
    """(last, cur, next) rows of the reference's driver -> the flag bytes of the n_frames written blocks (Close: 0)"""
    rows = np.asarray(rows)
    out = np.zeros(n_frames, np.uint8)
    out[:len(rows)] = (rows[:, 0] != 0) * 1 + (rows[:, 1] != 0) * 2 + (rows[:, 2] != 0) * 4
    return out


def header_len(pac):
    n_bands = struct.unpack("<L", pac[26:30])[0]                      # coder/pacfile.py:136-151
    return 30 + 2 * n_bands


def split_records(pac):
    """-> (the body: everything behind the header, the payload of every record)"""
    pos = header_len(pac)
    body, out = pac[pos:], []
    while pos < len(pac):
        n = int.from_bytes(pac[pos:pos + 4], "little")
        out.append(pac[pos + 4:pos + 4 + n])
        pos += 4 + n
    assert pos == len(pac)
    return body, out


@functools.lru_cache(maxsize=None)
def scalar_material(name, variant):
    """the 64-hop stereo excerpt as the scalar coder at 128 kb/s takes it, with the reference's .pac of it:
    variant "long" (no flags) or "bs" (the reference driver's flags)"""
    ex = excerpt(name)
    pcm = ex["pcm"]
    n_frames = len(pcm) // HOP + 2
    pac = bytes(ex[f"pac_{variant}"])
    body, records = split_records(pac)
    return {"pcm": pcm, "planar": planar_stream(pcm), "n_frames": n_frames, "n_ch": pcm.shape[1], "pac": pac,
            "flags": packed_flags(ex["flags_bs"], n_frames) if variant == "bs" else None, "body": body,
            "records": records}


@functools.lru_cache(maxsize=None)
def vq_material(name, kbps):
    """the first 24 hops through the gain-shape coder (128 kb/s; 96 kb/s with SBR), block-switched, with the
    reference's .pac"""
    gold = np.load(os.path.join(GOLDEN, f"excerpt_vq_{name}.npz"))
    hops = int(gold["hops"])
    pcm = excerpt(name)["pcm"][:hops * HOP]
    n_frames = hops + 2
    pac = bytes(gold[f"pac_vq{kbps}"])
    body, records = split_records(pac)
    return {"pcm": pcm, "planar": planar_stream(pcm), "n_frames": n_frames, "n_ch": pcm.shape[1], "pac": pac,
            "flags": packed_flags(gold[f"flags_vq{kbps}"], n_frames), "body": body, "records": records}


def decoded(name, tag):
    """the reference decoder's int16 PCM of the .pac above: tag long, bs, vq128, vq96"""
    vq = tag.startswith("vq")
    return np.load(os.path.join(GOLDEN, f"decoded_vq_{name}.npz" if vq else f"decoded_{name}.npz"))[f"pcm_{tag}"]


def padded_bodies(a, b):
    """two bodies as uint8 arrays of one length: the longer one's plus the eight zero bytes the parsers may read"""
    n = max(len(a), len(b)) + 8
    out = []
    for body in (a, b):
        buf = np.zeros(n, np.uint8)
        buf[:len(body)] = np.frombuffer(body, np.uint8)
        out.append(buf)
    return out


# the flagged items of mixed_batches: 64 stereo frames of atoms that code something under every flag byte, the real
# and the decoy batch of one name never the same atom in a frame
FLAGGED_FRAMES = 64
_ALIVE = [k for k in range(mb.N_ATOMS) if k not in (mb.DROP, mb.ZEROS)]
FLAGGED = {"no_short": mb.LONG_FLAGS, "no_long": mb.SHORT_FLAGS}


@functools.lru_cache(maxsize=None)
def flagged_material(name, decoy):
    """a flagged batch without one short-coded frame (no_short) or without one long-coded frame (no_long): under the
    split one of the two frame lists is empty.  -> blocks int16 [64, 2, 2048], flags uint8 [64], items"""
    f = np.arange(FLAGGED_FRAMES)
    atom = np.array(_ALIVE)[(f + (4 if decoy else 0)) % len(_ALIVE)]
    flags = np.array(FLAGGED[name])[(f // (3 if decoy else 1) + (1 if decoy else 0)) % 4].astype(np.uint8)
    blocks = np.ascontiguousarray(mb.atoms(2)[atom])
    return {"blocks": blocks, "flags": flags, "items": atom * 8 + flags, "n_frames": FLAGGED_FRAMES, "n_ch": 2}


def flagged_records(material):
    """the oracle's payload of every channel-frame of a flagged batch (mixed_batches.oracle_items)"""
    _, records = mb.oracle_items("scalar", 2)
    return [records[int(i)][ch] for i in material["items"] for ch in range(2)]


# ---- curves no encoder made (segment_model.synthetic, the band tables of 44100 Hz) and the solves queued on them
CURVE_CF, CURVE_CH = 130, 2
T_LO, T_HI = -30 * 64, 30 * 64
KINDS = ("band", "rate")


@functools.lru_cache(maxsize=None)
def curve_material(kind, decoy):
    import segment_model as sm
    return sm.synthetic(kind, CURVE_CF, 23 if decoy else 7)


def evaluate(kind, c, t):
    """(total, per_cf, n_bytes, capped) of the model at grid target t"""
    import abr_model as am
    import band_model as bm
    return (bm.evaluate if kind == "band" else am.evaluate)(c, t)[:4]


@functools.lru_cache(maxsize=None)
def solve_jobs(kind):
    """the limits, segments and buckets of every solve the GPU tests queue, fixed on the REAL curve: a limit half way
    between the smallest and the largest body of the stretch it governs, so that the answer lies inside the range and
    moves with the curve"""
    import bucket_model as kb
    import segment_model as sm
    c = curve_material(kind, False)

    def mid(a, b):
        part = sm.slice_curve(kind, c, a, b)
        return (sm.total(kind, part, T_HI) + sm.total(kind, part, T_LO)) // 2

    def mids(first):
        return np.array([mid(a, b) for a, b in zip(first, first[1:])], np.int64)
    first_a, first_b, first_c = (np.array(v, np.int64) for v in ([0, 1, 4, 67, 130], [0, 50, 130], [0, 30, 60, 130]))
    n_hops = CURVE_CF // CURVE_CH
    drain = (evaluate(kind, c, 0)[0] << kb.Q) // n_hops + 999

    def peak(t):
        return -(-kb.scan(evaluate(kind, c, t)[2], CURVE_CH, (drain, kb.SIZE_MAX, 0))["peak_q16"] >> kb.Q)
    return {"limit": int(mid(0, CURVE_CF)),
            "segments_a": (first_a, mids(first_a)), "segments_b": (first_b, mids(first_b) * 3 // 4),
            "peak": (first_c, mids(first_c) * 7 // 8, int(mid(0, CURVE_CF))),
            "bucket": (drain, peak(T_HI) + (peak(T_LO) - peak(T_HI)) // 4, 0), "bucket_limit": 1 << 62}


def model_answers(kind, c):
    """what the models give for solve_jobs(kind) on curve c: name -> dict of arrays"""
    import abr_model as am
    import band_model as bm
    import bucket_model as kb
    import peak_model as pk
    import segment_model as sm
    jobs = solve_jobs(kind)
    per = sm.PER_CF[kind][0]
    plain = (bm.solve if kind == "band" else am.solve)(c, jobs["limit"], T_LO, T_HI)
    out = {"plain": {"t": np.array([plain["t"]]), "met": np.array([plain["met"]]), "total": np.array([plain["total"]]),
                     "per_cf": plain[per], "n_bytes": plain["n_bytes"], "capped": plain["capped"]}}
    for name in ("segments_a", "segments_b"):
        r = sm.solve_segments(kind, c, *jobs[name], T_LO, T_HI)
        out[name] = {"t": r["t"], "met": r["met"], "total": r["total"], "per_cf": r[per], "n_bytes": r["n_bytes"],
                     "capped": r["capped"]}
    first, peaks, limit = jobs["peak"]
    r = pk.solve_peak(kind, c, first, peaks, limit, T_LO, T_HI)
    out["peak"] = {"t": r["t"], "met": r["met"], "total": r["total"], "floor": r["floor"],
                   "stream": np.array([r["t_stream"], r["met_stream"], r["total_stream"]], np.int64),
                   "per_cf": r[per], "n_bytes": r["n_bytes"], "capped": r["capped"]}
    ev = functools.lru_cache(maxsize=None)(lambda t: evaluate(kind, c, t))
    r = kb.solve(ev, CURVE_CH, jobs["bucket_limit"], jobs["bucket"], T_LO, T_HI)
    out["bucket"] = {"t": np.array([r["t"]]), "met": np.array([int(r["met"])]), "total": np.array([r["total"]]),
                     "per_cf": r["per_cf"], "n_bytes": r["n_bytes"], "capped": r["capped"],
                     "scan": np.array([r["bucket"][k] for k in kb.FIELDS], np.int64),
                     "level": np.array(kb.scan(r["n_bytes"], CURVE_CH, jobs["bucket"])["level"], np.int64).reshape(-1)}
    return out


# ------------------------------------------------------------------------------------------------- comparison
def valid_payload(n_bytes, payload):
    """the bytes a channel-frame's record holds: what lies behind n_bytes in a slot is not defined"""
    return [bytes(payload[i, :max(int(n_bytes[i]), 0)]) for i in range(len(n_bytes))]


def same_records(got, want):
    """two results of an encode (dicts of NumPy arrays with n_bytes, payload, status) -> the rows that differ"""
    bad = set(np.flatnonzero(got["n_bytes"] != want["n_bytes"]).tolist())
    if "status" in got:
        bad |= set(np.flatnonzero(got["status"] != want["status"]).tolist())
    a, b = valid_payload(got["n_bytes"], got["payload"]), valid_payload(want["n_bytes"], want["payload"])
    bad |= {i for i in range(len(a)) if a[i] != b[i]}
    return sorted(bad)


def same_arrays(got, want):
    """-> the names whose arrays differ, bit for bit (NaN equals NaN)"""
    bad = []
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------- the GPU side
class Job:
    """what prepare() returns: the buffers a call reads (they hold the DECOY), and whatever else call and collect share.
    add(real, decoy) -> the buffer."""

    def __init__(self, device):
        self.device = device
        self.inputs = []                  # (buffer, real, decoy): device tensors of one shape and type
        self.checkpoint = lambda name: None

    def add(self, real, decoy):
        import torch
        real, decoy = np.ascontiguousarray(real), np.ascontiguousarray(decoy)
        assert real.shape == decoy.shape and real.dtype == decoy.dtype
        r, d = torch.as_tensor(real, device=self.device), torch.as_tensor(decoy, device=self.device)
        buf = d.clone()
        self.inputs.append((buf, r, d))
        return buf

    def load(self, which):
        """queue real (1) or decoy (2) over the buffers on the current stream"""
        for t in self.inputs:
            t[0].copy_(t[which], non_blocking=True)


class Clock:
    """the spin of torch.cuda._sleep in cycles per microsecond, by an event-timed calibration as EncoderPool.align
    makes it; without _sleep the producer is a loop of large device copies, calibrated the same way"""

    def __init__(self, device):
        import torch
        self.device = device
        self.spin = hasattr(torch.cuda, "_sleep")
        if not self.spin:
            self.a = torch.zeros((64 << 20,), dtype=torch.uint8, device=device)
            self.b = torch.zeros_like(self.a)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self._hold(100_000 if self.spin else 1)
        t0.record()
        self._hold(2_000_000 if self.spin else 8)
        t1.record()
        t1.synchronize()
        self.per_us = (2_000_000 if self.spin else 8) / max(t0.elapsed_time(t1) * 1e3, 1.0)

    def _hold(self, units):
        import torch
        if self.spin:
            torch.cuda._sleep(int(units))
        else:
            for _ in range(int(units)):
                self.b.copy_(self.a, non_blocking=True)

    def hold(self, ms):
        """queue a producer of about `ms` milliseconds on the current stream"""
        self._hold(max(int(ms * 1e3 * self.per_us), 1))


def _poison(tensors):
    import torch
    for t in tensors:
        t.view(-1).view(torch.uint8).fill_(POISON) if t.is_contiguous() else t.fill_(0)


def _to_host(kept):
    return {k: v.cpu().numpy() for k, v in kept.items()}


def run_direct(prepare, call, collect):
    """truth: the call made synchronously on the default stream with the real inputs -> dict of NumPy arrays"""
    import torch
    job = prepare()
    job.load(1)
    torch.cuda.synchronize()
    call(job)
    torch.cuda.synchronize()
    return _to_host(collect(job))


def _sequence(job, call, collect, call_stream=None):
    """steps 3 to 6 on the current stream -> the keep-buffers"""
    import torch
    job.load(1)
    if call_stream is None:
        call(job)
    else:
        with torch.cuda.stream(call_stream):       # the negative control: the call on a stream that waits for nothing
            call(job)
    outs = collect(job)
    kept = {k: torch.empty_like(v) for k, v in outs.items()}
    for k, v in outs.items():
        kept[k].copy_(v, non_blocking=True)
    job.load(2)
    _poison(outs.values())
    return kept


def run_delayed(enc, stream, prepare, call, collect, clock, call_stream=None, what=""):
    """The schedule of the module docstring on `stream` (a torch stream of the test's).  prepare() -> Job, call(job)
    queues the call or chain under test on the current stream, collect(job) -> dict of the output tensors.
    call_stream: make the call on that stream instead (test_the_method_bites).  -> dict of NumPy arrays, the
    keep-buffers.  Fails when the host was slower than the delay."""
    import torch
    job = prepare()
    with torch.cuda.stream(stream):
        # 1. warm-up on the decoy, twice: the first grows the workspaces and fills them with stale but valid lists and
        # lines, the second is the timed dry pass the delay is sized by
        _sequence(job, call, collect)
        torch.cuda.synchronize()
        job.load(2)
        torch.cuda.synchronize()
        t = time.perf_counter()
        kept = _sequence(job, call, collect)
        dry_ms = (time.perf_counter() - t) * 1e3
        torch.cuda.synchronize()
        del kept
        job.load(2)
        torch.cuda.synchronize()
        delay_ms = min(max(DELAY_MULTIPLE * dry_ms, DELAY_MIN_MS), DELAY_MAX_MS)
        begun, released = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        state = {"checked": False}

        def still_held(where):
            host_ms = (time.perf_counter() - t0) * 1e3
            assert not released.query(), \
                f"{what}: the host took {host_ms:.2f} ms to queue the sequence up to {where}, the producer held the " \
                f"stream for {delay_ms:.2f} ms ({DELAY_MULTIPLE} x the dry pass of {dry_ms:.3f} ms, at least " \
                f"{DELAY_MIN_MS} ms): the schedule proves nothing"
            return host_ms

        def checkpoint(name):
            assert name in BLOCKING_CALLS, f"{name} is not in stream_order.MAY_BLOCK"
            if not state["checked"]:
                state["host_ms"] = still_held("the call that may wait, " + name)
                state["checked"] = True
        job.checkpoint = checkpoint
        t0 = time.perf_counter()
        begun.record()
        clock.hold(delay_ms)                                               # 2. the producer
        released.record()
        kept = _sequence(job, call, collect, call_stream)                  # 3. - 6.
        if not state["checked"]:
            state["host_ms"] = still_held("its end")                       # 7. validity
        torch.cuda.synchronize()                                           # 8.
    LOG.append({"what": what, "dry_ms": dry_ms, "delay_ms": delay_ms, "host_ms": state["host_ms"],
                "held_ms": begun.elapsed_time(released), "control": call_stream is not None})
    return _to_host(kept)


def run_pool(pool, cases, what=""):
    """Two handles side by side: cases[k] = (prepare, call, collect) for slot k of an engine.EncoderPool.  The producer
    is the pool's own start gate (align): both slots' sequences are queued while it holds their streams, so both really
    start together.  -> the keep-buffers of every slot as NumPy arrays."""
    import torch
    jobs = [c[0]() for c in cases]
    for k, (_, call, collect) in enumerate(cases):
        with torch.cuda.stream(pool.streams[k]):
            _sequence(jobs[k], call, collect)                      # warm-up on the decoy
        torch.cuda.synchronize()
        jobs[k].load(2)
    pool.align()                                                   # the default gate: its calibration happens here, once
    torch.cuda.synchronize()
    delay_ms = DELAY_MIN_MS
    t0 = time.perf_counter()
    pool.align(delay_ms * 1e3)
    kept = []
    for k, (_, call, collect) in enumerate(cases):
        with pool.slot(k):
            kept.append(_sequence(jobs[k], call, collect))
    host_ms = (time.perf_counter() - t0) * 1e3
    assert not pool._gate.query(), \
        f"{what}: the host took {host_ms:.2f} ms to queue both slots, the gate held their streams for " \
        f"{delay_ms:.2f} ms: the schedule proves nothing"
    pool.synchronize()
    torch.cuda.synchronize()
    LOG.append({"what": what, "dry_ms": float("nan"), "delay_ms": delay_ms, "host_ms": host_ms, "held_ms": float("nan"),
                "control": False})
    return [_to_host(k) for k in kept]


def caller_streams(device, n=N_CALLER_STREAMS):
    import torch
    return [torch.cuda.Stream(device=device) for _ in range(n)]


# ---- rate control through the C entry points: the wrappers of engine.Encoder read the solves' results back
KEYS = {"band": ("nmr", "cap", "cap_alloc"), "rate": ("worst", "bits", "steps")}


def curve_args(enc, kind, dev):
    """(head, array pointers, width of the per-frame output) of a curve on the device"""
    from audio_codec_amd.engine import _ptr
    head = [] if kind == "band" else [int(dev["row"]), int(dev["sub_stride"])]
    return head, [_ptr(dev[k]) for k in KEYS[kind]], enc.band_stride if kind == "band" else 8


def solve_outputs(enc, kind, n_cf, n_result):
    """per_cf, n_bytes, capped, result rows: what a solve writes, prefilled"""
    import torch
    width = enc.band_stride if kind == "band" else 8
    return {"per_cf": torch.zeros((n_cf, width), dtype=torch.int32, device=enc.device),
            "n_bytes": torch.zeros((n_cf,), dtype=torch.int32, device=enc.device),
            "capped": torch.zeros((n_cf,), dtype=torch.uint8, device=enc.device),
            "result": torch.full((n_result, 4), -1, dtype=torch.int32, device=enc.device)}


def queue_solve(enc, kind, op, dev, n_cf, out, limit=None, seg_first=None, limits=None, bucket=None, n_ch=None,
                lo=-30.0, hi=30.0):
    """pacx_<kind>_<op> on the current stream, nothing read back.  op: solve (limit), solve_segments (seg_first,
    limits: host int64 arrays; result [n_seg]), solve_peak (seg_first, limits = the peaks, limit = the stream's;
    result [n_seg + 1 + ceil(n_seg / 4)]: segments, the stream, the floors), solve_bucket (limit, bucket, n_ch; result
    [4]: the result, then pacx_bucket_result)."""
    import ctypes
    from audio_codec_amd import _lib
    from audio_codec_amd.engine import _ptr
    head, arrays, _ = curve_args(enc, kind, dev)
    name = f"pacx_{kind}_{op}"
    per = [_ptr(out["per_cf"]), _ptr(out["n_bytes"]), _ptr(out["capped"])]
    res = out["result"]
    if op == "solve":
        args = [n_cf, *head, *arrays, int(limit), lo, hi, *per, _ptr(res)]
    elif op == "solve_bucket":
        args = [n_cf, int(n_ch), *head, *arrays, int(limit), ctypes.byref(_lib.PacxBucket(*bucket)), lo, hi, *per,
                _ptr(res), _ptr(res[1:])]
    else:
        first = np.ascontiguousarray(seg_first, np.int64)
        lim = np.ascontiguousarray(limits, np.int64)
        n_seg = len(lim)
        assert len(first) == n_seg + 1
        if op == "solve_segments":
            args = [n_cf, *head, *arrays, n_seg, first.ctypes.data, lim.ctypes.data, lo, hi, *per, _ptr(res)]
        else:
            assert op == "solve_peak"
            args = [n_cf, *head, *arrays, n_seg, first.ctypes.data, lim.ctypes.data, int(limit), lo, hi, *per,
                    _ptr(res[n_seg + 1:]), _ptr(res), _ptr(res[n_seg:])]
    rc = getattr(enc.lib, name)(enc.h, *args, enc._stream())
    assert rc == 0, (name, enc.lib.pacx_last_error(enc.h))


def result_words(res):
    """pacx_rate_result rows (int32 [n, 4]) -> (t, met, total) int64 arrays"""
    res = np.ascontiguousarray(res)
    return res[:, 0].astype(np.int64), res[:, 1].astype(np.int64), res[:, 2:].copy().view(np.int64)[:, 0]
