"""Cost of the buffered solve in chunks (include/pacx_bucket_kept.h: pacx_band_bytes_thresholds / pacx_rate_bytes_thresholds,
pacx_bucket_scan_targets, pacfile.encode_stream_abr_buffered_kept).

1. A pass, on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks,
   curves with the cap 128 kb/s kept as thresholds, resident on the device): the bytes kernel at 15 targets and
   bucket_scan_targets over them, against 15 times the existing pair -- the single-target pick on the kept curve
   (pacx_*_pick_thresholds) and pacx_bucket_scan of its n_bytes -- in the same process, for both kinds of curve.  Both
   sides are called through the C entry points with their outputs made once and nothing read back.  Timed in
   alternation, `rounds` times, with device events around a window of at least `min-seconds` of calls after `warmup`, as
   tools/band_probe.py does; every round is kept.
2. Per-target scaling: the bytes kernels alone at 1 and 31 targets beside the single-target pick alone.
3. End to end, host PCM to .pac bytes, 4096 blocks in chunks of 512 by the wall clock: encode_stream_abr_buffered_kept at
   levels 1, 4 and 5 beside encode_stream_abr_kept and the one-batch encode_stream_abr_buffered, `rounds` alternating
   rounds of `stream-calls` calls each.

    python tools/bucket_kept_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--stream-calls 2]
                                      [--out FILE] [--no-streams]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from band_probe import timed, workload          # noqa: E402

LO, HI = -30.0, 30.0


def passes(a, A, torch):
    from audio_codec_amd.curves import BAND, RATE
    pcm, enc, view = workload(A, torch, a.frames)
    ptr = A.engine._ptr
    n_cf, n_ch = view.n_cf, 2
    kept = {"band": enc.band_thresholds(enc.band_curve(view, None, 128 / 48.0), LO, HI),
            "rate": enc.rate_thresholds(enc.rate_curve(view, None, 128 / 48.0), LO, HI)}
    bucket = A.pacfile.bucket(96, n_ch, 48000, 96 * 1000 * n_ch // 8)              # one second of the drain
    b = A._lib.PacxBucket(*bucket)
    targets = {n: torch.as_tensor(np.linspace(-640, 640, n).astype(np.int32), device=enc.device) for n in (1, 15, 31)}
    rows = torch.zeros((31, n_cf), dtype=torch.int32, device=enc.device)
    acc = torch.as_tensor(enc.bucket_no_hop(bucket, 31), device=enc.device)
    result = torch.zeros(5, dtype=torch.int64, device=enc.device)
    calls = {}
    for name, kind in (("band", BAND), ("rate", RATE)):
        k = kept[name]
        checked = enc._checked(kind, k, name, True)
        rng = enc._kept_range(name, k)
        out = enc._picked(kind, checked)
        outs = (ptr(out[kind.per_cf.key]), ptr(out["n_bytes"]), ptr(out["capped"]))
        op = getattr(enc, f"{name}_bytes_thresholds")

        def pick(t, name=name, checked=checked, rng=rng, outs=outs):
            enc._curve_call(f"{name}_pick_thresholds", checked, *rng, ctypes.c_double(t / 64.0), *outs)

        def pair(t, pick=pick, out=out):
            pick(t)
            enc._call("pacx_bucket_scan", ctypes.c_int64(n_cf // n_ch), n_ch, ptr(out["n_bytes"]), ctypes.byref(b), None,
                      ptr(result), enc._stream())

        def composed(pair=pair):
            for t in np.linspace(-640, 640, 15).astype(int):
                pair(int(t))

        def one_pass(n=15, op=op, k=k):
            op(k, targets[n], out=rows[:n])
            enc.bucket_scan_targets(rows[:n], n_ch, bucket[0], bucket[1], 0, acc[:n])

        calls[f"{name}_pass_15"] = one_pass
        calls[f"{name}_pairs_15"] = composed
        calls[f"{name}_pick_1"] = lambda pick=pick: pick(0)
        for n in (1, 31):
            calls[f"{name}_bytes_{n}"] = lambda n=n, op=op, k=k: op(k, targets[n], out=rows[:n])
    res = {"workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, curves with the "
                       f"cap 128 kb/s kept as thresholds on [{LO:g}, {HI:g}] dB, resident; bucket {tuple(bucket)}; C entry "
                       f"points, outputs made once, nothing read back",
           "rate_row": int(kept["rate"]["row"]), "band_stride": int(enc.band_stride),
           "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(enc.device), "calls_per_window": {}}
    for name in calls:
        res[name + "_ms"] = []
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(torch, fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    res["median_ms"] = med
    for name in ("band", "rate"):
        res[f"{name}_pass_median_below_pairs_fastest"] = med[f"{name}_pass_15"] < min(res[f"{name}_pairs_15_ms"])
        res[f"{name}_pairs_over_pass"] = med[f"{name}_pairs_15"] / med[f"{name}_pass_15"]
        res[f"{name}_bytes_31_over_pick_1"] = med[f"{name}_bytes_31"] / med[f"{name}_pick_1"]
        res[f"{name}_bytes_1_over_pick_1"] = med[f"{name}_bytes_1"] / med[f"{name}_pick_1"]
    return res, pcm


def streams(a, A, torch, pcm):
    kw = dict(max_kbps_per_channel=128)
    size = 96 * 1000 * 2 // 8
    calls = {"encode_stream_abr_kept": lambda: A.pacfile.encode_stream_abr_kept(pcm, 48000, 96, chunk_hops=512,
                                                                                allocation="budget", **kw),
             "encode_stream_abr_buffered": lambda: A.pacfile.encode_stream_abr_buffered(pcm, 48000, 96, size, **kw)}
    for levels in (1, 4, 5):
        calls[f"encode_stream_abr_buffered_kept_levels_{levels}"] = \
            lambda levels=levels: A.pacfile.encode_stream_abr_buffered_kept(pcm, 48000, 96, size, chunk_hops=512,
                                                                            levels=levels, **kw)
    same = calls["encode_stream_abr_buffered"]()
    wall = {k: [] for k in calls}
    for name, fn in calls.items():
        if name.startswith("encode_stream_abr_buffered_kept"):
            assert fn() == same, name
        else:
            fn()
    for _ in range(a.rounds):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.stream_calls):
                fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / a.stream_calls)
    return {"stream": f"{len(pcm) // 1024} blocks of stereo at 48 kHz, chunks of 512, allocation 'budget', 96 kb/s, a buffer "
                      f"of {size} bytes; the buffered streams' bytes are equal",
            "stream_wall_ms": wall, "stream_wall_ms_median": {k: float(np.median(v)) for k, v in wall.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stream-calls", type=int, default=2)
    ap.add_argument("--no-streams", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import audio_codec_amd as A
    if not torch.cuda.is_available():
        sys.exit("bucket_kept_probe: no GPU; nothing here is measured without one")
    res, pcm = passes(a, A, torch)
    if not a.no_streams:
        res.update(streams(a, A, torch, pcm))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
