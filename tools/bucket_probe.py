"""Cost and yield of the leaky bucket (pacx_bucket_scan, pacx_band_solve_bucket / pacx_rate_solve_bucket,
pacfile.encode_stream_abr_buffered).

1. Cost, on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks,
   curves with the cap 128 kb/s): Encoder.bucket_scan at 4096 and 131 072 hops of drawn record sizes, and
   band_solve_bucket / rate_solve_bucket -- the 96 kb/s size, a buffer of one second of the 96 kb/s drain -- beside
   band_solve / rate_solve of the same build in the same process.  The calls are timed in alternation, `rounds` times,
   with device events around a window of at least `min-seconds` of calls after `warmup`, as tools/band_probe.py does,
   and every round is kept.  Every call reads its result back, so the times hold one device-to-host copy and the wait
   for it.  What to compare with: a buffered solve is as many pairs as the plain one, each a pick and the scan step
   of one workgroup instead of the plain solve's pick and its one-thread step.
2. pacfile.encode_stream_abr_buffered beside encode_stream_abr on the same PCM by the wall clock, `rounds` alternating
   rounds of `stream-calls` calls each.
3. Yield, on the four golden excerpts, block switching on, cap 320 kb/s, allocation "band", a 96 kb/s average and
   drain with buffers of 0.25, 1 and 4 seconds of the drain: the target found, the worst band and the share of bands
   above the mask, beside the whole-stream solve and segment_hops = 8 at the same rate.

    python tools/bucket_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--stream-calls 3]
                                 [--out FILE] [--no-excerpts] [--no-cost]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from band_probe import EXCERPTS, timed, workload          # noqa: E402


def cost(a, A, torch):
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf, n_ch = view.n_cf, 2
    r128, b128 = enc.rate_curve(view, None, 128 / 48.0), enc.band_curve(view, None, 128 / 48.0)
    limit = int(96 * 1000 * n_ch * view.n_frames * 1024 / 48000 / 8)
    bucket = A.pacfile.bucket(96, n_ch, 48000, 96 * 1000 * n_ch // 8)              # one second of the drain
    calls = {"band_solve": lambda: enc.band_solve(b128, limit),
             "band_solve_bucket": lambda: enc.band_solve_bucket(b128, n_ch, limit, bucket),
             "rate_solve": lambda: enc.rate_solve(r128, None, limit),
             "rate_solve_bucket": lambda: enc.rate_solve_bucket(r128, None, n_ch, limit, bucket)}
    rng = np.random.default_rng(1)
    for hops in (4096, 131072):
        nb = torch.as_tensor(rng.integers(200, 800, hops * n_ch).astype(np.int32), device=enc.device)
        calls[f"bucket_scan_{hops}"] = lambda nb=nb: enc.bucket_scan(nb, n_ch, bucket)
    on = {}
    for kind in ("band", "rate"):
        plain, buf = calls[f"{kind}_solve"](), calls[f"{kind}_solve_bucket"]()
        on[kind] = {"solve_target_nmr_db": plain["target_nmr_db"], "solve_bucket_target_nmr_db": buf["target_nmr_db"],
                    "solve_bucket_met": buf["met"], "peak_bytes": buf["bucket"]["peak_bytes"],
                    "plain_peak_bytes": enc.bucket_scan(plain["n_bytes"], n_ch, bucket)["peak_bytes"]}
    pairs = 2 + int(np.ceil(np.log2(60 * 64 + 2)))
    res = {"workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, curves with "
                       f"the cap 128 kb/s; limit {limit} bytes (96 kb/s), bucket {tuple(bucket)}; every call reads its "
                       f"result back; a solve is {pairs} pairs",
           "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(enc.device), "on_workload": on, "calls_per_window": {}}
    for k in calls:
        res[k + "_ms"] = []
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(torch, fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    res["median_ms"] = med
    res["spread"] = {k: (max(res[k + "_ms"]) - min(res[k + "_ms"])) / med[k] for k in calls}
    for kind in ("band", "rate"):
        res[f"{kind}_solve_bucket_over_{kind}_solve"] = med[f"{kind}_solve_bucket"] / med[f"{kind}_solve"]
        res[f"{kind}_step_ms_per_pair"] = (med[f"{kind}_solve_bucket"] - med[f"{kind}_solve"]) / pairs
    # the streams, by the wall clock
    kw = dict(kbps_per_channel=96, max_kbps_per_channel=128)
    streams = {"encode_stream_abr": lambda: A.pacfile.encode_stream_abr(pcm, 48000, **kw),
               "encode_stream_abr_buffered": lambda: A.pacfile.encode_stream_abr_buffered(pcm, 48000, 96, bucket.size_bytes,
                                                                                          max_kbps_per_channel=128)}
    wall = {k: [] for k in streams}
    for fn in streams.values():
        fn()
    for _ in range(a.rounds):
        for name, fn in streams.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.stream_calls):
                fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / a.stream_calls)
    res["stream_wall_ms"] = wall
    res["stream_wall_ms_median"] = {k: float(np.median(v)) for k, v in wall.items()}
    return res


def yields(A):
    out = {}
    for name in EXCERPTS:
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        n_ch = x.shape[1]
        kw = dict(kbps_per_channel=96, block_switching=True, allocation="band")

        def row(data, target):
            rep = A.quality.nmr_of_file(x, data, block_switching=True)
            return {"target_nmr_db": target, "bytes": len(data), "worst_nmr_db": rep.maximum(),
                    "share_audible": rep.share_audible()}
        data, _, info = A.quality.encode_stream_to_rate(x, sr, **kw)
        rows = {"whole_stream": row(data, info["target_nmr_db"])}
        one_second = 96 * 1000 * n_ch // 8
        rows["whole_stream"]["peak_bytes_at_96_drain"] = A.quality.buffer_report(data, 96, 1 << 40)["peak_bytes"]
        try:
            data, _, info = A.quality.encode_stream_to_rate(x, sr, segment_hops=8, **kw)
            t = info["segments"]["target_nmr_db"]
            rows["segment_hops_8"] = dict(row(data, None), target_nmr_db_min_median_max=[float(t.min()), float(np.median(t)),
                                                                                       float(t.max())])
        except ValueError as e:
            rows["segment_hops_8"] = {"unreachable": str(e)}
        for seconds in (0.25, 1, 4):
            size = int(seconds * one_second)
            try:
                data, info = A.quality.encode_stream_to_buffer(x, sr, 96, size, block_switching=True, allocation="band")
                rows[f"buffer_{seconds:g}s"] = dict(row(data, info["target_nmr_db"]), buffer_bytes=size,
                                                    peak_bytes=info["peak_bytes"], peak_block=info["peak_block"],
                                                    mean_kbps_per_channel=info["mean_kbps_per_channel"],
                                                    max_kbps_per_channel_seen=info["max_kbps_per_channel_seen"])
            except ValueError as e:
                rows[f"buffer_{seconds:g}s"] = {"buffer_bytes": size, "unreachable": str(e)}
        out[name] = {"hops": len(x) // 1024, "sample_rate": sr, **rows}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stream-calls", type=int, default=3)
    ap.add_argument("--no-excerpts", action="store_true")
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import audio_codec_amd as A
    if not torch.cuda.is_available():
        sys.exit("bucket_probe: no GPU; nothing here is measured without one")
    res = {} if a.no_cost else cost(a, A, torch)
    if not a.no_excerpts:
        res["excerpts"] = yields(A)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
