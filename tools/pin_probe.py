"""Cost and yield of per-block targets under a leaky bucket (pacx_bucket_through, pacx_band_solve_bucket_pinned /
pacx_rate_solve_bucket_pinned, pacfile.encode_stream_abr_pinned).

1. Cost, on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks,
   curves with the cap 128 kb/s): Encoder.bucket_through beside bucket_scan at 4096 and 131 072 hops of drawn record
   sizes, and both pinned solves at max_phases 1, 4 and 8 -- the 96 kb/s size, a buffer of a quarter second of the
   96 kb/s drain, the default step of 1 dB -- beside band_solve_bucket / rate_solve_bucket of the same build in the
   same process.  The calls are timed in alternation, `rounds` times, with device events around a window of at least
   `min-seconds` of calls after `warmup`, as tools/bucket_probe.py does, and every round is kept.  Every call reads
   its result back.  What to compare with: a pinned solve launches max_phases (2 pairs + 2) + 3 kernels whatever the
   data, a buffered one 2 pairs + 1; the step kernels of a phase whose level is found return before they scan, the
   picks between them run.
2. pacfile.encode_stream_abr_pinned beside encode_stream_abr_buffered on the same PCM by the wall clock, `rounds`
   alternating rounds of `stream-calls` calls each.
3. Yield, on the four golden excerpts, block switching on, cap 320 kb/s, allocation "band", a 96 kb/s average and
   drain with buffers of 0.25, 1 and 4 seconds of the drain, the defaults (a step of 1 dB, 8 phases): phases used,
   open, blocks pinned per phase, the levels, bytes, the worst band and the share of bands above the mask, beside the
   one-target stream (encode_stream_abr_buffered) and the whole-stream solve.

    python tools/pin_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--stream-calls 3]
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

PHASES = (1, 4, 8)


def cost(a, A, torch):
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf, n_ch = view.n_cf, 2
    curves = {"rate": enc.rate_curve(view, None, 128 / 48.0), "band": enc.band_curve(view, None, 128 / 48.0)}
    limit = int(96 * 1000 * n_ch * view.n_frames * 1024 / 48000 / 8)
    bucket = A.pacfile.bucket(96, n_ch, 48000, 96 * 1000 * n_ch // 8 // 4)         # a quarter second of the drain
    calls = {"band_solve_bucket": lambda: enc.band_solve_bucket(curves["band"], n_ch, limit, bucket),
             "rate_solve_bucket": lambda: enc.rate_solve_bucket(curves["rate"], None, n_ch, limit, bucket)}
    for k in PHASES:
        calls[f"band_solve_bucket_pinned_{k}"] = lambda k=k: enc.band_solve_bucket_pinned(curves["band"], n_ch, limit, bucket,
                                                                                          max_phases=k)
        calls[f"rate_solve_bucket_pinned_{k}"] = lambda k=k: enc.rate_solve_bucket_pinned(curves["rate"], None, n_ch, limit,
                                                                                          bucket, max_phases=k)
    rng = np.random.default_rng(1)
    for hops in (4096, 131072):
        nb = torch.as_tensor(rng.integers(200, 800, hops * n_ch).astype(np.int32), device=enc.device)
        calls[f"bucket_scan_{hops}"] = lambda nb=nb: enc.bucket_scan(nb, n_ch, bucket)
        calls[f"bucket_through_{hops}"] = lambda nb=nb: enc.bucket_through(nb, n_ch, bucket)
    on = {}
    for kind in ("band", "rate"):
        buf = calls[f"{kind}_solve_bucket"]()
        on[kind] = {"solve_bucket_target_nmr_db": buf["target_nmr_db"], "solve_bucket_met": buf["met"],
                    "solve_bucket_total_bytes": buf["total_bytes"]}
        for k in PHASES:
            sol = calls[f"{kind}_solve_bucket_pinned_{k}"]()
            phase_of = sol["phase_of"].cpu().numpy()
            on[kind][f"pinned_{k}"] = {"target_nmr_db": sol["target_nmr_db"], "met": sol["met"], "phases": sol["phases"],
                                       "open": sol["open"], "hops_pinned": int((phase_of >= 0).sum()),
                                       "total_bytes": sol["total_bytes"], "peak_bytes": sol["bucket"]["peak_bytes"]}
    pairs = 2 + int(np.ceil(np.log2(60 * 64 + 2)))
    res = {"workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, curves with "
                       f"the cap 128 kb/s; limit {limit} bytes (96 kb/s), bucket {tuple(bucket)}, pin_step_db 1.0; every "
                       f"call reads its result back; a buffered solve is {2 * pairs + 1} launches, a pinned one "
                       f"{[k * (2 * pairs + 2) + 3 for k in PHASES]} at max_phases {list(PHASES)}",
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
    res["range_ms"] = {k: [min(res[k + "_ms"]), max(res[k + "_ms"])] for k in calls}
    for kind in ("band", "rate"):
        for k in PHASES:
            res[f"{kind}_pinned_{k}_over_{kind}_solve_bucket"] = med[f"{kind}_solve_bucket_pinned_{k}"] / med[f"{kind}_solve_bucket"]
    for hops in (4096, 131072):
        res[f"bucket_through_over_bucket_scan_{hops}"] = med[f"bucket_through_{hops}"] / med[f"bucket_scan_{hops}"]
    # the streams, by the wall clock
    streams = {"encode_stream_abr_buffered": lambda: A.pacfile.encode_stream_abr_buffered(pcm, 48000, 96, bucket.size_bytes,
                                                                                          max_kbps_per_channel=128),
               "encode_stream_abr_pinned": lambda: A.pacfile.encode_stream_abr_pinned(pcm, 48000, 96, bucket.size_bytes,
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
        kw = dict(block_switching=True, allocation="band")

        def row(data, target):
            rep = A.quality.nmr_of_file(x, data, block_switching=True)
            return {"target_nmr_db": target, "bytes": len(data), "worst_nmr_db": rep.maximum(),
                    "share_audible": rep.share_audible()}
        data, _, info = A.quality.encode_stream_to_rate(x, sr, kbps_per_channel=96, **kw)
        rows = {"whole_stream": row(data, info["target_nmr_db"])}
        one_second = 96 * 1000 * n_ch // 8
        for seconds in (0.25, 1, 4):
            size = int(seconds * one_second)
            try:
                data, info = A.quality.encode_stream_to_buffer(x, sr, 96, size, **kw)
                rows[f"buffer_{seconds:g}s_one_target"] = dict(row(data, info["target_nmr_db"]), buffer_bytes=size,
                                                               peak_bytes=info["peak_bytes"])
                data, info = A.quality.encode_stream_to_buffer_pinned(x, sr, 96, size, **kw)
                phase_of, t = info["phase_of"], info["block_target_nmr_db"]
                free = phase_of < 0
                rows[f"buffer_{seconds:g}s_pinned"] = dict(
                    row(data, info["target_nmr_db"]), buffer_bytes=size, peak_bytes=info["peak_bytes"],
                    phases=info["phases"], open=info["open"], blocks=int(len(phase_of)), blocks_free=int(free.sum()),
                    blocks_pinned_per_phase=[int((phase_of == k).sum()) for k in range(int(phase_of.max()) + 1)],
                    levels_nmr_db=sorted({float(v) for v in t}, reverse=True),
                    block_target_nmr_db_min_median_max=[float(t.min()), float(np.median(t)), float(t.max())])
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
        sys.exit("pin_probe: no GPU; nothing here is measured without one")
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
