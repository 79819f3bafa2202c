"""Cost and yield of coding to an average bit rate (pacx_rate_curve_batch, pacx_rate_solve, pacfile.encode_stream_abr).

1. Times on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks):
   Encoder.rate_curve with the caps 128 and 320 kb/s, Encoder.rate_solve on the 128 kb/s curve (limit: 96 kb/s), and
   pacfile.encode_stream_abr as a whole (host PCM to host bytes, wall clock, cap 128 kb/s, 96 kb/s wanted).  The
   yardstick is Encoder.encode_pack_nmr (-3 dB, cap 128 kb/s) in the same process: the calls are timed in alternation,
   `rounds` times, with device events around a window of at least `min-seconds` of calls after `warmup`, as
   tools/rate_probe.py does, and every round is kept.  rate_solve reads its result back, so its time holds one
   device-to-host copy and the wait for it.
2. encode_pack_nmr's own time against the one profiles/rate_probe.json holds for the parent commit, beside the
   spread that file reports: the search now calls the evaluation function it shares with the curve.  (That figure is
   from another run; profiles/abr_search_ab.json holds an alternating run of both commits.)
3. On the four golden excerpts at 96 and 128 kb/s per channel, block switching on, cap 320 kb/s: the target found, the
   fill (body / limit), Report.share_audible() and the largest NMR, beside the constant-rate encode at the same rate.

    python tools/abr_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out profiles/abr_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as A  # noqa: E402

EXCERPTS = ["castanet", "harpsichord", "quar48_1", "spmg"]


def region(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps                       # ms per call


def timed(fn, min_seconds, warmup):
    """-> (ms per call, calls in the window): the window holds as many calls as fill min_seconds, judged from a pilot
    of `warmup` calls after `warmup` untimed ones"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    steps = max(warmup, int(np.ceil(min_seconds * 1e3 / region(fn, warmup))))
    return region(fn, steps), steps


def wall(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pcm = A.synth.stream(a.frames, 2)
    enc = A.context.encoder(48000, 128 / 48.0)
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    view = A.engine.PcmView.stream(planar)
    n_cf = view.n_cf
    vbr = enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0)
    c128 = enc.rate_curve(view, None, 128 / 48.0)
    c320 = enc.rate_curve(view, None, 320 / 48.0)
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    sol = enc.rate_solve(c128, None, limit)
    stream_pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks; rate_curve with "
                    "caps 128 and 320 kb/s, rate_solve on the 128 kb/s curve for 96 kb/s, encode_stream_abr (cap 128 kb/s, "
                    "96 kb/s) from host PCM to host bytes by the wall clock",
        "yardstick": "encode_pack_nmr (-3 dB, cap 128 kb/s) of this build in the same process, alternating rounds",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
        "device": torch.cuda.get_device_name(enc.device),
        "curve_rows": {"cap_128": c128["row"], "cap_320": c320["row"]},
        "solve_launch_pairs": 2 + int(np.ceil(np.log2(60 * 64 + 2))),
        "solve_on_workload": {"target_nmr_db": sol["target_nmr_db"], "met": sol["met"],
                              "fill": sol["total_bytes"] / limit},
        "encode_pack_nmr_ms": [], "rate_curve_128_ms": [], "rate_curve_320_ms": [], "rate_solve_ms": [],
        "encode_stream_abr_wall_ms": [], "calls_per_window": {},
    }
    calls = {
        "encode_pack_nmr": lambda: enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0, vbr),
        "rate_curve_128": lambda: enc.rate_curve(view, None, 128 / 48.0, c128),
        "rate_curve_320": lambda: enc.rate_curve(view, None, 320 / 48.0, c320),
        "rate_solve": lambda: enc.rate_solve(c128, None, limit),
    }
    abr = lambda: A.pacfile.encode_stream_abr(stream_pcm, 48000, kbps_per_channel=96, max_kbps_per_channel=128)  # noqa: E731
    abr()
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
        res["encode_stream_abr_wall_ms"].append(wall(abr, 3))
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    res["median_ms"] = med
    res["curve_128_over_nmr"] = med["rate_curve_128"] / med["encode_pack_nmr"]
    res["curve_320_over_nmr"] = med["rate_curve_320"] / med["encode_pack_nmr"]
    res["solve_over_nmr"] = med["rate_solve"] / med["encode_pack_nmr"]
    res["encode_stream_abr_wall_ms_median"] = float(np.median(res["encode_stream_abr_wall_ms"]))
    parent = os.path.join(ROOT, "profiles", "rate_probe.json")
    if os.path.exists(parent):
        old = json.load(open(parent))["encode_pack_nmr_ms"]
        res["encode_pack_nmr_against_parent"] = {
            "parent_ms_median": float(np.median(old)), "parent_spread_ms": float(max(old) - min(old)),
            "this_ms_median": med["encode_pack_nmr"],
            "this_spread_ms": float(max(res["encode_pack_nmr_ms"]) - min(res["encode_pack_nmr_ms"])),
            "difference_ms": med["encode_pack_nmr"] - float(np.median(old)),
            "note": "the parent's figure is the stored one of profiles/rate_probe.json, from another run and possibly "
                    "another machine of the same kind; the parent's library was not built or timed here",
        }

    res["excerpts"] = {}
    for name in EXCERPTS:
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        rows = {}
        both = A.quality.encode_stream_to_rate(x, sr, kbps_per_channel=[96, 128], block_switching=True)
        for kbps, (data, rep, info) in zip((96, 128), both):
            cbr, cbr_rep = A.quality.encode_stream_report(x, sr, kbps, block_switching=True)
            rows[f"{kbps} kb/s"] = {
                "target_nmr_db": info["target_nmr_db"],
                "fill": info["total_bytes"] / info["limit_bytes"],
                "kbps_per_channel": info["kbps_per_channel"],
                "capped_channel_blocks_share": float(info["capped"][info["written"]].mean()),
                "share_audible": rep.share_audible(), "worst_nmr_db": rep.maximum(), "bytes": len(data),
                "constant_rate": {"share_audible": cbr_rep.share_audible(), "worst_nmr_db": cbr_rep.maximum(),
                                  "bytes": len(cbr)},
            }
        res["excerpts"][name] = {"hops": len(x) // 1024, "sample_rate": sr, "rates": rows}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
