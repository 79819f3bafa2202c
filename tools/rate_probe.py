"""Cost and yield of the constant-quality mode (pacx_encode_pack_nmr_batch).

1. Time of Encoder.encode_pack_nmr against Encoder.encode_pack on the bench workload (8192 channel-frames of synthetic
   stereo, scalar mantissas, 128 kb/s, all long blocks; cap = the same 128 kb/s, target -3 dB).  encode_pack's kernels
   are untouched by the constant-quality mode, so THIS build's encode_pack stands in for the parent commit's as the
   yardstick (the parent's library is not built or run here; the result says so).  The two are timed in alternation,
   `rounds` times in one process, with device events around a window of at least `min-seconds` of calls after
   `warmup`, and every round is kept so that the spread can be read beside the difference.  encode_pack_budget (the same path without the search) is timed too.
2. Mean kb/s per channel and the share of channel-blocks that reach the cap at targets 0 / -3 / -6 dB, cap 320 kb/s,
   block switching on, on the four golden excerpts, beside the stream's worst NMR as quality.nmr_of_file reports it.

    python tools/rate_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out profiles/rate_probe.json]
"""
import argparse
import json
import os
import sys

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
    out = enc.encode_pack(view)
    vbr = enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0)
    budget = vbr["budget"].clone()
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo, scalar mantissas, all long blocks; encode_pack at 128 kb/s, "
                    "encode_pack_nmr at -3 dB with a 128 kb/s cap",
        "yardstick": "encode_pack of this build, in the same process: the constant-rate kernels are the parent commit's, "
                     "unchanged; the parent's own library was not built or timed",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
        "device": torch.cuda.get_device_name(enc.device),
        "encode_pack_ms": [], "encode_pack_nmr_ms": [], "encode_pack_budget_ms": [], "calls_per_window": {},
    }
    calls = {
        "encode_pack": lambda: enc.encode_pack(view, None, out),
        "encode_pack_nmr": lambda: enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0, vbr),
        "encode_pack_budget": lambda: enc.encode_pack_budget(view, None, budget, vbr),
    }
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
    cbr, nmr = float(np.median(res["encode_pack_ms"])), float(np.median(res["encode_pack_nmr_ms"]))
    res["encode_pack_M_cf_per_s"] = n_cf / cbr / 1e3
    res["encode_pack_nmr_M_cf_per_s"] = n_cf / nmr / 1e3
    res["nmr_over_pack"] = nmr / cbr
    st = vbr["status"].cpu().numpy()
    res["workload_capped_share"] = float(np.mean((st & A._lib.ST_RATE_CAP) != 0))
    res["workload_mean_budget_bits"] = float(vbr["budget"][:, 0].double().mean().item())

    res["excerpts"] = {}
    for name in EXCERPTS:
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        rows = {}
        for target in (0.0, -3.0, -6.0):
            data, rep, info = A.quality.encode_stream_to_nmr(x, sr, target, max_kbps_per_channel=320, block_switching=True)
            written = info["written"]
            rows[f"{target:+.0f} dB"] = {
                "kbps_per_channel": info["kbps_per_channel"],
                "capped_channel_blocks_share": float(info["capped"][written].mean()),
                "worst_nmr_db": rep.maximum(),
                "bytes": len(data),
            }
        rows["128 kb/s constant rate"] = {"bytes": len(A.pacfile.encode_stream(x, sr, 128, block_switching=True))}
        res["excerpts"][name] = {"hops": len(x) // 1024, "sample_rate": sr, "targets": rows}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
