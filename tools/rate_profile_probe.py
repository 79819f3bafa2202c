"""Cost of the whole-grid profile of a rate curve and of the chunked average-bit-rate encode with allocation="budget"
(pacx_rate_profile, pacx_rate_profile_segments, pacx_rate_pick, pacfile.encode_stream_abr_chunked(allocation="budget")).

The procedure of tools/profile_probe.py.  On the bench workload (8192 channel-frames of synthetic stereo at 48 kHz,
scalar mantissas, all long blocks), for the caps 128 and 320 kb/s (the curve's rows grow with the cap), 96 kb/s wanted:
  Encoder.rate_profile at G = 3841 (+-30 dB) beside Encoder.rate_curve (what a chunk pays anyway) and Encoder.rate_solve
  (the 14 picks the profile replaces; it reads its result back);
  Encoder.rate_profile_segments with the frames as 1 / 64 / 8192 segments;
  Encoder.rate_pick at the target found beside Encoder.rate_solve;
  pacfile.encode_stream_abr_chunked(allocation="budget") as a whole, host PCM to host bytes by the wall clock, in chunks
  of `chunk-hops` blocks, against pacfile.encode_stream_abr(allocation="budget") on the same stream: the same bytes.
The yardsticks -- rate_curve, rate_solve and the one-batch call -- are this build's own in the same process; none of
their kernels differs from the build before.  The calls are timed in alternation, `rounds` times, with device events
around a window of at least `min-seconds` of calls after `warmup`; every round is kept.

    python tools/rate_profile_probe.py [--frames 4096] [--chunk-hops 512] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from band_probe import timed, wall, workload  # noqa: E402

SEGMENTS = (1, 64, 8192)


def one_cap(A, torch, a, pcm, enc, view, cap_kbps):
    n_cf = view.n_cf
    cap = cap_kbps / 48.0
    curve = enc.rate_curve(view, None, cap)
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    profile = enc.rate_profile(curve)
    sol, psol = enc.rate_solve(curve, None, limit), enc.profile_solve(profile, limit)
    assert (sol["target_nmr_db"], sol["met"], sol["total_bytes"]) == \
        (psol["target_nmr_db"], psol["met"], psol["total_bytes"])
    pick = enc.rate_pick(curve, sol["target_nmr_db"])
    assert all(bool((pick[k] == sol[k]).all()) for k in ("budget", "n_bytes", "capped"))
    scratch = torch.zeros_like(profile)
    rows = {n: torch.zeros((n, profile.numel()), dtype=torch.int64, device=enc.device) for n in SEGMENTS}
    for n in SEGMENTS:
        enc.rate_profile_segments(curve, -(-n_cf // n), 0, out=rows[n])
        assert bool((rows[n].sum(dim=0) == profile).all())
    calls = {
        "rate_curve": lambda: enc.rate_curve(view, None, cap, curve),
        "rate_profile": lambda: enc.rate_profile(curve, out=scratch),
        "rate_solve": lambda: enc.rate_solve(curve, None, limit),
        "rate_pick": lambda: enc.rate_pick(curve, sol["target_nmr_db"]),
    }
    for n in SEGMENTS:
        calls[f"rate_profile_segments_{n}"] = lambda n=n: enc.rate_profile_segments(curve, -(-n_cf // n), 0, out=rows[n])
    stream_pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    size = dict(kbps_per_channel=96, max_kbps_per_channel=cap_kbps)
    walls = {
        "encode_stream_abr_budget": lambda: A.pacfile.encode_stream_abr(stream_pcm, 48000, allocation="budget", **size),
        "encode_stream_abr_chunked_budget": lambda: A.pacfile.encode_stream_abr_chunked(
            stream_pcm, 48000, chunk_hops=a.chunk_hops, allocation="budget", **size),
    }
    assert walls["encode_stream_abr_chunked_budget"]() == walls["encode_stream_abr_budget"]()
    res = {"cap_kbps": cap_kbps, "row": curve["row"], "n_cf": n_cf, "G": profile.numel(),
           "solve": {"target_nmr_db": psol["target_nmr_db"], "met": psol["met"], "fill": psol["total_bytes"] / limit},
           "calls_per_window": {}}
    for k in calls:
        res[k + "_ms"] = []
    for k in walls:
        res[k + "_wall_ms"] = []
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(torch, fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
        for name, fn in walls.items():
            res[name + "_wall_ms"].append(wall(torch, fn, 3))
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    med.update({k + "_wall": float(np.median(res[k + "_wall_ms"])) for k in walls})
    res["median_ms"] = med
    res["spread_ms"] = {k: max(res[k + "_ms"]) - min(res[k + "_ms"]) for k in calls}
    res["spread_ms"].update({k + "_wall": max(res[k + "_wall_ms"]) - min(res[k + "_wall_ms"]) for k in walls})
    res["rate_profile_over_rate_curve"] = med["rate_profile"] / med["rate_curve"]
    res["rate_profile_over_rate_solve"] = med["rate_profile"] / med["rate_solve"]
    res["rate_pick_over_rate_solve"] = med["rate_pick"] / med["rate_solve"]
    res["chunked_over_one_batch_wall"] = med["encode_stream_abr_chunked_budget_wall"] / med["encode_stream_abr_budget_wall"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--chunk-hops", type=int, default=512)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--caps", type=float, nargs="+", default=[128, 320])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_profile_probe.json"))
    a = ap.parse_args()
    import torch
    import audio_codec_amd as A
    pcm, enc, view = workload(A, torch, a.frames)
    res = {
        "workload": f"{view.n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks; per cap "
                    "rate: rate_profile at G = 3841 on the rate curve beside rate_curve and rate_solve for 96 kb/s, "
                    f"rate_profile_segments with the frames as {' / '.join(map(str, SEGMENTS))} segments, rate_pick at the "
                    f"target found; encode_stream_abr_chunked(allocation='budget') in chunks of {a.chunk_hops} blocks and "
                    "encode_stream_abr(allocation='budget') from host PCM to host bytes by the wall clock, the same bytes",
        "yardsticks": "rate_curve, rate_solve and encode_stream_abr(allocation='budget') of this build in the same "
                      "process, alternating rounds",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds, "chunk_hops": a.chunk_hops,
        "device": torch.cuda.get_device_name(enc.device),
        "caps": [one_cap(A, torch, a, pcm, enc, view, cap) for cap in a.caps],
    }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
