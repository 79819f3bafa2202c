"""Cost of the whole-grid rate profile and of the chunked average-bit-rate encode (pacx_band_profile, pacx_profile_solve,
pacfile.encode_stream_abr_chunked).

On the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks), cap
128 kb/s, 96 kb/s wanted:
  Encoder.band_profile at G = 3841 (+-30 dB) on the band curve, beside Encoder.band_curve (what a chunk pays anyway),
  Encoder.band_solve (the 14 picks the profile replaces) and Encoder.profile_solve.  The two solves read their result
  back, so their times hold one device-to-host copy and the wait for it.
  pacfile.encode_stream_abr_chunked as a whole, host PCM to host bytes by the wall clock, with chunks of `chunk-hops`
  blocks and as one chunk, against pacfile.encode_stream_abr(allocation="band") on the same stream.
The yardsticks -- band_curve, band_solve and the one-batch call -- are this build's own in the same process; none of
their kernels differs from the build before.  The calls are timed in alternation, `rounds` times, with device events
around a window of at least `min-seconds` of calls after `warmup`, as tools/band_probe.py does; every round is kept.

    python tools/profile_probe.py [--frames 4096] [--chunk-hops 512] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--chunk-hops", type=int, default=512)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_probe.json"))
    a = ap.parse_args()
    import torch
    import audio_codec_amd as A
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf = view.n_cf
    cap = 128 / 48.0
    curve = enc.band_curve(view, None, cap)
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    profile = enc.band_profile(curve)
    sol, psol = enc.band_solve(curve, limit), enc.profile_solve(profile, limit)
    assert (sol["target_nmr_db"], sol["met"], sol["total_bytes"]) == \
        (psol["target_nmr_db"], psol["met"], psol["total_bytes"])
    scratch = torch.zeros_like(profile)
    stream_pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    hops = len(stream_pcm) // 1024
    calls = {
        "band_curve": lambda: enc.band_curve(view, None, cap, curve),
        "band_profile": lambda: enc.band_profile(curve, out=scratch),
        "band_solve": lambda: enc.band_solve(curve, limit),
        "profile_solve": lambda: enc.profile_solve(profile, limit),
    }
    size = dict(kbps_per_channel=96, max_kbps_per_channel=128)
    walls = {
        "encode_stream_abr_band": lambda: A.pacfile.encode_stream_abr(stream_pcm, 48000, allocation="band", **size),
        "encode_stream_abr_chunked": lambda: A.pacfile.encode_stream_abr_chunked(stream_pcm, 48000,
                                                                                 chunk_hops=a.chunk_hops, **size),
        "encode_stream_abr_chunked_one_chunk": lambda: A.pacfile.encode_stream_abr_chunked(stream_pcm, 48000,
                                                                                           chunk_hops=hops, **size),
    }
    one = walls["encode_stream_abr_band"]()
    assert walls["encode_stream_abr_chunked"]() == one and walls["encode_stream_abr_chunked_one_chunk"]() == one
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, cap 128 kb/s; "
                    f"band_profile at G = {profile.numel()} on the band curve, band_solve and profile_solve for 96 kb/s; "
                    f"encode_stream_abr_chunked (chunks of {a.chunk_hops} blocks, and one chunk of {hops}) and "
                    "encode_stream_abr(allocation='band') from host PCM to host bytes by the wall clock, the same bytes",
        "yardsticks": "band_curve, band_solve and encode_stream_abr(allocation='band') of this build in the same "
                      "process, alternating rounds",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds, "chunk_hops": a.chunk_hops,
        "device": torch.cuda.get_device_name(enc.device),
        "solve": {"target_nmr_db": psol["target_nmr_db"], "met": psol["met"], "fill": psol["total_bytes"] / limit},
        "calls_per_window": {},
    }
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
    res["band_profile_over_band_curve"] = med["band_profile"] / med["band_curve"]
    res["band_profile_over_band_solve"] = med["band_profile"] / med["band_solve"]
    res["profile_solve_over_band_solve"] = med["profile_solve"] / med["band_solve"]
    res["chunked_over_one_batch_wall"] = med["encode_stream_abr_chunked_wall"] / med["encode_stream_abr_band_wall"]
    res["one_chunk_over_one_batch_wall"] = med["encode_stream_abr_chunked_one_chunk_wall"] / med["encode_stream_abr_band_wall"]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
