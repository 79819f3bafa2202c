"""Cost of the per-segment rate profile and of segments and peaks in the chunked average-bit-rate encode
(pacx_band_profile_segments, pacx_profile_solve_segments, pacx_profile_clamp_add, pacx_band_pick_segments,
pacfile.encode_stream_abr_chunked(segment_hops=..., peak_kbps_per_channel=...)).

On the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks), cap
128 kb/s, G = 3841 (+-30 dB):
  Encoder.band_profile_segments with the curve cut into 1, 64 and 8192 segments beside Encoder.band_profile;
  Encoder.profile_solve_segments followed by Encoder.profile_clamp_add on 64 and on 8192 rows, nothing read back: on
  copies of the rows that no other call adds to, with limits that spread the targets over the grid (a quarter of the
  rows cannot be reached);
  Encoder.band_pick_segments with 64 segments beside Encoder.band_pick;
  pacfile.encode_stream_abr_chunked with and without segment_hops=8, peak_kbps_per_channel=128, host PCM to host bytes
  by the wall clock.
The yardsticks are this build's own calls in the same process.  The procedure is tools/profile_probe.py's: the calls are
timed in alternation, `rounds` times, with device events around a window of at least `min-seconds` of calls after
`warmup`; every round is kept.

    python tools/segprofile_probe.py [--frames 4096] [--chunk-hops 512] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segprofile_probe.json"))
    a = ap.parse_args()
    import torch
    import audio_codec_amd as A
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf = view.n_cf
    cap = 128 / 48.0
    curve = enc.band_curve(view, None, cap)
    profile = enc.band_profile(curve)
    G = profile.numel()
    counts = sorted({1, 64, n_cf})
    rows = {n: enc.band_profile_segments(curve, n_cf // n, 0) for n in counts}
    for n in counts:
        assert torch.equal(rows[n].sum(dim=0), profile)
    # the solve and the clamped sum work on copies that nothing adds to, against limits that spread the targets over
    # the grid: row s is asked for its own size at a grid point that moves with s, every fourth row for one byte less
    # than its smallest size, which it cannot reach
    solve_rows = {n: rows[n].clone() for n in counts if n > 1}
    sums = {n: int(solve_rows[n].sum().item()) for n in solve_rows}
    limits = {}
    for n, r in solve_rows.items():
        s = torch.arange(n, device=enc.device)
        at = (s * 2654435761) % G
        limit = r.gather(1, at[:, None])[:, 0]
        limits[n] = torch.where(s % 4 == 3, (r[:, -1] - 1).clamp(min=0), limit).contiguous()
    outs = {n: (torch.zeros((n, 4), dtype=torch.int32, device=enc.device),
                torch.zeros((n,), dtype=torch.int64, device=enc.device)) for n in solve_rows}
    scratch, star = torch.zeros_like(profile), torch.zeros_like(profile)
    targets = torch.zeros(64, dtype=torch.int32, device=enc.device)
    plain, seg = enc.band_pick(curve, 0.0), enc.band_pick_segments(curve, n_cf // 64, 0, targets)
    assert all(torch.equal(plain[k], seg[k]) for k in ("bit_alloc", "n_bytes", "capped"))

    def add_rows(n):
        return lambda: enc.band_profile_segments(curve, n_cf // n, 0, out=rows[n])

    def solve_clamp(n):
        def fn():
            enc.profile_solve_segments(solve_rows[n], limits[n], out=outs[n])
            enc.profile_clamp_add(solve_rows[n], outs[n][0], out=star)
        return fn
    calls = {"band_profile": lambda: enc.band_profile(curve, out=scratch)}
    calls.update({f"band_profile_segments_{n}": add_rows(n) for n in counts})
    calls.update({f"solve_segments_clamp_add_{n}": solve_clamp(n) for n in counts if n > 1})
    calls["band_pick"] = lambda: enc.band_pick(curve, 0.0)
    calls["band_pick_segments_64"] = lambda: enc.band_pick_segments(curve, n_cf // 64, 0, targets)
    stream_pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    size = dict(kbps_per_channel=96, max_kbps_per_channel=128, chunk_hops=a.chunk_hops)
    peak = dict(segment_hops=8, peak_kbps_per_channel=128)
    walls = {
        "encode_stream_abr_chunked": lambda: A.pacfile.encode_stream_abr_chunked(stream_pcm, 48000, **size),
        "encode_stream_abr_chunked_peak": lambda: A.pacfile.encode_stream_abr_chunked(stream_pcm, 48000, **size, **peak),
    }
    assert walls["encode_stream_abr_chunked_peak"]() == \
        A.pacfile.encode_stream_abr(stream_pcm, 48000, allocation="band", kbps_per_channel=96, max_kbps_per_channel=128,
                                    **peak)
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, cap 128 kb/s; "
                    f"G = {G}; band_profile_segments at {counts} segments beside band_profile; profile_solve_segments + "
                    f"profile_clamp_add on {counts[1:]} rows of their own, targets spread over the grid, nothing read "
                    "back; band_pick_segments (64 segments) beside "
                    f"band_pick; encode_stream_abr_chunked (chunks of {a.chunk_hops} blocks, 96 kb/s) with and without "
                    "segment_hops=8, peak_kbps_per_channel=128, host PCM to host bytes by the wall clock",
        "yardsticks": "band_profile, band_pick and encode_stream_abr_chunked without segments, this build, the same "
                      "process, alternating rounds",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds, "chunk_hops": a.chunk_hops,
        "device": torch.cuda.get_device_name(enc.device),
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
    res["solve_targets"] = {}
    for n in solve_rows:                                    # what the timed solves decided, and that their rows stood still
        assert int(solve_rows[n].sum().item()) == sums[n]
        dec = enc.decode_results(outs[n][0])
        t = dec["target_nmr_db"]
        res["solve_targets"][str(n)] = {"met_share": float(dec["met"].mean()), "lowest_db": float(t.min()),
                                        "median_db": float(np.median(t)), "highest_db": float(t.max()),
                                        "distinct": int(len(np.unique(t))),
                                        "rows_bytes": solve_rows[n].numel() * 8}
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    med.update({k + "_wall": float(np.median(res[k + "_wall_ms"])) for k in walls})
    res["median_ms"] = med
    res["spread_ms"] = {k: max(res[k + "_ms"]) - min(res[k + "_ms"]) for k in calls}
    res["spread_ms"].update({k + "_wall": max(res[k + "_wall_ms"]) - min(res[k + "_wall_ms"]) for k in walls})
    for n in counts:
        res[f"band_profile_segments_{n}_over_band_profile"] = med[f"band_profile_segments_{n}"] / med["band_profile"]
    res["band_pick_segments_over_band_pick"] = med["band_pick_segments_64"] / med["band_pick"]
    res["chunked_peak_over_chunked_wall"] = med["encode_stream_abr_chunked_peak_wall"] / med["encode_stream_abr_chunked_wall"]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
