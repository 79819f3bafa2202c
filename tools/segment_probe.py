"""Cost and yield of one noise-to-mask target per stretch of a stream (pacx_rate_solve_segments,
pacx_band_solve_segments, the segment_hops keyword of pacfile.encode_stream_abr).

1. Cost, on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks,
   curves with the cap 128 kb/s): Encoder.band_solve_segments and rate_solve_segments with n_seg = 1, 64 and 8192
   equal segments, every segment's limit the 96 kb/s share of its frames, against band_solve and rate_solve of the
   same build in the same process.  The calls are timed in alternation, `rounds` times, with device events around a
   window of at least `min-seconds` of calls after `warmup`, as tools/band_probe.py does, and every round is kept.
   Every solve reads its result back, so the times hold one device-to-host copy and the wait for it; the segmented
   ones also hold the upload of the boundaries and limits.
2. Yield, on the four golden excerpts, block switching on, cap 320 kb/s, allocation "band", at 96 and 128 kb/s with
   segment_hops = 8 and 32: the segments' targets (min / median / max), the fill of every segment's limit, and size
   and worst-band NMR against the whole-stream solve at the same nominal rate.
3. --ab LIB: band_solve, rate_solve, band_pick and encode_pack_nmr -- the calls whose kernels now share their
   per-frame work with the segmented ones -- with this tree's library and with another build (the parent commit's),
   in alternating processes, `rounds` rounds of one window each; PACX_LIB names the library a child loads, and one
   that lacks the new entry points is loaded without them.  The loader takes a PACX_LIB library only with a `.hash`
   file beside it that holds this tree's build.library_hash(): write one for the other build.  Written to --ab-out.

    python tools/segment_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out FILE]
                                  [--ab LIB --ab-out FILE] [--no-excerpts] [--no-cost]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from band_probe import EXCERPTS, timed, workload          # noqa: E402

NEW = ("pacx_rate_solve_segments", "pacx_band_solve_segments")
AB_CALLS = ("band_solve", "rate_solve", "band_pick", "encode_pack_nmr")


def old_calls(enc, view):
    """the four calls of the A/B on the bench workload -> dict name: callable"""
    vbr = enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0)
    r128 = enc.rate_curve(view, None, 128 / 48.0)
    b128 = enc.band_curve(view, None, 128 / 48.0)
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    return {"band_solve": lambda: enc.band_solve(b128, limit),
            "rate_solve": lambda: enc.rate_solve(r128, None, limit),
            "band_pick": lambda: enc.band_pick(b128, -3.0),
            "encode_pack_nmr": lambda: enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0, vbr)}, r128, b128


def ab_child(a):
    """one window of each of the four calls -> one JSON line"""
    import ctypes
    import torch
    import audio_codec_amd as A
    probe = ctypes.CDLL(A._lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            A._lib.SIGNATURES.pop(name, None)
    pcm, enc, view = workload(A, torch, a.frames)
    calls, _, _ = old_calls(enc, view)
    print(json.dumps({"library": A._lib.LIB_PATH,
                      "ms": {k: timed(torch, fn, a.min_seconds, a.warmup)[0] for k, fn in calls.items()}}))


def ab(a):
    rows = {w: {k: [] for k in AB_CALLS} for w in ("parent", "this")}
    for _ in range(a.rounds):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("PACX_LIB", None)
            if which == "parent":
                env["PACX_LIB"] = os.path.abspath(a.ab)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--frames", str(a.frames),
                                  "--min-seconds", str(a.min_seconds), "--warmup", str(a.warmup)],
                                 env=env, capture_output=True, text=True, timeout=300, check=True).stdout
            for k, v in json.loads(out.strip().split("\n")[-1])["ms"].items():
                rows[which][k].append(v)
    res = {"method": f"alternating processes, {a.rounds} rounds, one window of {a.min_seconds:g} s per call and round; "
                     f"{2 * a.frames} channel-frames of the bench workload",
           "parent_library": a.ab, "calls": {}}
    for k in AB_CALLS:
        p, t = rows["parent"][k], rows["this"][k]
        mp, mt = float(np.median(p)), float(np.median(t))
        spread = (max(p) - min(p)) / mp
        res["calls"][k] = {"parent_ms": p, "this_ms": t, "parent_ms_median": mp, "this_ms_median": mt,
                           "this_over_parent": mt / mp, "parent_spread": spread,
                           "within_parent_spread": bool(mt <= max(p))}
    return res


def cost(a, A, torch):
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf = view.n_cf
    calls, r128, b128 = old_calls(enc, view)
    calls = {k: calls[k] for k in ("band_solve", "rate_solve")}
    per_cf = 96 * 1000 * 1024 / 48000 / 8                       # bytes of one channel-frame at 96 kb/s
    results = {}
    for n_seg in (1, 64, n_cf):
        first = np.linspace(0, n_cf, n_seg + 1).astype(np.int64)
        limits = np.floor(np.diff(first) * per_cf).astype(np.int64)
        calls[f"band_solve_segments_{n_seg}"] = lambda f=first, l=limits: enc.band_solve_segments(b128, f, l)
        calls[f"rate_solve_segments_{n_seg}"] = lambda f=first, l=limits: enc.rate_solve_segments(r128, f, l)
        sol = enc.band_solve_segments(b128, first, limits)
        results[f"band_{n_seg}"] = {"met_share": float(sol["met"].mean()),
                                    "target_nmr_db_min_median_max": [float(np.min(sol["target_nmr_db"])),
                                                                     float(np.median(sol["target_nmr_db"])),
                                                                     float(np.max(sol["target_nmr_db"]))]}
    res = {"workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, curves with "
                       "the cap 128 kb/s; equal segments, every limit the 96 kb/s share of its frames; every solve reads "
                       "its result back",
           "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(enc.device), "on_workload": results, "calls_per_window": {}}
    for k in calls:
        res[k + "_ms"] = []
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(torch, fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    res["median_ms"] = med
    for kind in ("band", "rate"):
        for n_seg in (1, 64, n_cf):
            res[f"{kind}_solve_segments_{n_seg}_over_{kind}_solve"] = med[f"{kind}_solve_segments_{n_seg}"] / med[f"{kind}_solve"]
    return res


def yields(A):
    out = {}
    for name in EXCERPTS:
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        rows = {}
        for kbps in (96, 128):
            kw = dict(kbps_per_channel=kbps, block_switching=True, allocation="band")
            data, rep, info = A.quality.encode_stream_to_rate(x, sr, **kw)
            row = {"whole_stream": {"target_nmr_db": info["target_nmr_db"], "bytes": len(data),
                                    "fill": info["total_bytes"] / info["limit_bytes"], "worst_nmr_db": rep.maximum()}}
            for hops in (8, 32):
                try:
                    data, rep, info = A.quality.encode_stream_to_rate(x, sr, segment_hops=hops, **kw)
                except ValueError as e:
                    row[f"segment_hops_{hops}"] = {"unreachable": str(e)}
                    continue
                seg = info["segments"]
                fill = seg["total_bytes"] / np.maximum(seg["limit_bytes"], 1)
                t = seg["target_nmr_db"]
                row[f"segment_hops_{hops}"] = {
                    "segments": len(t), "target_nmr_db_min_median_max": [float(t.min()), float(np.median(t)), float(t.max())],
                    "fill_min_median_max": [float(fill.min()), float(np.median(fill)), float(fill.max())],
                    "bytes": len(data), "bytes_over_whole_stream": len(data) / row["whole_stream"]["bytes"],
                    "worst_nmr_db": rep.maximum()}
            rows[f"{kbps} kb/s"] = row
        out[name] = {"hops": len(x) // 1024, "sample_rate": sr, **rows}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab", default=None, help="another build of libpacx.so (the parent commit's) to time the old calls against")
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--no-excerpts", action="store_true")
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a)
    if a.ab:
        line = json.dumps(ab(a), indent=1)
        print(line)
        if a.ab_out:
            with open(a.ab_out, "w") as f:
                f.write(line + "\n")
    import torch
    import audio_codec_amd as A
    res = {} if a.no_cost else cost(a, A, torch)
    if not a.no_excerpts:
        res["excerpts"] = yields(A)
    if not res:
        return
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
