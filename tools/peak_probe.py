"""Cost and yield of an average for the stream with a peak per segment (pacx_rate_solve_peak, pacx_band_solve_peak, the
peak_kbps_per_channel keyword of pacfile.encode_stream_abr).

1. Cost of the new level, on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all
   long blocks, curves with the cap 128 kb/s): Encoder.band_solve_peak and rate_solve_peak with n_seg = 1, 64 and 8192
   equal segments -- every peak the 128 kb/s share of the segment's frames, the stream's limit the 96 kb/s size --
   against band_solve_segments and rate_solve_segments at the same partitions with the 96 kb/s shares, in the same
   process.  Timed in alternation, `rounds` times, with device events around a window of at least `min-seconds` of
   calls after `warmup` (tools/band_probe.py's timed), every round kept.  Every solve reads its results back.
2. Yield, on the four golden excerpts, block switching on, cap 320 kb/s, allocation "band", a 96 kb/s average with
   segment_hops = 8 and 32: the whole-stream solve, the segmented solve at 96 kb/s, and the peak solve with a peak of
   128 kb/s -- file size, worst band NMR and share of bands above the mask (quality's Report), pinned segments.
3. --ab LIB: rate_solve, band_solve, band_pick, both segmented solves at 64 segments and the control encode_pack_nmr
   with this tree's library and with another build (the parent commit's), in alternating processes, `rounds` rounds
   of one window each, as tools/segment_probe.py --ab (see there for PACX_LIB and the `.hash` file).  Written to
   --ab-out.

    python tools/peak_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--out FILE]
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
from segment_probe import old_calls                       # noqa: E402

NEW = ("pacx_rate_solve_peak", "pacx_band_solve_peak")
AB_CALLS = ("rate_solve", "band_solve", "band_pick", "rate_solve_segments_64", "band_solve_segments_64", "encode_pack_nmr")
PER_CF = 1000 * 1024 / 48000 / 8                          # bytes of one channel-frame of the workload at 1 kb/s


def equal_segments(n_cf, n_seg, kbps):
    first = np.linspace(0, n_cf, n_seg + 1).astype(np.int64)
    return first, np.floor(np.diff(first) * kbps * PER_CF).astype(np.int64)


def ab_child(a):
    """one window of each call of the A/B -> one JSON line"""
    import ctypes
    import torch
    import audio_codec_amd as A
    probe = ctypes.CDLL(A._lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            A._lib.SIGNATURES.pop(name, None)
    pcm, enc, view = workload(A, torch, a.frames)
    calls, r128, b128 = old_calls(enc, view)
    first, limits = equal_segments(view.n_cf, 64, 96)
    calls["rate_solve_segments_64"] = lambda: enc.rate_solve_segments(r128, first, limits)
    calls["band_solve_segments_64"] = lambda: enc.band_solve_segments(b128, first, limits)
    print(json.dumps({"library": A._lib.LIB_PATH,
                      "ms": {k: timed(torch, calls[k], a.min_seconds, a.warmup)[0] for k in AB_CALLS}}))


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
                     f"{2 * a.frames} channel-frames of the bench workload; the segmented solves at 64 equal segments",
           "parent_library": a.ab, "calls": {}}
    for k in AB_CALLS:
        p, t = rows["parent"][k], rows["this"][k]
        mp, mt = float(np.median(p)), float(np.median(t))
        res["calls"][k] = {"parent_ms": p, "this_ms": t, "parent_ms_median": mp, "this_ms_median": mt,
                           "this_over_parent": mt / mp, "parent_spread": (max(p) - min(p)) / mp,
                           "within_parent_rounds": bool(min(p) <= mt <= max(p)), "not_above_parent_rounds": bool(mt <= max(p))}
    return res


def cost(a, A, torch):
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf = view.n_cf
    r128 = enc.rate_curve(view, None, 128 / 48.0)
    b128 = enc.band_curve(view, None, 128 / 48.0)
    limit = int(96 * PER_CF * n_cf)
    calls, on = {}, {}
    for n_seg in (1, 64, n_cf):
        first, share = equal_segments(n_cf, n_seg, 96)
        _, peaks = equal_segments(n_cf, n_seg, 128)
        calls[f"band_solve_segments_{n_seg}"] = lambda f=first, l=share: enc.band_solve_segments(b128, f, l)
        calls[f"band_solve_peak_{n_seg}"] = lambda f=first, p=peaks: enc.band_solve_peak(b128, f, p, limit)
        calls[f"rate_solve_segments_{n_seg}"] = lambda f=first, l=share: enc.rate_solve_segments(r128, f, l)
        calls[f"rate_solve_peak_{n_seg}"] = lambda f=first, p=peaks: enc.rate_solve_peak(r128, f, p, limit)
        for kind, sol in (("band", enc.band_solve_peak(b128, first, peaks, limit)),
                          ("rate", enc.rate_solve_peak(r128, first, peaks, limit))):
            on[f"{kind}_{n_seg}"] = {"stream_target_nmr_db": sol["stream_target_nmr_db"], "stream_met": sol["stream_met"],
                                     "pinned_share": float(sol["pinned"].mean()), "met_share": float(sol["met"].mean())}
    t_lo, t_hi = -30 * 64, 30 * 64
    pairs = 2 + int(np.ceil(np.log2(t_hi - t_lo + 2)))
    res = {"workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, curves with "
                       "the cap 128 kb/s; equal segments; peaks the 128 kb/s share of a segment's frames and the stream's "
                       "limit the 96 kb/s size for the peak solves, limits the 96 kb/s shares for the segmented ones; "
                       "every solve reads its results back",
           "kernel_launches": {"segmented": 2 * pairs + 1, "peak": 4 * pairs + 1},
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
    for kind in ("band", "rate"):
        for n_seg in (1, 64, n_cf):
            res[f"{kind}_solve_peak_{n_seg}_over_segments"] = med[f"{kind}_solve_peak_{n_seg}"] / \
                med[f"{kind}_solve_segments_{n_seg}"]
    return res


def yields(A):
    out = {}
    for name in EXCERPTS:
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        kw = dict(kbps_per_channel=96, block_switching=True, allocation="band")

        def row(data, rep, info):
            return {"bytes": len(data), "fill": info["total_bytes"] / info["limit_bytes"],
                    "worst_nmr_db": rep.maximum(), "share_audible": rep.share_audible()}

        data, rep, info = A.quality.encode_stream_to_rate(x, sr, **kw)
        rows = {"whole_stream": dict(row(data, rep, info), target_nmr_db=info["target_nmr_db"])}
        for hops in (8, 32):
            for what, more in (("segmented", {}), ("peak_128", {"peak_kbps_per_channel": 128})):
                try:
                    data, rep, info = A.quality.encode_stream_to_rate(x, sr, segment_hops=hops, **more, **kw)
                except ValueError as e:
                    rows[f"{what}_hops_{hops}"] = {"refused": str(e)}
                    continue
                seg = info["segments"]
                t = seg["target_nmr_db"]
                r = dict(row(data, rep, info), segments=len(t),
                         bytes_over_whole_stream=len(data) / rows["whole_stream"]["bytes"],
                         target_nmr_db_min_median_max=[float(t.min()), float(np.median(t)), float(t.max())])
                if more:
                    fill = seg["total_bytes"] / np.maximum(seg["limit_bytes"], 1)
                    r.update(stream_target_nmr_db=info["stream_target_nmr_db"], pinned=int(seg["pinned"].sum()),
                             peak_fill_max=float(fill.max()))
                rows[f"{what}_hops_{hops}"] = r
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
