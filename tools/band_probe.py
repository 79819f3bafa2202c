"""Cost and yield of handing the bits to the bands one by one (pacx_band_curve_batch, pacx_band_pick, pacx_band_solve,
pacx_encode_pack_alloc_batch, the allocation="band" keyword of pacfile).

1. Times on the bench workload (8192 channel-frames of synthetic stereo at 48 kHz, scalar mantissas, all long blocks):
   Encoder.band_curve with the caps 128 and 320 kb/s, band_pick (-3 dB) and band_solve (limit: 96 kb/s) on the 128 kb/s
   curve, encode_pack_alloc with that pick's allocation, and pacfile.encode_stream_abr(allocation="band") as a whole
   (host PCM to host bytes, wall clock, cap 128 kb/s, 96 kb/s wanted).  Yardsticks in the same process, none of whose
   kernels this feature changes: encode_pack_nmr (-3 dB, cap 128 kb/s), rate_curve (cap 128 kb/s), rate_solve and
   encode_pack.  The calls are timed in alternation, `rounds` times, with device events around a window of at least
   `min-seconds` of calls after `warmup`, as tools/abr_probe.py does, and every round is kept.  The solves read their
   result back, so their times hold one device-to-host copy and the wait for it.
2. On the four golden excerpts, block switching on, cap 320 kb/s: kb/s per channel at 0 / -3 / -6 dB with both
   allocations, and the targets the two average-rate solves find at 96 and 128 kb/s.
3. --ab-child (used by --ab): encode_pack_nmr alone, with the library PACX_LIB names, for an A/B of that call between
   this tree and another build of the library (the parent commit's, say) in alternating processes.  A library that
   lacks the new entry points is loaded without them.

    python tools/band_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 5] [--rounds 5] [--ab LIB] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXCERPTS = ["castanet", "harpsichord", "quar48_1", "spmg"]
NEW = ("pacx_band_curve_batch", "pacx_band_pick", "pacx_band_solve", "pacx_encode_pack_alloc_batch")


def region(torch, fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps                       # ms per call


def timed(torch, fn, min_seconds, warmup):
    """-> (ms per call, calls in the window): the window holds as many calls as fill min_seconds, judged from a pilot
    of `warmup` calls after `warmup` untimed ones"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    steps = max(warmup, int(np.ceil(min_seconds * 1e3 / region(torch, fn, warmup))))
    return region(torch, fn, steps), steps


def wall(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def workload(A, torch, frames):
    pcm = A.synth.stream(frames, 2)
    enc = A.context.encoder(48000, 128 / 48.0)
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    return pcm, enc, A.engine.PcmView.stream(planar)


def ab_child(a):
    """encode_pack_nmr alone -> one JSON line {ms: [...]}"""
    import ctypes
    import torch
    import audio_codec_amd as A
    probe = ctypes.CDLL(A._lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            A._lib.SIGNATURES.pop(name, None)
    pcm, enc, view = workload(A, torch, a.frames)
    vbr = enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0)
    fn = lambda: enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0, vbr)        # noqa: E731
    ms = [timed(torch, fn, a.min_seconds, a.warmup)[0] for _ in range(a.rounds)]
    print(json.dumps({"library": A._lib.LIB_PATH, "ms": ms}))


def ab(a):
    """alternating processes: this tree's library, the other one, `rounds` times each"""
    rows = {"this": [], "other": []}
    for _ in range(a.rounds):
        for which in ("this", "other"):
            env = dict(os.environ)
            env.pop("PACX_LIB", None)
            if which == "other":
                env["PACX_LIB"] = os.path.abspath(a.ab)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--frames", str(a.frames),
                                  "--min-seconds", str(a.min_seconds), "--warmup", str(a.warmup), "--rounds", "2"],
                                 env=env, capture_output=True, text=True, timeout=300, check=True).stdout
            rows[which] += json.loads(out.strip().split("\n")[-1])["ms"]
    this, other = float(np.median(rows["this"])), float(np.median(rows["other"]))
    return {"call": "encode_pack_nmr (-3 dB, cap 128 kb/s)", "other_library": a.ab, "this_ms": rows["this"],
            "other_ms": rows["other"], "this_ms_median": this, "other_ms_median": other, "this_over_other": this / other,
            "this_spread_ms": max(rows["this"]) - min(rows["this"]), "other_spread_ms": max(rows["other"]) - min(rows["other"]),
            "method": "alternating processes, two one-second windows each"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab", default=None, help="another build of libpacx.so to time encode_pack_nmr against")
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--no-excerpts", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a)
    import torch
    import audio_codec_amd as A
    pcm, enc, view = workload(A, torch, a.frames)
    n_cf = view.n_cf
    vbr = enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0)
    cbr = enc.encode_pack(view, None)
    r128 = enc.rate_curve(view, None, 128 / 48.0)
    b128 = enc.band_curve(view, None, 128 / 48.0)
    b320 = enc.band_curve(view, None, 320 / 48.0)
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    pick = enc.band_pick(b128, -3.0)
    sol = enc.band_solve(b128, limit)
    rsol = enc.rate_solve(r128, None, limit)
    second = enc.encode_pack_alloc(view, None, pick["bit_alloc"])
    assert torch.equal(second["n_bytes"], pick["n_bytes"])
    stream_pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    calls = {
        "band_curve_128": lambda: enc.band_curve(view, None, 128 / 48.0, b128),
        "band_curve_320": lambda: enc.band_curve(view, None, 320 / 48.0, b320),
        "band_pick": lambda: enc.band_pick(b128, -3.0),
        "band_solve": lambda: enc.band_solve(b128, limit),
        "encode_pack_alloc": lambda: enc.encode_pack_alloc(view, None, pick["bit_alloc"], second),
        "encode_pack_nmr": lambda: enc.encode_pack_nmr(view, None, -3.0, 128 / 48.0, vbr),
        "rate_curve_128": lambda: enc.rate_curve(view, None, 128 / 48.0, r128),
        "rate_solve": lambda: enc.rate_solve(r128, None, limit),
        "encode_pack": lambda: enc.encode_pack(view, None, cbr),
    }
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks; band_curve with "
                    "caps 128 and 320 kb/s, band_pick at -3 dB and band_solve for 96 kb/s on the 128 kb/s curve, "
                    "encode_pack_alloc with that pick, encode_stream_abr(allocation='band') (cap 128 kb/s, 96 kb/s) from "
                    "host PCM to host bytes by the wall clock",
        "yardsticks": "encode_pack_nmr (-3 dB, cap 128 kb/s), rate_curve (cap 128 kb/s), rate_solve, encode_pack of this "
                      "build in the same process, alternating rounds",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
        "device": torch.cuda.get_device_name(enc.device),
        "on_workload": {
            "pick_bytes_over_search_bytes": float(pick["n_bytes"].sum().item()) / float(vbr["n_bytes"].sum().item()),
            "pick_capped_share": float(pick["capped"].float().mean().item()),
            "band_solve": {"target_nmr_db": sol["target_nmr_db"], "met": sol["met"], "fill": sol["total_bytes"] / limit},
            "rate_solve": {"target_nmr_db": rsol["target_nmr_db"], "met": rsol["met"], "fill": rsol["total_bytes"] / limit}},
        "calls_per_window": {}, "encode_stream_abr_band_wall_ms": [],
    }
    for k in calls:
        res[k + "_ms"] = []
    abr = lambda: A.pacfile.encode_stream_abr(stream_pcm, 48000, kbps_per_channel=96, max_kbps_per_channel=128,  # noqa: E731
                                              allocation="band")
    abr()
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(torch, fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
        res["encode_stream_abr_band_wall_ms"].append(wall(torch, abr, 3))
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    res["median_ms"] = med
    res["band_curve_128_over_rate_curve_128"] = med["band_curve_128"] / med["rate_curve_128"]
    res["band_curve_128_over_encode_pack_nmr"] = med["band_curve_128"] / med["encode_pack_nmr"]
    res["band_curve_320_over_encode_pack_nmr"] = med["band_curve_320"] / med["encode_pack_nmr"]
    res["band_solve_over_rate_solve"] = med["band_solve"] / med["rate_solve"]
    res["encode_pack_alloc_over_encode_pack"] = med["encode_pack_alloc"] / med["encode_pack"]
    res["encode_stream_abr_band_wall_ms_median"] = float(np.median(res["encode_stream_abr_band_wall_ms"]))
    if a.ab:
        res["encode_pack_nmr_against_other_library"] = ab(a)

    res["excerpts"] = {}
    for name in ([] if a.no_excerpts else EXCERPTS):
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        rows = {"kbps_per_channel": {}, "abr_target_nmr_db": {}}
        for target in (0.0, -3.0, -6.0):
            row = {}
            for alloc in ("budget", "band"):
                data, rep, info = A.quality.encode_stream_to_nmr(x, sr, target, block_switching=True, allocation=alloc)
                row[alloc] = {"kbps_per_channel": info["kbps_per_channel"], "worst_nmr_db": rep.maximum(),
                              "capped_channel_blocks_share": float(info["capped"][info["written"]].mean())}
            row["band_over_budget"] = row["band"]["kbps_per_channel"] / row["budget"]["kbps_per_channel"]
            rows["kbps_per_channel"][f"{target:+.0f} dB"] = row
        for alloc in ("budget", "band"):
            both = A.quality.encode_stream_to_rate(x, sr, kbps_per_channel=[96, 128], block_switching=True, allocation=alloc)
            for kbps, (data, rep, info) in zip((96, 128), both):
                rows["abr_target_nmr_db"].setdefault(f"{kbps} kb/s", {})[alloc] = {
                    "target_nmr_db": info["target_nmr_db"], "fill": info["total_bytes"] / info["limit_bytes"],
                    "share_audible": rep.share_audible(), "worst_nmr_db": rep.maximum()}
        res["excerpts"][name] = {"hops": len(x) // 1024, "sample_rate": sr, **rows}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
