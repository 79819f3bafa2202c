"""Cost and yield of coding gain-shape streams band by band (pacx_vq_band_curve_batch, pacx_encode_vq_alloc_batch,
pacfile.encode_stream_vq_nmr / encode_stream_vq_abr).

1. Times on the vq128 bench workload (8192 channel-frames of synthetic stereo at 48 kHz, gain-shape coder without SBR,
   128 kb/s per channel, all long blocks): Encoder.vq_band_curve with the cap 128 kb/s, encode_vq_alloc with the
   allocation the sibling's band_pick gives at -3 dB, and pacfile.encode_stream_vq_abr as a whole (host PCM to host
   bytes, wall clock, cap 128 kb/s, 96 kb/s wanted).  Yardsticks in the same process, none of whose kernels this
   feature changes: encode_vq and decode_vq (to lines).  The curve is maxMantBits - 1 = 15 passes through the
   gain-shape coder and its decoder, so a figure near 15 times one encode plus one decode is what to expect.  The calls
   are timed in alternation, `rounds` times, with device events around a window of at least `min-seconds` of calls
   after `warmup`, as tools/band_probe.py does, and every round is kept.
   Why it is more: `per_size` times one pass's coder (encode_vq_alloc with every band at that size) and decoder
   (decode_vq of its payload) for each of the 15 sizes, three calls each after one untimed.
2. On the four golden excerpts, block switching on, cap 320 kb/s: kb/s per channel, worst band and share of bands
   above the mask at 0 / -3 / -6 dB; the targets the average-rate solve finds at 96 and 128 kb/s with worst band and
   share above the mask, and beside them the constant-rate gain-shape encode (no SBR) at the same nominal rate.

    python tools/vq_band_probe.py [--frames 4096] [--min-seconds 1.0] [--warmup 3] [--rounds 5] [--out FILE]

Writes profiles/vq_band_probe.json unless --out names another file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXCERPTS = ["castanet", "harpsichord", "quar48_1", "spmg"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-excerpts", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_band_probe.json"))
    a = ap.parse_args()
    import torch
    import audio_codec_amd as A
    pcm = A.synth.stream(a.frames, 2)
    enc = A.context.encoder(48000, 128 / 48.0, use_vq=True)
    sib = A.context.scalar_sibling(enc)
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    view = A.engine.PcmView.stream(planar)
    n_cf, n_ch = view.n_cf, 2
    cbr = enc.encode_vq(view, None)
    curve = enc.vq_band_curve(view, None, 128 / 48.0)
    pick = sib.band_pick(curve, -3.0)
    second = enc.encode_vq_alloc(view, None, pick["bit_alloc"])
    assert torch.equal(second["n_bytes"], pick["n_bytes"])
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    sol = sib.band_solve(curve, limit)
    stream_pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    calls = {
        "vq_band_curve_128": lambda: enc.vq_band_curve(view, None, 128 / 48.0, curve),
        "encode_vq_alloc": lambda: enc.encode_vq_alloc(view, None, pick["bit_alloc"], second),
        "encode_vq": lambda: enc.encode_vq(view, None, cbr),
        "decode_vq_lines": lambda: enc.decode_vq(cbr["payload"], cbr["n_bytes"], n_ch, want_lines=True, want_pcm=False),
    }
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo at 48 kHz, gain-shape coder without SBR at 128 kb/s per "
                    "channel, all long blocks; vq_band_curve with the cap 128 kb/s, encode_vq_alloc with the sibling's "
                    "band_pick at -3 dB, encode_stream_vq_abr (cap 128 kb/s, 96 kb/s) from host PCM to host bytes by "
                    "the wall clock",
        "yardsticks": "encode_vq and decode_vq (to lines) of this build in the same process, alternating rounds",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds,
        "device": torch.cuda.get_device_name(enc.device),
        "on_workload": {
            "pick_bytes_over_constant_rate_bytes": float(pick["n_bytes"].sum().item()) / float(cbr["n_bytes"].sum().item()),
            "pick_capped_share": float(pick["capped"].float().mean().item()),
            "band_solve": {"target_nmr_db": sol["target_nmr_db"], "met": sol["met"], "fill": sol["total_bytes"] / limit}},
        "calls_per_window": {}, "encode_stream_vq_abr_wall_ms": [],
    }
    for k in calls:
        res[k + "_ms"] = []
    abr = lambda: A.pacfile.encode_stream_vq_abr(stream_pcm, 48000, kbps_per_channel=96, max_kbps_per_channel=128)  # noqa: E731
    abr()
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms, steps = timed(torch, fn, a.min_seconds, a.warmup)
            res[name + "_ms"].append(ms)
            res["calls_per_window"][name] = steps
        res["encode_stream_vq_abr_wall_ms"].append(wall(torch, abr, 2))
    med = {k: float(np.median(res[k + "_ms"])) for k in calls}
    res["median_ms"] = med
    res["spread_ms"] = {k: max(res[k + "_ms"]) - min(res[k + "_ms"]) for k in calls}
    res["vq_band_curve_128_over_encode_vq"] = med["vq_band_curve_128"] / med["encode_vq"]
    res["vq_band_curve_128_over_encode_plus_decode"] = med["vq_band_curve_128"] / (med["encode_vq"] + med["decode_vq_lines"])
    res["encode_vq_alloc_over_encode_vq"] = med["encode_vq_alloc"] / med["encode_vq"]
    res["encode_stream_vq_abr_wall_ms_median"] = float(np.median(res["encode_stream_vq_abr_wall_ms"]))

    res["per_size"] = {}
    for bits in range(2, 17):
        alloc = torch.full((n_cf, enc.band_stride), bits, dtype=torch.int32, device=enc.device)
        out = enc.encode_vq_alloc(view, None, alloc)
        dec = lambda: enc.decode_vq(out["payload"], out["n_bytes"], n_ch, want_lines=True, want_pcm=False)  # noqa: E731
        dec()
        torch.cuda.synchronize()
        res["per_size"][str(bits)] = {
            "encode_vq_alloc_ms": region(torch, lambda: enc.encode_vq_alloc(view, None, alloc, out), 3),
            "decode_vq_lines_ms": region(torch, dec, 3), "mean_record_bytes": float(out["n_bytes"].float().mean().item())}
    res["per_size_sum_ms"] = sum(v["encode_vq_alloc_ms"] + v["decode_vq_lines_ms"] for v in res["per_size"].values())

    res["excerpts"] = {}
    for name in ([] if a.no_excerpts else EXCERPTS):
        ex = np.load(os.path.join(ROOT, "tests", "golden", f"excerpt_{name}.npz"))
        x, sr = ex["pcm"], int(ex["sr"])
        x = np.ascontiguousarray(x[:len(x) // 1024 * 1024])
        rows = {"to_nmr": {}, "to_rate": {}}
        for target in (0.0, -3.0, -6.0):
            data, rep, info = A.quality.encode_stream_vq_to_nmr(x, sr, target, block_switching=True)
            rows["to_nmr"][f"{target:+.0f} dB"] = {
                "kbps_per_channel": info["kbps_per_channel"], "worst_nmr_db": rep.maximum(),
                "share_audible": rep.share_audible(),
                "capped_channel_blocks_share": float(info["capped"][info["written"]].mean())}
        both = A.quality.encode_stream_vq_to_rate(x, sr, kbps_per_channel=[96, 128], block_switching=True)
        for kbps, (data, rep, info) in zip((96, 128), both):
            _, flat = A.quality.encode_stream_report(x, sr, kbps, block_switching=True, use_vq=True)
            rows["to_rate"][f"{kbps} kb/s"] = {
                "target_nmr_db": info["target_nmr_db"], "fill": info["total_bytes"] / info["limit_bytes"],
                "share_audible": rep.share_audible(), "worst_nmr_db": rep.maximum(),
                "constant_rate_gain_shape": {"share_audible": flat.share_audible(), "worst_nmr_db": flat.maximum()}}
        res["excerpts"][name] = {"hops": len(x) // 1024, "sample_rate": sr, **rows}
    line = json.dumps(res, indent=1)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
