"""Cost of the NMR report on the bench workload (8192 channel-frames of synthetic stereo, scalar mantissas at
128 kb/s): pacx_nmr_batch alone, pacx_nmr_summary alone, and quality.encode_stream_report against
pacfile.encode_stream on the same stream.  Device events around `steps` calls after `warmup`; the stream-level
pair is host to host (it ends in device-to-host copies), so a host clock around it.

    python tools/nmr_probe.py [--frames 4096] [--steps 20] [--warmup 5] [--out profiles/nmr_probe.json]

Bytes per channel-frame are counted from shapes: k_nmr reads 3 x 8 KB (original lines, decoded lines, threshold)
+ 32 B of overall scales and writes 3 x band_stride doubles; the front end in front of it is the encoder's own
(MDCT, side chain, mask) with the 8 KB threshold written on top.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_codec_amd as A  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps                       # ms per call


def host_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pcm = A.synth.stream(a.frames, 2)
    enc = A.context.encoder(48000, 128 / 48.0)
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    view = A.engine.PcmView.stream(planar)
    n_cf = view.n_cf
    out = enc.encode_pack(view)
    codes = enc.unpack(out["payload"], out["n_bytes"])
    extra = {}
    enc.decode(codes, 2, want_pcm=False, extra=extra)
    lines, overall = extra["lines"], codes["overall"]
    r = enc.nmr(view, None, lines, overall)
    words = enc.nmr_summary(r["nmr_db"], 2)
    res = {
        "workload": f"{n_cf} channel-frames, synthetic stereo, scalar mantissas, 128 kb/s, all long blocks",
        "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(enc.device),
        "band_stride": enc.band_stride,
        "k_nmr_bytes_per_cf": {"read": 3 * 8192 + 32, "written": 3 * 8 * enc.band_stride},
        "front_end_extra_bytes_per_cf": {"threshold_written": 8192},
    }
    res["encode_pack_ms"] = timed(lambda: enc.encode_pack(view, None, out), a.steps, a.warmup)
    res["nmr_batch_ms"] = timed(lambda: enc.nmr(view, None, lines, overall), a.steps, a.warmup)
    res["nmr_summary_ms"] = timed(lambda: enc.nmr_summary(r["nmr_db"], 2, None, words), a.steps, a.warmup)
    res["nmr_batch_M_cf_per_s"] = n_cf / res["nmr_batch_ms"] / 1e3
    res["encode_stream_ms"] = host_timed(lambda: A.pacfile.encode_stream(pcm, 48000, 128), a.steps, a.warmup)
    res["encode_stream_report_ms"] = host_timed(lambda: A.quality.encode_stream_report(pcm, 48000, 128), a.steps, a.warmup)
    res["encode_stream_report_chunk_hops"] = 4096
    assert A.quality.encode_stream_report(pcm, 48000, 128)[0] == A.pacfile.encode_stream(pcm, 48000, 128)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
