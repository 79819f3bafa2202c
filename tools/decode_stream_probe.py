"""Whole-stream decode, host bytes in to host int16 out: pacfile.decode_stream(data) (one batch, the length
prefixes walked on the host) against decode_stream(data, chunk_bytes=c) (chunks, record index built on the
device), alternating in one process, plus the device-event time of pacx_index_body and of the decode kernels
for one chunk on their own.

    python tools/decode_stream_probe.py [--hops 65536] [--reps 5] [--out profiles/decode_stream_probe.json]

Every step runs under a time limit of its own (SIGALRM): a step that hangs ends the process."""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_codec_amd as A  # noqa: E402

MIB = 1 << 20


class step:
    """with step("name", seconds): ... -- the time limit of one step"""

    def __init__(self, name, limit):
        self.name, self.limit = name, int(limit)

    def _expired(self, *_):
        raise TimeoutError(f"step '{self.name}' exceeded its {self.limit} s")

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.limit)
        print(f"[{self.name}]", flush=True)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_chunk_events(pac, chunk_bytes, reps):
    """pacx_index_body and the decode kernels (unpack + decode, before the overlap-and-add) of the first chunk, each
    alone on the device: median device-event milliseconds"""
    from audio_codec_amd.streaming import HostStreamDecoder
    cp, pos = A.pacfile.parse_header(pac)
    enc = A.context.encoder_for_params(cp)
    hs = HostStreamDecoder(enc, cp.nChannels, chunk_bytes, max(1, chunk_bytes // (128 * cp.nChannels)), timing=True)
    n = min(chunk_bytes, len(pac) - pos)
    hs.input(0)[:n] = np.frombuffer(pac, dtype=np.uint8, count=n, offset=pos)
    for _ in range(reps + 1):
        hs.submit_index(0, n, n == len(pac) - pos)
        n_rec, consumed, error_at = hs.index_result(0)
        torch.cuda.synchronize()
        hs.submit_decode(0, n_rec, False)
        torch.cuda.synchronize()
        hs.result(0)
    t = hs.timings()[1:]                                        # the first pass grows the handle's workspaces
    return {"chunk_bytes": n, "records": t[0][0], "index_ms_median": statistics.median(x[1] for x in t),
            "decode_kernels_ms_median": statistics.median(x[2] for x in t),
            "index_ms_all": [x[1] for x in t], "decode_kernels_ms_all": [x[2] for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks-mib", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_stream_probe.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True,
                                             stderr=subprocess.DEVNULL).strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    report = {"commit": commit, "device": torch.cuda.get_device_name(0), "hops": a.hops, "channels": 2, "sample_rate": 48000,
              "repetitions": a.reps,
              "what": "host bytes in to host int16 out; *_cf_per_s from a wall clock around a final device synchronise, "
                      "one_chunk.*_ms from device events with nothing else on the device",
              "inputs": {}}
    with step("synthesise", 120):
        pcm = A.synth.stream(a.hops, 2)
    n_cf = (a.hops + 2) * 2
    inputs = (("scalar128", dict(kbps_per_channel=128)),
              ("vq96_sbr_bs", dict(kbps_per_channel=96, use_vq=True, use_sbr=True, block_switching=True)))
    ok = True
    for name, kw in inputs:
        with step(f"encode {name}", 300):
            pac = A.pacfile.encode_stream(pcm, 48000, chunk_hops=8192, **kw)
        contenders = [("one_batch", None)] + [(f"chunks_{c}MiB", c * MIB) for c in a.chunks_mib]
        with step(f"warm up {name}", 300):
            want = A.pacfile.decode_stream(pac)
            for tag, c in contenders[1:]:
                assert np.array_equal(A.pacfile.decode_stream(pac, chunk_bytes=c), want), tag
        secs = {tag: [] for tag, _ in contenders}
        for r in range(a.reps):                                 # alternating, in one process
            for tag, c in contenders:
                with step(f"{name} {tag} #{r}", 120):
                    dt, _ = timed(lambda: A.pacfile.decode_stream(pac, chunk_bytes=c) if c else A.pacfile.decode_stream(pac))
                secs[tag].append(dt)
        res = {"pac_bytes": len(pac), "channel_frames": n_cf, "contenders": {}}
        for tag, _ in contenders:
            rate = [n_cf / s for s in secs[tag]]
            res["contenders"][tag] = {"seconds": secs[tag], "cf_per_s_median": statistics.median(rate),
                                      "cf_per_s_min": min(rate), "cf_per_s_max": max(rate)}
        best = max((t for t, _ in contenders[1:]), key=lambda t: res["contenders"][t]["cf_per_s_min"])
        res["best_chunked"] = best
        res["chunked_slowest_beats_one_batch_fastest"] = bool(
            res["contenders"][best]["cf_per_s_min"] > res["contenders"]["one_batch"]["cf_per_s_max"])
        with step(f"{name} one chunk, device events", 120):
            res["one_chunk"] = one_chunk_events(pac, dict(contenders)[best], a.reps)
        res["index_below_decode_kernels"] = bool(res["one_chunk"]["index_ms_median"] < res["one_chunk"]["decode_kernels_ms_median"])
        ok = ok and res["chunked_slowest_beats_one_batch_fastest"]
        report["inputs"][name] = res
        print(json.dumps(res["contenders"], indent=1), json.dumps(res["one_chunk"]), flush=True)
    report["accepted"] = bool(ok and report["inputs"]["scalar128"]["index_below_decode_kernels"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("accepted" if report["accepted"] else "NOT accepted", "->", a.out)


if __name__ == "__main__":
    main()
