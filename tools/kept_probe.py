"""Cost of keeping the curves of a chunked average-bit-rate encode as thresholds (pacx_band_thresholds,
pacx_rate_thresholds, the picks on them, pacfile.encode_stream_abr_kept).

The procedure of tools/profile_probe.py.  On the bench workload (8192 channel-frames of synthetic stereo at 48 kHz,
scalar mantissas, all long blocks), 96 kb/s wanted:
  Encoder.band_thresholds at G = 3841 (+-30 dB) beside Encoder.band_curve and Encoder.band_profile (what a chunk's first
  pass pays anyway); Encoder.band_pick_thresholds beside Encoder.band_pick at the target found;
  Encoder.rate_thresholds and rate_pick_thresholds beside Encoder.rate_curve and rate_pick, at caps of 128 and 320 kb/s;
  by the wall clock, host PCM to host bytes, pacfile.encode_stream_abr_kept beside pacfile.encode_stream_abr_chunked: the
  same bytes, for scalar band (chunks of `chunk-hops` blocks), budget at both caps, and the vq128 workload (gain-shape
  coder without SBR at 128 kb/s) on `vq-frames` frames so that a round stays within the window.
The calls are timed in alternation, `rounds` times, with device events around a window of at least `min-seconds` of
calls after `warmup`; every round is kept.

--ab ROOT: the yardstick for the unchanged call.  ROOT is a checkout of the parent commit, built from source; its
encode_stream_abr_chunked and this tree's are timed in alternating processes, `rounds` times each, on the same four
configurations.  This tree's must lie within the parent's own rounds; the kept call is worth its memory where its median
lies below the parent's fastest round.

    python tools/kept_probe.py [--frames 4096] [--vq-frames 256] [--chunk-hops 512] [--min-seconds 1.0] [--warmup 5]
                               [--rounds 5] [--ab ROOT] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("band", "budget_128", "budget_320", "vq128")


def stream_calls(A, a, kept):
    """{configuration: a call from host PCM to host bytes}; kept: encode_stream_abr_kept, else encode_stream_abr_chunked"""
    pcm = A.synth.stream(a.frames, 2)
    pcm = np.ascontiguousarray(pcm[:len(pcm) // 1024 * 1024])
    vq_pcm = np.ascontiguousarray(pcm[:a.vq_frames * 1024])
    fn = A.pacfile.encode_stream_abr_kept if kept else A.pacfile.encode_stream_abr_chunked
    size = dict(kbps_per_channel=96, chunk_hops=a.chunk_hops)
    return {
        "band": lambda: fn(pcm, 48000, max_kbps_per_channel=128, **size),
        "budget_128": lambda: fn(pcm, 48000, max_kbps_per_channel=128, allocation="budget", **size),
        "budget_320": lambda: fn(pcm, 48000, max_kbps_per_channel=320, allocation="budget", **size),
        "vq128": lambda: fn(vq_pcm, 48000, max_kbps_per_channel=128, use_vq=True, **size),
    }


def wall_once(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab_child(a):
    """encode_stream_abr_chunked of the tree at a.root alone -> one JSON line {configuration: [ms, ...]}"""
    sys.path.insert(0, a.root)
    import torch
    import audio_codec_amd as A
    assert os.path.realpath(A._lib.LIB_PATH).startswith(os.path.realpath(a.root) + os.sep), A._lib.LIB_PATH
    calls = stream_calls(A, a, False)
    out = {}
    for name, fn in calls.items():
        fn()                                                # buffers, handles
        out[name] = [wall_once(torch, fn) for _ in range(2)]
    print(json.dumps({"root": a.root, "ms": out}))


def ab(a):
    rows = {"this": {c: [] for c in CONFIGS}, "parent": {c: [] for c in CONFIGS}}
    for r in range(a.rounds):
        for which, root in (("this", ROOT), ("parent", os.path.abspath(a.ab))):
            print(f"process pair {r + 1} of {a.rounds}: {which}", file=sys.stderr, flush=True)
            env = dict(os.environ)
            env.pop("PACX_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--root", root, "--frames",
                                  str(a.frames), "--vq-frames", str(a.vq_frames), "--chunk-hops", str(a.chunk_hops)],
                                 env=env, capture_output=True, text=True, timeout=600, check=True).stdout
            for c, ms in json.loads(out.strip().split("\n")[-1])["ms"].items():
                rows[which][c] += ms
    res = {"method": "alternating processes, two calls each after one untimed, host PCM to host bytes by the wall clock",
           "call": "encode_stream_abr_chunked"}
    for c in CONFIGS:
        this, parent = rows["this"][c], rows["parent"][c]
        res[c] = {"this_ms": this, "parent_ms": parent, "this_ms_median": float(np.median(this)),
                  "parent_ms_median": float(np.median(parent)), "parent_ms_min": min(parent), "parent_ms_max": max(parent),
                  "this_within_parents_rounds": min(parent) <= float(np.median(this)) <= max(parent)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--vq-frames", type=int, default=256)
    ap.add_argument("--chunk-hops", type=int, default=512)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="length of every timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_probe.json"))
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import audio_codec_amd as A
    from band_probe import timed, workload
    pcm, enc, view = workload(A, torch, a.frames)
    limit = int(96 * 1000 * 2 * view.n_frames * 1024 / 48000 / 8)
    calls, checks = {}, {}

    curve = enc.band_curve(view, None, 128 / 48.0)
    profile = enc.band_profile(curve)
    target = enc.profile_solve(profile, limit)["target_nmr_db"]
    kept = enc.band_thresholds(curve)
    a_pick, b_pick = enc.band_pick(curve, target), enc.band_pick_thresholds(kept, target)
    assert all(bool((a_pick[k] == b_pick[k]).all()) for k in a_pick)
    calls.update({
        "band_curve": lambda: enc.band_curve(view, None, 128 / 48.0, curve),
        "band_profile": lambda: enc.band_profile(curve, out=profile),
        "band_thresholds": lambda: enc.band_thresholds(curve, out=kept),
        "band_pick": lambda: enc.band_pick(curve, target),
        "band_pick_thresholds": lambda: enc.band_pick_thresholds(kept, target),
    })
    checks["band_target_nmr_db"] = target
    for cap_kbps in (128, 320):
        cap = cap_kbps / 48.0
        rc = enc.rate_curve(view, None, cap)
        rt = enc.profile_solve(enc.rate_profile(rc), limit)["target_nmr_db"]
        rk = enc.rate_thresholds(rc)
        a_pick, b_pick = enc.rate_pick(rc, rt), enc.rate_pick_thresholds(rk, rt)
        assert all(bool((a_pick[k] == b_pick[k]).all()) for k in a_pick)
        calls.update({
            f"rate_curve_{cap_kbps}": lambda rc=rc, cap=cap: enc.rate_curve(view, None, cap, rc),
            f"rate_thresholds_{cap_kbps}": lambda rc=rc, rk=rk: enc.rate_thresholds(rc, out=rk),
            f"rate_pick_{cap_kbps}": lambda rc=rc, rt=rt: enc.rate_pick(rc, rt),
            f"rate_pick_thresholds_{cap_kbps}": lambda rk=rk, rt=rt: enc.rate_pick_thresholds(rk, rt),
        })
        checks[f"rate_target_nmr_db_{cap_kbps}"] = rt
    chunked, keeping = stream_calls(A, a, False), stream_calls(A, a, True)
    for c in CONFIGS:
        assert keeping[c]() == chunked[c](), c
    res = {
        "workload": f"{view.n_cf} channel-frames, synthetic stereo at 48 kHz, scalar mantissas, all long blocks, 96 kb/s "
                    "wanted, G = 3841; band calls at a cap of 128 kb/s, rate calls at caps of 128 and 320 kb/s; streams "
                    f"from host PCM to host bytes by the wall clock in chunks of {a.chunk_hops} blocks, the vq128 stream "
                    f"(gain-shape coder without SBR, cap 128 kb/s) on {a.vq_frames} blocks; the kept call writes the "
                    "chunked call's bytes",
        "yardsticks": "the curve, profile and pick calls and encode_stream_abr_chunked of this build in the same process, "
                      "alternating rounds; with --ab, encode_stream_abr_chunked of the parent commit in alternating processes",
        "min_seconds": a.min_seconds, "warmup": a.warmup, "rounds": a.rounds, "chunk_hops": a.chunk_hops,
        "device": torch.cuda.get_device_name(enc.device), "checks": checks, "calls_per_window": {},
        "kept_bytes_per_cf": {"band": A.pacfile._BandPath(enc).kept_bytes_per_cf(128 / 48.0),
                              "budget_128": A.pacfile._BudgetPath(enc).kept_bytes_per_cf(128 / 48.0),
                              "budget_320": A.pacfile._BudgetPath(enc).kept_bytes_per_cf(320 / 48.0)},
    }
    ms = {k: [] for k in calls}
    walls = {f"{kind}_{c}": [] for c in CONFIGS for kind in ("chunked", "kept")}
    for r in range(a.rounds):
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
        for name, fn in calls.items():
            t, steps = timed(torch, fn, a.min_seconds, a.warmup)
            ms[name].append(t)
            res["calls_per_window"][name] = steps
        for c in CONFIGS:
            walls[f"chunked_{c}"].append(wall_once(torch, chunked[c]))
            walls[f"kept_{c}"].append(wall_once(torch, keeping[c]))
    res["ms"], res["wall_ms"] = ms, walls
    res["median_ms"] = {k: float(np.median(v)) for k, v in {**ms, **walls}.items()}
    res["spread_ms"] = {k: max(v) - min(v) for k, v in {**ms, **walls}.items()}
    res["kept_over_chunked_wall"] = {c: res["median_ms"][f"kept_{c}"] / res["median_ms"][f"chunked_{c}"] for c in CONFIGS}
    if a.ab:
        res["ab"] = ab(a)
        for c in CONFIGS:
            res["ab"][c]["kept_ms_median"] = res["median_ms"][f"kept_{c}"]
            res["ab"][c]["kept_below_parents_fastest_round"] = res["median_ms"][f"kept_{c}"] < res["ab"][c]["parent_ms_min"]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
