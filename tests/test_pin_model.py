"""CPU checks of per-block targets under a leaky bucket (include/pacx_bucket_pin.h): tests/pin_model.py's level through a
hop by the recursion against the maximum over all stretches, what the pinned solve holds by construction on monotone
curves, a curve that is not monotone, phases that run out, the exports and what the Python layer refuses before it
touches a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import abr_model as am
import band_model as bm
import bucket_model as kb
import pin_model as pn

Q = kb.Q
T_LO, T_HI = -30 * 64, 30 * 64
NAMES = ("pacx_bucket_through", "pacx_band_solve_bucket_pinned", "pacx_rate_solve_bucket_pinned")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


def drawn(rng):
    """hops of one to three channels against a drain of the same order or one beyond every level, a start level anywhere
    in the buffer; sometimes the largest entries, buffer and start level of the domain"""
    n_ch, n_hops = int(rng.integers(1, 4)), int(rng.integers(0, 14))
    n = n_hops * n_ch
    if rng.random() < 0.15:
        return np.full(n, 65535), n_ch, (int(rng.choice([0, 1, 65539 << Q, (1 << 63) - 1])), 1 << 40, 1 << 56)
    n_bytes = rng.integers(-3, 400, n) * (rng.random(n) < 0.7)
    drain = int(rng.integers(0, 500 << Q)) if rng.random() < 0.8 else int(rng.choice([1 << 50, (1 << 62) + (1 << 57),
                                                                                       (1 << 63) - 1]))
    size = int(rng.integers(0, 3000))
    return n_bytes, n_ch, (drain, size, int(rng.integers(0, (size << Q) + 1)))


def test_the_recursion_is_the_maximum_over_all_stretches():
    rng = np.random.default_rng(11)
    seen = {"over": 0, "clamped": 0, "start_counts": 0, "largest": 0}
    for _ in range(400):
        n_bytes, n_ch, b = drawn(rng)
        thr, s = pn.through(n_bytes, n_ch, b)
        assert thr == pn.brute(n_bytes, n_ch, b)
        X = [x << Q for x in kb.hop_bytes(n_bytes, n_ch)]
        # a hop's own level is a stretch that ends at it; through is the same for F_h + R_h and L_h + R_h - X_h
        assert all(t >= lv for t, lv in zip(thr, s["level"]))
        assert all(t < (1 << 62) + (1 << 57) for t in thr)
        # a hop lies in a stretch that overflows exactly when a level at or behind it, reached without running empty
        # between, is above the buffer: the first hop above the buffer is the first entry above it too
        over = [h for h, t in enumerate(thr) if t > b[1] << Q]
        assert (s["first_over"] >= 0) == bool(over) and (not over or over[0] <= s["first_over"])
        assert max([b[2]] + thr) == s["peak_q16"]
        seen["over"] += bool(over)
        seen["clamped"] += any(lv - b[0] < 0 for lv in s["level"][:-1])
        seen["start_counts"] += bool(X) and b[2] > 0 and thr[0] > X[0]
        seen["largest"] += b[2] == 1 << 56 and len(X) > 0
    assert min(seen.values()) > 5, seen


def monotone(n_hops, n_ch, seed, loud=()):
    """bytes that never rise with the target: frame cf takes weight[cf] (T_HI + 64 - t) / 64 bytes, the hops in `loud`
    eight times the weight of the others.  -> evaluate(targets) -> n_bytes"""
    rng = np.random.default_rng(seed)
    w = rng.integers(2, 9, n_hops * n_ch)
    for h in loud:
        w[h * n_ch:(h + 1) * n_ch] *= 8
    return lambda targets: (w * (T_HI + 64 - np.repeat(np.asarray(targets, np.int64), n_ch)) // 64).astype(np.int64)


def uniform_solve(ev, n_ch, n_hops, limit, b):
    return kb.solve(lambda t: ev([t] * n_hops), n_ch, limit, b, T_LO, T_HI)


def test_phase_zero_is_the_buffered_solve():
    """max_phases = 1: every shared output is bucket_model.solve's, on the models' own curves and every probe's path"""
    band, rate = bm.synthetic(60, 3), am.synthetic(60, 40, 12, 3)
    for c, evaluate in ((band, bm.evaluate), (rate, am.evaluate)):
        one = lambda t: evaluate(c, t)                                           # noqa: E731
        ev = pn.per_hop(one, 2)
        small, big = one(T_HI)[0], one(T_LO)[0]
        peaks = [kb.scan(one(t)[2], 2, (300 << Q, kb.SIZE_MAX, 0))["peak_q16"] >> Q for t in (T_HI, T_LO)]
        for limit in ((small + big) // 2, small - 1, 10 ** 12):
            for size in (kb.SIZE_MAX, peaks[0] + (peaks[1] - peaks[0]) // 5, 0):
                b = (300 << Q, size, 0)
                ref = kb.solve(one, 2, limit, b, T_LO, T_HI)
                sol = pn.solve(ev, 2, 30, limit, b, T_LO, T_HI, 64, 1)
                for k in ("t", "met", "total"):
                    assert sol[k] == ref[k], (limit, size, k)
                for k in ("n_bytes", "per_cf", "capped"):
                    assert np.array_equal(sol[k], ref[k]), (limit, size, k)
                assert {k: sol["bucket"][k] for k in kb.FIELDS} == {k: ref["bucket"][k] for k in kb.FIELDS}
                assert [p[2:] for p in sol["path"] if p[1] == "fit"] == ref["path"]
                assert sol["phases"] == ref["met"] and sol["target_t"] == [ref["t"]] * 30
                if size == kb.SIZE_MAX:                      # a buffer no level reaches: nothing is pinned, not open
                    assert set(sol["phase_of"]) == {-1} and not sol["open"]
                    many = pn.solve(ev, 2, 30, limit, b, T_LO, T_HI, 64, 8)
                    assert many["phases"] == ref["met"] and many["target_t"] == sol["target_t"]
                    assert np.array_equal(many["n_bytes"], sol["n_bytes"]) and set(many["phase_of"]) == {-1}


@pytest.mark.parametrize("step", [1, 64, 640])
def test_by_construction_on_monotone_curves(step):
    n_hops, n_ch, loud = 40, 2, (5, 6, 7, 20, 33, 34)
    ev = monotone(n_hops, n_ch, 4, loud)
    mean = kb.scan(ev([0] * n_hops), n_ch, (0, kb.SIZE_MAX, 0))["total"] // n_hops
    drain = mean << Q
    limit = mean * n_hops
    one_hop = max(kb.hop_bytes(ev([0] * n_hops), n_ch))
    b = (drain, one_hop, 0)                                   # the loud hops at 0 dB just fit one by one: runs bind
    one = uniform_solve(ev, n_ch, n_hops, limit, b)
    whole = uniform_solve(ev, n_ch, n_hops, limit, (drain, kb.SIZE_MAX, 0))
    assert one["met"] and whole["met"] and one["t"] > whole["t"] + 64       # the buffer costs the one target over a dB
    sol = pn.solve(ev, n_ch, n_hops, limit, b, T_LO, T_HI, step, 16)
    found = sol["levels"]
    # p_k is the lowest level phase k's bisection accepted, p_k-1 if it accepted none
    for k in range(sol["phases"]):
        accepted = [p[2] for p in sol["path"] if p[0] == k and p[1] == "fit" and p[5]]
        assert found[k] == min(accepted + found[max(k - 1, 0):k]) and len(found) == sol["phases"]
    # the premise: more than one phase pinned hops, and hops stayed free
    assert sol["met"] and not sol["open"] and sol["phases"] >= 3
    assert len({k for k in sol["phase_of"] if k >= 0}) == sol["phases"] - 1 and -1 in sol["phase_of"]
    # the assignment returned fits, both ways
    assert sol["total"] <= limit and sol["bucket"]["peak_q16"] <= one_hop << Q and sol["bucket"]["first_over"] == -1
    assert sol["total"] == kb.scan(ev(sol["target_t"]), n_ch, b)["total"]
    # phase 0 found the one-target answer; no hop ends above it; the free hops end below it
    assert found[0] == one["t"] == max(sol["target_t"])
    assert sol["t"] == min(sol["target_t"]) < one["t"]
    assert all((t == sol["t"]) == (k < 0 or t == sol["t"]) for t, k in zip(sol["target_t"], sol["phase_of"]))
    # a pinned hop carries the level of its phase, and the levels fall by at least the step every phase the buffer bound
    assert found[-1] == sol["t"]
    for h, k in enumerate(sol["phase_of"]):
        assert sol["target_t"][h] == (sol["t"] if k < 0 else found[k])
    froze = [p for p in sol["path"] if p[1] == "freeze"]
    for k in range(1, sol["phases"] - 1):                  # in the last phase the size may bind
        assert found[k] <= max(T_LO, found[k - 1] - step), (k, found)
    # the end: the lowest target is reached, or the probe below the last level pinned nothing
    assert found[-1] <= found[-2] and (found[-1] == T_LO or (len(froze) == sol["phases"] and froze[-1][3] == 0))
    assert all(p[3] > 0 for p in froze[:sol["phases"] - 1]) and len(froze) >= sol["phases"] - 1
    # more bytes spent than under the one target, within the same size and the same buffer
    assert one["total"] < sol["total"] <= limit
    print(f"step {step}: one target {one['t']}, whole stream {whole['t']}, levels {found}, "
          f"pinned {sum(k >= 0 for k in sol['phase_of'])} of {n_hops}, bytes {one['total']} -> {sol['total']} of {limit}")


def test_a_step_of_the_whole_range():
    """the probe lies at t_lo: every hop in a stretch that overflows THERE is pinned at p_0 at once -- here all of them,
    so the second phase's level moves no hop and falls to t_lo.  The guarantees hold; nothing is gained"""
    n_hops, n_ch = 40, 2
    ev = monotone(n_hops, n_ch, 4, (5, 6, 7, 20, 33, 34))
    mean = kb.scan(ev([0] * n_hops), n_ch, (0, kb.SIZE_MAX, 0))["total"] // n_hops
    b = (mean << Q, max(kb.hop_bytes(ev([0] * n_hops), n_ch)), 0)
    one = uniform_solve(ev, n_ch, n_hops, mean * n_hops, b)
    sol = pn.solve(ev, n_ch, n_hops, mean * n_hops, b, T_LO, T_HI, T_HI - T_LO, 16)
    assert sol["met"] and not sol["open"] and sol["phases"] == 2 and sol["levels"] == [one["t"], T_LO]
    assert set(sol["phase_of"]) == {0} and sol["target_t"] == [one["t"]] * n_hops
    assert np.array_equal(sol["n_bytes"], one["n_bytes"]) and sol["bucket"]["peak_q16"] <= b[1] << Q


def test_phases_run_out():
    n_hops, n_ch, loud = 40, 2, (5, 6, 7, 20, 33, 34)
    ev = monotone(n_hops, n_ch, 4, loud)
    mean = kb.scan(ev([0] * n_hops), n_ch, (0, kb.SIZE_MAX, 0))["total"] // n_hops
    b = (mean << Q, max(kb.hop_bytes(ev([0] * n_hops), n_ch)), 0)
    full = pn.solve(ev, n_ch, n_hops, mean * n_hops, b, T_LO, T_HI, 1, 16)
    assert full["phases"] >= 3 and not full["open"]
    for K in (1, 2):
        sol = pn.solve(ev, n_ch, n_hops, mean * n_hops, b, T_LO, T_HI, 1, K)
        assert sol["open"] == 1 and sol["phases"] == K and sol["met"]
        assert sol["bucket"]["peak_q16"] <= b[1] << Q and sol["total"] <= mean * n_hops
        assert max(sol["phase_of"]) == K - 1               # the last phase's hops are marked, at the level returned
        assert all(sol["target_t"][h] == sol["t"] for h, k in enumerate(sol["phase_of"]) if k in (-1, K - 1))
        assert sol["t"] >= full["t"]
    # the phase that ends a solve without pinning does not count as open, whatever the count allowed
    exact = pn.solve(ev, n_ch, n_hops, mean * n_hops, b, T_LO, T_HI, 1, full["phases"])
    assert not exact["open"] and exact["target_t"] == full["target_t"]


def test_a_curve_that_is_not_monotone_still_fits():
    """hops 2 and 3 take MORE bytes from -5 dB up to 5 dB than below: every probe is measured, so what is returned fits"""
    n_hops, n_ch = 8, 1
    quiet = lambda t: 40 if t < 0 else 30                                          # noqa: E731
    odd = lambda t: 42 if t < -320 else 755 if t < 320 else 30                    # noqa: E731
    ev = lambda targets: np.array([odd(t) if h in (2, 3) else quiet(t) for h, t in enumerate(targets)])   # noqa: E731
    b = (100 << Q, 500, 0)
    uniform = lambda t: kb.scan(ev([t] * n_hops), n_ch, b)                         # noqa: E731
    assert uniform(-321)["peak_q16"] <= 500 << Q < uniform(-320)["peak_q16"] and uniform(320)["peak_q16"] <= 500 << Q
    for step in (1, 64, 700):
        sol = pn.solve(ev, n_ch, n_hops, 1 << 62, b, T_LO, T_HI, step, 8)
        assert sol["met"] and sol["bucket"]["peak_q16"] <= 500 << Q and sol["bucket"]["first_over"] == -1
        accepted = [p for p in sol["path"] if p[1] == "fit" and p[5]]
        assert accepted[-1][3:5] == (sol["total"], sol["bucket"]["peak_q16"]) or sol["t"] == accepted[-1][2]
        assert max(sol["target_t"]) <= uniform_solve(ev, n_ch, n_hops, 1 << 62, b)["t"]


def test_library_exports_the_pinned_calls(A):
    lib = A.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pacx.h")).read()
    assert text.index('#include "pacx_bucket.h"') < text.index('#include "pacx_bucket_pin.h"')
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pacx_bucket_pin.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header)) == set(NAMES) == set(A._lib.BUCKET_PIN_SIGNATURES)
    assert not set(NAMES) & (set(A._lib.SIGNATURES) | set(A._lib.BUCKET_SIGNATURES))
    for name in NAMES:
        assert hasattr(lib, name), name
        args = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(A._lib.BUCKET_PIN_SIGNATURES[name][1]) == len(args.split(",")), name
        assert getattr(lib, name).argtypes == A._lib.BUCKET_PIN_SIGNATURES[name][1]
    # a pinned solve takes its buffered sibling's arguments, the step and the phases behind the range, the per-hop
    # arrays behind capped, the third result behind the other two
    for kind in ("band", "rate"):
        plain = re.search(r"\bint pacx_%s_solve_bucket\((.*?)\);" % kind,
                          open(os.path.join(root, "include", "pacx_bucket.h")).read(), flags=re.S).group(1)
        pinned = re.search(r"\bint pacx_%s_solve_bucket_pinned\((.*?)\);" % kind, header, flags=re.S).group(1)
        words = lambda s: [" ".join(a.split()) for a in s.split(",")]            # noqa: E731
        p, q = words(plain), words(pinned)
        at = p.index("double nmr_hi_db") + 1
        assert q == p[:at] + ["int32_t pin_step_t", "int32_t max_phases"] + p[at:at + 3] + \
            ["int32_t *target_t", "int32_t *phase_of"] + p[at + 3:-1] + ["pacx_pin_result *pin_result", "void *stream"]
    assert "#define PACX_PIN_PHASES_MAX 16" in header and A._lib.PIN_PHASES_MAX == pn.PHASES_MAX == 16
    assert A._lib.PIN_RESULT == ("phases", "open")
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7
    Encoder = A.engine.Encoder
    assert list(inspect.signature(Encoder.bucket_through).parameters) == \
        ["self", "n_bytes", "n_channels", "bucket", "want_level"]
    assert list(inspect.signature(Encoder.band_solve_bucket_pinned).parameters) == \
        ["self", "curve", "n_channels", "limit_bytes", "bucket", "nmr_lo_db", "nmr_hi_db", "pin_step_db", "max_phases"]
    assert list(inspect.signature(Encoder.rate_solve_bucket_pinned).parameters) == \
        ["self", "curve", "flags", "n_channels", "limit_bytes", "bucket", "nmr_lo_db", "nmr_hi_db", "pin_step_db",
         "max_phases"]
    for name in ("band_solve_bucket_pinned", "rate_solve_bucket_pinned"):
        p = inspect.signature(getattr(Encoder, name)).parameters
        assert (p["pin_step_db"].default, p["max_phases"].default) == (1.0, 8)
    buffered = list(inspect.signature(A.pacfile.encode_stream_abr_buffered).parameters)
    pinned = inspect.signature(A.pacfile.encode_stream_abr_pinned).parameters
    assert list(pinned) == buffered + ["pin_step_db", "max_phases"]
    assert (pinned["pin_step_db"].default, pinned["max_phases"].default) == (1.0, 8)
    assert all(pinned[k].default == inspect.signature(A.pacfile.encode_stream_abr_buffered).parameters[k].default
               for k in buffered)
    # a null handle is refused before anything is read
    assert lib.pacx_bucket_through(None, 0, 1, None, None, None, None, None, None) == A._lib.E_ARG
    assert lib.pacx_band_solve_bucket_pinned(None, 0, 1, None, None, None, 0, None, -30.0, 30.0, 64, 8, None, None, None,
                                             None, None, None, None, None, None) == A._lib.E_ARG
    assert lib.pacx_rate_solve_bucket_pinned(None, 0, 1, 8, 1, None, None, None, 0, None, -30.0, 30.0, 64, 8, None, None,
                                             None, None, None, None, None, None, None) == A._lib.E_ARG


def test_refusals_before_gpu_work(A, monkeypatch):
    from audio_codec_amd import context, pacfile, quality
    Encoder = A.engine.Encoder
    assert Encoder._pin_args("x", 1.0, 8) == (64, 8) and Encoder._pin_args("x", 1 / 64, 1) == (1, 1)
    assert Encoder._pin_args("x", 60, np.int64(16)) == (3840, 16)
    for bad in (0, -1, 0.01, 1 / 128, "a", None, float("nan"), float("inf"), 1e9):
        with pytest.raises(ValueError, match="pin_step_db"):
            Encoder._pin_args("x", bad, 8)
    for bad in (0, 17, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="max_phases"):
            Encoder._pin_args("x", 1.0, bad)

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    for call in (pacfile.encode_stream_abr_pinned, quality.encode_stream_to_buffer_pinned):
        for kw, word in ((dict(pin_step_db=0), "pin_step_db"), (dict(pin_step_db=0.01), "pin_step_db"),
                         (dict(pin_step_db=-1), "pin_step_db"), (dict(max_phases=0), "max_phases"),
                         (dict(max_phases=17), "max_phases"), (dict(max_phases=1.5), "max_phases"),
                         (dict(allocation="bands"), "allocation"), (dict(buffer_bytes=-1), None),
                         (dict(kbps_per_channel=0), None), (dict(start_bytes=4001), None),
                         (dict(nmr_range_db=(3, -3)), None)):
            with pytest.raises(ValueError, match=word):
                call(pcm, 44100, **dict(dict(kbps_per_channel=96, buffer_bytes=4000), **kw))
        with pytest.raises(NotImplementedError, match="^gain-shape streams: allocation 'band' only$"):
            call(pcm, 44100, 96, 4000, use_vq=True)
        for kw in (dict(), dict(allocation="band", use_vq=True), dict(pin_step_db=1 / 64, max_phases=16)):
            with pytest.raises(AssertionError, match="an encoder was asked for"):
                call(pcm, 44100, 96, 4000, **kw)
