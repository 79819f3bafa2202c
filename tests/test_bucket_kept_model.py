"""CPU checks of the buffered solve for a stream in chunks (include/pacx_bucket_kept.h): tests/bucket_kept_model.py's tree
against bucket_model.solve -- the same target, the same results and the same probes in the same order, for every depth,
on ranges from one target to 8193 and on data whose fit is monotone in the target or arbitrary; the fold of a scan in
pieces against the whole scan for a cut at every hop; the header's exports against the binding; what the two new pacfile
calls and solve_bucket refuse before an encoder exists; and the new signatures."""
import inspect
import os
import re

import numpy as np
import pytest

import bucket_kept_model as bt
import bucket_model as bk

NAMES = ("pacx_band_bytes_thresholds", "pacx_rate_bytes_thresholds", "pacx_bucket_scan_targets", "pacx_bucket_tree_begin",
         "pacx_bucket_tree_step")
RANGES = [(-7, -7), (0, 1), (-1, 1), (-128, 128), (-1920, 1920), (-4096, 4096)]      # 1, 2, 3, 257, 3841, 8193 targets


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


def monotone(t_lo, t_hi, seed):
    """six hops of two channels whose bytes fall as the target rises"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 9, 12)
    return lambda t: [int(v) * (t_hi - t + 1) for v in w]


def arbitrary(t_lo, t_hi, seed):
    """bytes drawn afresh at every target: total and peak go up and down with it"""
    def at(t):
        rng = np.random.default_rng((seed, t - t_lo))
        return [int(v) for v in rng.integers(0, 400, 12)]
    return at


def rising_peak(t_lo, t_hi, seed):
    """the total falls with the target while one hop's burst rises with it: the buffer binds from above"""
    return lambda t: [4 * (t_hi - t + 1), 0, 0, 0, 3 * (t - t_lo), 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("t_lo,t_hi", RANGES)
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_the_tree_walks_the_plain_bisections_path(t_lo, t_hi, levels):
    G = t_hi - t_lo + 1
    for make in (monotone, arbitrary, rising_peak):
        for seed in range(6):
            evaluate = make(t_lo, t_hi, seed)
            sizes = [sum(v + 4 for v in evaluate(t) if v > 0) for t in (t_lo, (t_lo + t_hi) // 2, t_hi)]
            # limits that never bind, bind in the middle, and fail at t_hi; buffers that do the same
            for limit in (max(sizes) * 4, sizes[1], max(min(sizes) - 1, 0)):
                for size in (1 << 30, 900 if make is not monotone else 8 * G, 3):
                    bucket = (int(2.5 * 65536) * (seed + 1), size, min(size, 2) << 16)
                    want = bk.solve(evaluate, 2, limit, bucket, t_lo, t_hi)
                    got = bt.solve(evaluate, 2, limit, bucket, t_lo, t_hi, levels, cuts=(1, 4))
                    assert (got["t"], got["met"], got["total"]) == (want["t"], want["met"], want["total"])
                    assert got["bucket"] == {k: want["bucket"][k] for k in bt.FIELDS}
                    assert got["path"] == [p[0] for p in want["path"]]
                    assert got["passes"] == -(-(1 + G.bit_length()) // levels)
                    assert got["evaluated"] == got["passes"] * ((1 << levels) - 1)


def test_the_passes_of_the_default_range():
    assert [bt.passes(-1920, 1920, L) for L in (1, 2, 3, 4, 5)] == [13, 7, 5, 4, 3]
    assert [bt.passes(0, 0, L) for L in (1, 5)] == [2, 1]


def test_a_pass_holds_every_target_the_bisection_can_reach():
    """the heap's children are the decisions' probes; a slot below the end repeats the target found"""
    s = bt.begin(-3, 3)
    tt = bt.targets(s, 3)
    assert tt[0] == 3 and tt[1] == 3 and tt[2] == -1                  # t_hi fails: done at t_hi; fits: mid of (-4, 3]
    assert tt[3] == tt[4] == 3                                        # below the failed probe of t_hi
    assert tt[5] == 1 and tt[6] == -3                                 # lo = -1 -> mid 1; hi = -1 -> floor(-5 / 2)
    one = bt.targets(bt.begin(5, 5), 5)
    assert one == [5] * 31


def test_the_fold_of_pieces_is_the_whole_scan_for_a_cut_at_every_hop():
    rng = np.random.default_rng(70)
    n_ch, n_hops = 2, 70
    base = rng.integers(0, 120, n_hops * n_ch)
    base[rng.random(n_hops * n_ch) < 0.2] = 0
    patterns = {"drawn": base.copy(), "silence": np.zeros_like(base)}
    twin = np.zeros_like(base)                                        # equal peaks in two pieces: the earlier hop stands
    twin[2 * 10], twin[2 * 50] = 5000, 5000
    patterns["twin"] = twin
    burst = base.copy()
    burst[2 * 33:2 * 36] = 900                                        # over the buffer in the middle, and it stays full
    patterns["burst"] = burst
    for name, nb in patterns.items():
        for bucket in ((int(90.25 * 65536), 600, 0), (int(90.25 * 65536), 600, 600 << 16), (1 << 60, 5004, 0),
                       (0, 1 << 40, 7)):
            whole = bk.scan(nb, n_ch, bucket)
            want = {k: whole[k] for k in bt.FIELDS}
            for cut in range(n_hops + 1):
                assert bt.scan_pieces(nb, n_ch, bucket, (cut,)) == want, (name, bucket, cut)
            assert bt.scan_pieces(nb, n_ch, bucket, range(1, n_hops)) == want       # a hop a piece
            assert bt.scan_pieces(nb, n_ch, bucket, (0, 0, 10, 10, 50, 70)) == want  # empty pieces
    assert bk.scan(twin, n_ch, (1 << 60, 5004, 0))["peak_hop"] == 10


def test_the_header_and_the_binding_name_the_same_exports(A):
    lib = A.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pacx.h")).read()
    assert text.index('#include "pacx_bucket_pin.h"') < text.index('#include "pacx_bucket_kept.h"')
    between = text[text.index('#include "pacx_bucket_pin.h"'):text.index('#include "pacx_bucket_kept.h"')]
    assert "#include" not in between[len('#include "pacx_bucket_pin.h"'):]              # right behind it
    raw = open(os.path.join(root, "include", "pacx_bucket_kept.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header)) == set(NAMES) == set(A._lib.BUCKET_KEPT_SIGNATURES)
    assert not set(NAMES) & set(A._lib.SIGNATURES)
    for name in NAMES:
        args = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(A._lib.BUCKET_KEPT_SIGNATURES[name][1]) == len(args.split(",")), name
        assert getattr(lib, name).argtypes == A._lib.BUCKET_KEPT_SIGNATURES[name][1]
    consts = dict(re.findall(r"#define (PACX_BUCKET_TREE_[A-Z_]+) (\d+)", header))
    assert (int(consts["PACX_BUCKET_TREE_LEVELS_MAX"]), int(consts["PACX_BUCKET_TREE_TARGETS"]),
            int(consts["PACX_BUCKET_TREE_STATE_BYTES"])) == \
        (A._lib.BUCKET_TREE_LEVELS_MAX, A._lib.BUCKET_TREE_TARGETS, A._lib.BUCKET_TREE_STATE_BYTES) == \
        (bt.LEVELS_MAX, bt.TARGETS, 128)
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7
    for name in ("band_bytes_thresholds", "rate_bytes_thresholds", "bucket_scan_targets", "bucket_tree_begin",
                 "bucket_tree_step", "bucket_tree_result"):
        assert callable(getattr(A.engine.Encoder, name)), name
    from audio_codec_amd import pacfile
    for path in (pacfile._BandPath, pacfile._BudgetPath):
        assert callable(path.bytes_kept)
    from audio_codec_amd import build
    assert "k_bucket_kept.hip" in build.SOURCES
    assert any(h.endswith("pacx_bucket_kept.h") for h in build._headers())
    for (t_lo, t_hi) in RANGES:
        for L in range(1, 6):
            assert A.engine.Encoder.bucket_tree_passes(t_lo / 64, t_hi / 64, L) == bt.passes(t_lo, t_hi, L)


def test_the_new_calls_refuse_before_an_encoder_is_asked_for(A, monkeypatch):
    from audio_codec_amd import context, pacfile, streaming

    def no_encoder(*a, **k):
        raise AssertionError("an encoder was asked for before the arguments were checked")
    monkeypatch.setattr(context, "encoder_for_params", no_encoder)
    pcm = np.zeros((4096, 2), np.int16)
    cp = pacfile._rate_coding_params(pcm, 44100, 320, None)
    pacfile.header_bytes(cp)
    for call in (pacfile.encode_stream_abr_buffered_kept, pacfile.iter_encode_abr_buffered_kept):
        ok = dict(kbps_per_channel=96, buffer_bytes=20000, chunk_hops=2)
        # encode_stream_abr_buffered's own refusals, word for word (that call checks them before it asks for an encoder)
        for kw in (dict(allocation="bands"), dict(allocation="budget", use_vq=True), dict(nmr_range_db=(3, -3)),
                   dict(nmr_range_db=(0.001, 1)), dict(kbps_per_channel=0), dict(buffer_bytes=-1),
                   dict(buffer_bytes=2.5), dict(start_bytes=20001), dict(drain_kbps_per_channel=-1),
                   dict(max_kbps_per_channel=2000)):
            with pytest.raises((ValueError, NotImplementedError)) as ours:
                call(pcm, 44100, **{**ok, **kw})
            kw1 = {k: v for k, v in {**ok, **kw}.items() if k != "chunk_hops"}
            with pytest.raises((ValueError, NotImplementedError)) as theirs:
                pacfile.encode_stream_abr_buffered(pcm, 44100, **kw1)
            assert type(ours.value) is type(theirs.value) and str(ours.value) == str(theirs.value), kw
        with pytest.raises(ValueError, match="^pcm: int16 \\[samples, channels\\]$"):
            call(np.zeros(4096, np.int16), 44100, **ok)
        # the chunked call's, with its messages
        for kw in (dict(chunk_hops=0), dict(chunk_hops=2.5), dict(chunk_hops=True), dict(nmr_range_db=(-100, 100))):
            with pytest.raises(ValueError) as ours:
                call(pcm, 44100, **{**ok, **kw})
            with pytest.raises(ValueError) as chunked:
                pacfile.encode_stream_abr_chunked(pcm, 44100, kbps_per_channel=96, allocation="budget",
                                                  **{"chunk_hops": 2, **kw})
            assert str(ours.value) == str(chunked.value)
        with pytest.raises(ValueError, match="at least one block"):
            call(np.zeros((0, 2), np.int16), 44100, **ok)
        with pytest.raises(ValueError, match="n a multiple of 1024"):
            call(np.zeros((1000, 2), np.int16), 44100, **ok)
        for bad in (0, 6, 2.0, True, None, "4"):
            with pytest.raises(ValueError, match="levels.*whole number in \\[1, 5\\]"):
                call(pcm, 44100, levels=bad, **ok)
        # the store's
        for allocation in ("band", "budget"):
            need = 6 * 2 * pacfile._kept_bytes_per_cf(cp, allocation)
            kw = dict(ok, allocation=allocation)
            with pytest.raises(ValueError, match="curve_store.*it holds %d" % (need - 1)):
                call(pcm, 44100, curve_store=np.zeros(need - 1, np.uint8), **kw)
            frozen = np.zeros(need, np.uint8)
            frozen.setflags(write=False)
            with pytest.raises(ValueError, match="curve_store.*read-only"):
                call(pcm, 44100, curve_store=frozen, **kw)
            with pytest.raises(ValueError, match="curve_store.*not uint8"):
                call(pcm, 44100, curve_store=np.zeros(need, np.int8), **kw)
            for store in (None, np.zeros(need, np.uint8), bytearray(need)):
                for levels in (1, 4, 5):
                    with pytest.raises(AssertionError, match="an encoder was asked for"):
                        call(pcm, 44100, curve_store=store, levels=levels, **kw)
    # solve_bucket on the object: RuntimeError without kept curves, ValueError for its own arguments, nothing queued
    hr = streaming.HostStreamRateEncoder.__new__(streaming.HostStreamRateEncoder)
    hr.keep, hr.kept = None, None
    bucket = pacfile.bucket(96, 2, 44100, 20000)
    with pytest.raises(RuntimeError, match="solve_bucket: after keep_curves\\(\\) and analyse\\(\\)"):
        hr.solve_bucket(1000, bucket)
    hr.keep_curves()
    with pytest.raises(RuntimeError, match="solve_bucket: after keep_curves\\(\\) and analyse\\(\\)"):
        hr.solve_bucket(1000, bucket)
    with pytest.raises(RuntimeError, match="level_at: after keep_curves"):
        hr.level_at(30, bucket, 0)
    hr.kept = {"store": np.zeros(8, np.uint8), "hops": 2, "per_block": 2}
    for kw, why in ((dict(levels=0), "levels"), (dict(levels=6), "levels"), (dict(levels=1.5), "levels"),
                    (dict(limit_bytes=-1), "limit_bytes"), (dict(limit_bytes=0.5), "limit_bytes"),
                    (dict(bucket=(1, 2)), "a bucket is three integers"), (dict(bucket=(1.5, 2, 0)), "three integers")):
        with pytest.raises(ValueError, match="solve_bucket.*" + why):
            hr.solve_bucket(**{"limit_bytes": 1000, "bucket": bucket, **kw})


def test_the_new_signatures(A):
    from audio_codec_amd import pacfile, streaming
    buffered = list(inspect.signature(pacfile.encode_stream_abr_buffered).parameters)
    for call in (pacfile.encode_stream_abr_buffered_kept, pacfile.iter_encode_abr_buffered_kept):
        sig = inspect.signature(call)
        assert list(sig.parameters) == buffered + ["chunk_hops", "curve_store", "levels"]
        for name in buffered:
            assert sig.parameters[name].default == inspect.signature(pacfile.encode_stream_abr_buffered).parameters[name].default
        assert (sig.parameters["chunk_hops"].default, sig.parameters["curve_store"].default,
                sig.parameters["levels"].default) == (4096, None, 4)
    sig = inspect.signature(streaming.HostStreamRateEncoder.solve_bucket)
    assert list(sig.parameters) == ["self", "limit_bytes", "bucket", "levels"] and sig.parameters["levels"].default == 4
    E = A.engine.Encoder
    assert list(inspect.signature(E.band_bytes_thresholds).parameters) == ["self", "kept", "target_t", "out"]
    assert list(inspect.signature(E.rate_bytes_thresholds).parameters) == ["self", "kept", "target_t", "out"]
    assert list(inspect.signature(E.bucket_scan_targets).parameters) == \
        ["self", "n_bytes_t", "n_channels", "drain_q16", "size_bytes", "hop_off", "acc"]
    assert list(inspect.signature(E.bucket_tree_begin).parameters) == \
        ["self", "bucket", "nmr_lo_db", "nmr_hi_db", "levels", "tree"]
    assert list(inspect.signature(E.bucket_tree_step).parameters) == ["self", "limit_bytes", "bucket", "levels", "tree"]
