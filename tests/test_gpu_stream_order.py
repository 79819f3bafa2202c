"""The stream contract of include/pacx.h ("work is enqueued on `stream` and is asynchronous", "handles are independent",
a segmented solve "waits for the upload of the segmented solve before it on the same handle, and for nothing else")
under the schedule of tests/stream_order.py: every case runs on four caller streams of the test's, behind a producer that
holds the stream while the real inputs, the call, the keep-copies and the overwrites are queued with no host wait.

Bars.  Plain equality, no tolerance: the same kernels on the same data.  Truth is the same call made synchronously on
the default stream; where tests/golden has the reference's bytes or PCM for the case, truth is those as well, and for
the solves on curves it is the models (abr_model, band_model, segment_model, peak_model, bucket_model, profile_model,
rate_profile_model, kept_model).  The vq_band chain and Encoder.nmr have the synchronous call alone: their models are
held to the kernels in test_gpu_vq_band.py and test_gpu_nmr.py on other material.

Measured on an MI355X (test_zz_report prints the figures of a run): the dry pass of a sequence takes the host 0.06 to
0.82 ms, the delay is 8 times that and 40 ms at least (39.8 to 60.4 ms by events), the largest host time from the
producer to the last queued overwrite was 0.83 ms (1.03 ms in another run); the negative control bit on all eight
stream pairs.  DESIGN.md
section 2, the row "stream contract", has the same figures.
"""
import ctypes

import numpy as np
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu

BPS128 = 128 / 44.1
CAP_BPS = 320 / 44.1
HOP = so.HOP


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


@pytest.fixture(scope="module")
def rig(A):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return {"clock": so.Clock(dev), "streams": so.caller_streams(dev), "device": dev}


@pytest.fixture
def handles(A):
    """encoders of a test, closed behind it; overrides are read when a handle is created, so a test that sets one does
    so (monkeypatch) before it asks for the handle"""
    made = []

    def make(bps=BPS128, sr=so.SR, **kw):
        made.append(A.engine.Encoder(sr, bps, **kw))
        return made[-1]
    yield make
    import torch
    torch.cuda.synchronize()
    for e in made:
        e.close()


def on_every_stream(rig, enc, case, what, check):
    """truth once, then the delayed schedule on each caller stream; check(got, truth) must hold on all of them"""
    truth = so.run_direct(*case)
    failed = []
    for i, s in enumerate(rig["streams"]):
        got = so.run_delayed(enc, s, *case, rig["clock"], what=f"{what}, caller stream {i}")
        try:
            check(got, truth)
        except AssertionError as e:
            failed.append(f"caller stream {i}: {e}")
    assert not failed, f"{what}: " + "; ".join(failed)
    return truth


# ------------------------------------------------------------------------------------------------- the encodes
def encode_case(A, enc, real, decoy, layout="planar", vq=False):
    """encode_pack / encode_vq of a whole batch; layout planar (PcmView.stream), interleaved (a strided view: not
    `fast`, so no split) or frames (PcmView.frames)"""
    V = A.engine.PcmView
    n_frames, n_ch = real["n_frames"], real["n_ch"]

    def prepare():
        job = so.Job(enc.device)
        if layout == "frames":
            job.pcm = job.add(real["blocks"], decoy["blocks"])
            job.view = V.frames(job.pcm)
        elif layout == "interleaved":
            job.pcm = job.add(real["planar"].T, decoy["planar"].T)
            job.view = V(job.pcm, n_ch, n_frames, n_ch * HOP, 1, n_ch)
        else:
            job.pcm = job.add(real["planar"], decoy["planar"])
            job.view = V.stream(job.pcm)
        job.flags = None if real["flags"] is None else job.add(real["flags"], decoy["flags"])
        n_cf = n_frames * n_ch
        job.out = enc.alloc_vq_outputs(n_cf) if vq else enc.alloc_outputs(n_cf, with_payload=True)
        return job

    def call(job):
        (enc.encode_vq if vq else enc.encode_pack)(job.view, job.flags, job.out)

    def collect(job):
        return {k: job.out[k] for k in ("n_bytes", "payload", "status")}
    return prepare, call, collect


def records_check(records):
    """a check for on_every_stream: the synchronous call's rows, which are the reference's records"""
    def check(got, truth):
        assert so.valid_payload(truth["n_bytes"], truth["payload"]) == records, "the synchronous call misses the reference"
        bad = so.same_records(got, truth)
        assert not bad, f"{len(bad)} of {len(records)} channel-frames differ, first {bad[:6]}"
    return check


BITES = {}


def test_the_method_bites(A, rig, handles):
    """Negative control: the producer and the copies on caller stream i, the call deliberately on stream i + 1, which
    waits for nothing -- it reads the decoy, and the result must differ from truth.  A pair that does not bite shares a
    hardware queue (the call was held behind the producer anyway); if none bites the method sees nothing here."""
    enc = handles()
    cases = {"all-long": encode_case(A, enc, *(so.scalar_material(n, "long") for n in so.PAIRS["long"])),
             "block-switched": encode_case(A, enc, *(so.scalar_material(n, "bs") for n in so.PAIRS["bs"]))}
    streams = rig["streams"]
    for name, case in cases.items():
        truth = so.run_direct(*case)
        for i, s in enumerate(streams):
            j = (i + 1) % len(streams)
            got = so.run_delayed(enc, s, *case, rig["clock"], call_stream=streams[j], what=f"control {name} {i}->{j}")
            BITES[(name, i, j)] = bool(so.same_records(got, truth))
    print("negative control bit on", sorted(k for k, v in BITES.items() if v), "and not on",
          sorted(k for k, v in BITES.items() if not v))
    assert any(BITES.values()), "a call made on a stream that waits for nothing gave the truth on every pair"
    # and the method itself, on the right stream, passes on the same handle
    def same(got, truth):
        bad = so.same_records(got, truth)
        assert not bad, (len(bad), bad[:6])
    for name, case in cases.items():
        on_every_stream(rig, enc, case, name, same)


ALL_LONG = {"default": ({}, False), "front0": ({"PACX_FUSE_FRONT": "0"}, False),
            "front0_side_fork": ({"PACX_FUSE_FRONT": "0"}, True), "tail0": ({"PACX_FUSE_TAIL": "0"}, False),
            "tail1": ({"PACX_FUSE_TAIL": "1"}, False)}


@pytest.mark.parametrize("path", sorted(ALL_LONG))
def test_encode_pack_all_long(A, rig, handles, monkeypatch, path):
    """scalar encode_pack without flags: the fused front (default), PACX_FUSE_FRONT=0 on one stream and with the side
    chain forked (side_stream, ev_fork / ev_join), the tail in k_mask or behind it"""
    env, fork = ALL_LONG[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    enc = handles()
    monkeypatch.undo()
    enc.set_side_fork(fork)
    real, decoy = (so.scalar_material(n, "long") for n in so.PAIRS["long"])
    on_every_stream(rig, enc, encode_case(A, enc, real, decoy), f"all-long {path}", records_check(real["records"]))


@pytest.mark.parametrize("path", ["split", "split0", "strided"])
def test_encode_pack_block_switched(A, rig, handles, monkeypatch, path):
    """castanet with the reference driver's flags: the split (ev_fork before the lists, ev_lists behind them,
    ev_short_done), PACX_SPLIT_SHORT=0, and a strided int16 view, which is not `fast` and takes no split"""
    if path == "split0":
        monkeypatch.setenv("PACX_SPLIT_SHORT", "0")
    enc = handles()
    monkeypatch.undo()
    real, decoy = (so.scalar_material(n, "bs") for n in so.PAIRS["bs"])
    case = encode_case(A, enc, real, decoy, layout="interleaved" if path == "strided" else "planar")
    on_every_stream(rig, enc, case, f"block-switched {path}", records_check(real["records"]))


@pytest.mark.parametrize("name", sorted(so.FLAGGED))
def test_encode_pack_with_an_empty_frame_list(A, rig, handles, name):
    """flagged batches of mixed_batches items without one short-coded frame, and without one long-coded frame: the
    split runs with one of its chains empty; rows against the oracle's"""
    import mixed_batches as mb
    enc = handles(128 / (mb.SR / 1000), sr=mb.SR)
    real, decoy = so.flagged_material(name, False), so.flagged_material(name, True)
    case = encode_case(A, enc, real, decoy, layout="frames")
    on_every_stream(rig, enc, case, f"flagged {name}", records_check(so.flagged_records(real)))


def test_the_benchmarks_step_as_one_chain(A, rig, handles):
    """pacx_transient_flags -> encode_pack with those device flags -> pacx_gather_body, nothing waiting on the host in
    between: the body is the reference's .pac body"""
    enc = handles()
    real, decoy = (so.scalar_material(n, "bs") for n in so.PAIRS["bs"])
    n_hops, n_cf = real["n_frames"] - 2, real["n_frames"] * 2

    def prepare():
        job = so.Job(enc.device)
        job.pcm = job.add(real["planar"], decoy["planar"])
        job.view = A.engine.PcmView.stream(job.pcm)
        job.out = enc.alloc_outputs(n_cf, with_payload=True)
        return job

    def call(job):
        _, job.fl = enc.transient_flags(job.pcm, n_hops)
        enc.encode_pack(job.view, job.fl, job.out)
        job.body, job.total = enc.gather_body(job.out["payload"], job.out["n_bytes"])

    def collect(job):
        return {"flags": job.fl, "body": job.body, "total": job.total, "n_bytes": job.out["n_bytes"]}

    def check(got, truth):
        n = int(truth["total"][0])
        assert truth["flags"].tolist() == real["flags"].tolist() and bytes(truth["body"][:n]) == real["body"], \
            "the synchronous chain misses the reference"
        assert got["flags"].tolist() == truth["flags"].tolist(), "flags"
        assert int(got["total"][0]) == n and np.array_equal(got["n_bytes"], truth["n_bytes"]), "sizes"
        assert bytes(got["body"][:n]) == real["body"], "body"
    on_every_stream(rig, enc, (prepare, call, collect), "benchmark step", check)


@pytest.mark.parametrize("path", ["vq128", "vq96_sbr", "vq128_frame0"])
def test_encode_vq(A, rig, handles, monkeypatch, path):
    """gain-shape, block-switched: 128 kb/s, 96 kb/s with SBR (the second fork site), PACX_VQ_FRAME=0 once"""
    kbps = 96 if path == "vq96_sbr" else 128
    if path == "vq128_frame0":
        monkeypatch.setenv("PACX_VQ_FRAME", "0")
    enc = handles(kbps / 44.1, use_vq=True, use_sbr=kbps < 128)
    monkeypatch.undo()
    real, decoy = (so.vq_material(n, kbps) for n in so.PAIRS["bs"])
    on_every_stream(rig, enc, encode_case(A, enc, real, decoy, vq=True), path, records_check(real["records"]))


# ------------------------------------------------------------------------------------------------- decode, NMR
def decode_case(A, enc, real, decoy, vq):
    """pacx_index_body -> unpack + decode (or decode_vq) -> pacx_overlap_add_pcm in two pieces with the tail carried, as
    decode_stream chains them; the bodies are the reference's own"""
    bodies = so.padded_bodies(real["body"], decoy["body"])
    n_rec, n_ch = len(real["records"]), real["n_ch"]
    half = n_rec // (2 * n_ch) * n_ch

    def prepare():
        job = so.Job(enc.device)
        job.body = job.add(*bodies)
        job.tail = job.add(np.zeros((n_ch, HOP)), np.full((n_ch, HOP), 0.25))
        return job

    def call(job):
        offs, sizes, index = enc.index_body(job.body[:-8], n_ch, True, n_rec)      # the parsers may read 8 bytes on
        pcm = []
        for a, b, flush in ((0, half, False), (half, n_rec, True)):
            if vq:
                blocks = enc.decode_vq(job.body, sizes[a:b], n_ch, offsets=offs[a:b], want_blocks=True,
                                       want_pcm=False)["blocks"]
            else:
                blocks = enc.decode(enc.unpack(job.body, sizes[a:b], offs[a:b]), n_ch, want_blocks=True, want_pcm=False)
            pcm.append(enc.overlap_add(blocks, job.tail, flush))
        job.res = {"index": index, "offsets": offs, "sizes": sizes, "pcm0": pcm[0], "pcm1": pcm[1]}

    def collect(job):
        return dict(job.res)
    return prepare, call, collect


@pytest.mark.parametrize("tag", ["bs", "long", "vq128", "vq96"])
def test_decode_chain(A, rig, handles, tag):
    vq = tag.startswith("vq")
    if vq:
        enc = handles(BPS128, use_vq=True, use_sbr=tag == "vq96")
        real, decoy = (so.vq_material(n, int(tag[2:])) for n in so.PAIRS["bs"])
    else:
        enc = handles()
        real, decoy = (so.scalar_material(n, tag) for n in so.PAIRS["bs"])
    want = so.decoded(so.PAIRS["bs"][0], tag)

    def check(got, truth):
        assert int(truth["index"][0]) == len(real["records"]), truth["index"]
        assert np.array_equal(np.concatenate((truth["pcm0"], truth["pcm1"])), want), "the synchronous chain misses the reference"
        bad = so.same_arrays(got, truth)
        assert not bad, bad
    on_every_stream(rig, enc, decode_case(A, enc, real, decoy, vq), f"decode {tag}", check)


def test_nmr_behind_the_encode_and_decode_that_feed_it(A, rig, handles):
    enc = handles()
    real, decoy = (so.scalar_material(n, "bs") for n in so.PAIRS["bs"])
    prepare, encode, _ = encode_case(A, enc, real, decoy)

    def call(job):
        encode(job)
        codes = enc.unpack(job.out["payload"], job.out["n_bytes"])
        extra = {}
        enc.decode(codes, real["n_ch"], want_pcm=False, extra=extra)
        job.nmr = enc.nmr(job.view, job.flags, extra["lines"], codes["overall"])

    def collect(job):
        return {**job.nmr, "n_bytes": job.out["n_bytes"]}

    def check(got, truth):
        assert np.isfinite(truth["nmr_db"]).any()
        bad = so.same_arrays(got, truth)
        assert not bad, bad
    on_every_stream(rig, enc, (prepare, call, collect), "nmr", check)


# ------------------------------------------------------------------------------------------------- two handles
def test_two_handles_behind_the_start_gate(A, rig):
    """EncoderPool(2) behind align, so that both slots really start together: block-switched scalar in both slots,
    block-switched scalar beside gain-shape, encode beside decode.  Each slot's result is the one-handle result."""
    import torch
    pool = A.engine.EncoderPool(2, so.SR, BPS128)
    vq_enc = A.engine.Encoder(so.SR, BPS128, use_vq=True)
    try:
        cas, har = so.scalar_material("castanet", "bs"), so.scalar_material("harpsichord", "bs")
        vq_r, vq_d = (so.vq_material(n, 128) for n in so.PAIRS["bs"])
        scalar = pool.encs[1]
        pairs = {
            "scalar beside scalar": (encode_case(A, pool.encs[0], cas, har), encode_case(A, pool.encs[1], har, cas), None),
            "scalar beside gain-shape": (encode_case(A, pool.encs[0], cas, har),
                                         encode_case(A, vq_enc, vq_r, vq_d, vq=True), vq_enc),
            "encode beside decode": (encode_case(A, pool.encs[0], cas, har), decode_case(A, pool.encs[1], cas, har, False),
                                     None),
        }
        for name, (c0, c1, other) in pairs.items():
            pool.encs[1] = other or scalar
            truth = [so.run_direct(*c0), so.run_direct(*c1)]
            got = so.run_pool(pool, (c0, c1), what=f"pool, {name}")
            for k in (0, 1):
                if "payload" in truth[k]:
                    bad = so.same_records(got[k], truth[k])
                    assert not bad, (name, k, len(bad), bad[:6])
                else:
                    assert not so.same_arrays(got[k], truth[k]), (name, k)
        pool.encs[1] = scalar
        want = so.valid_payload(truth[0]["n_bytes"], truth[0]["payload"])
        assert want == cas["records"]                      # what the slots were held to is the reference's
    finally:
        torch.cuda.synchronize()
        pool.close()
        vq_enc.close()


# ------------------------------------------------------------------------------------------------- rate control
def curve_truth(kind, curve_host):
    """the model's curve dict around arrays a GPU curve call wrote"""
    import band_model as bm
    from oracle import pac_oracle as po
    if kind == "band":
        return bm.with_arrays(bm.tables(po.make_params(so.SR, 1, 128)), curve_host["nmr"], curve_host["cap"],
                              curve_host["cap_alloc"])
    return {k: curve_host[k] for k in so.KEYS["rate"]}


@pytest.mark.parametrize("kind", so.KINDS)
def test_curve_solve_second_pass(A, rig, handles, kind):
    """rate_curve -> rate_solve -> encode_pack_budget and band_curve -> band_solve -> encode_pack_alloc on castanet,
    block-switched, the solve through its C entry point (the wrapper reads the result back).  The solve's answer is the
    model's on the curve the synchronous chain took."""
    import abr_model as am
    import band_model as bm
    enc = handles()
    real, decoy = (so.scalar_material(n, "bs") for n in so.PAIRS["bs"])
    limit = len(real["body"]) * 3 // 4
    n_cf = real["n_frames"] * real["n_ch"]
    prepare0, _, _ = encode_case(A, enc, real, decoy)

    def prepare():
        job = prepare0()
        job.sol = so.solve_outputs(enc, kind, n_cf, 1)
        return job

    def call(job):
        if kind == "rate":
            job.curve = enc.rate_curve(job.view, job.flags, CAP_BPS)
        else:
            job.curve = enc.band_curve(job.view, job.flags, CAP_BPS)
        so.queue_solve(enc, kind, "solve", job.curve, n_cf, job.sol, limit=limit)
        if kind == "rate":
            enc.encode_pack_budget(job.view, job.flags, job.sol["per_cf"], job.out)
        else:
            enc.encode_pack_alloc(job.view, job.flags, job.sol["per_cf"], job.out)

    def collect(job):
        return {**{k: job.curve[k] for k in so.KEYS[kind]}, **job.sol,
                **{k: job.out[k] for k in ("n_bytes", "payload", "status")}}
    seen = {}

    def check(got, truth):
        if not seen:
            c = curve_truth(kind, truth)
            if kind == "rate":
                c["row"], c["sub_stride"] = enc.rate_curve_layout(CAP_BPS)
            ref = (am.solve if kind == "rate" else bm.solve)(c, limit, so.T_LO, so.T_HI)
            t, met, total = so.result_words(truth["result"])
            assert (int(t[0]), int(met[0]), int(total[0])) == (ref["t"], ref["met"], ref["total"])
            assert so.T_LO < ref["t"] < so.T_HI and ref["met"]
            assert np.array_equal(truth["per_cf"], ref["budget" if kind == "rate" else "bit_alloc"])
            seen["ok"] = True
        bad = so.same_arrays({k: got[k] for k in got if k != "payload"}, {k: truth[k] for k in truth if k != "payload"})
        assert not bad, bad
        rows = so.same_records(got, truth)
        assert not rows, (len(rows), rows[:6])
    on_every_stream(rig, enc, (prepare, call, collect), f"{kind} curve, solve, second pass", check)


def curve_job(enc, kind):
    """a Job whose inputs are the arrays of the synthetic curve (real) over the other seed's (decoy)"""
    real, decoy = so.curve_material(kind, False), so.curve_material(kind, True)
    job = so.Job(enc.device)
    job.dev = {k: job.add(real[k], decoy[k]) for k in so.KEYS[kind]}
    if kind == "rate":
        assert (real["row"], real["sub_stride"]) == (decoy["row"], decoy["sub_stride"])
        job.dev["row"], job.dev["sub_stride"] = real["row"], real["sub_stride"]
    return job


def solved(out, n_seg=1):
    """a solve's outputs as the models name them"""
    t, met, total = so.result_words(out["result"][:n_seg])
    return {"t": t, "met": met, "total": total, "per_cf": out["per_cf"], "n_bytes": out["n_bytes"],
            "capped": out["capped"].astype(bool)}


def same_as_model(got, ref, what):
    for k, v in got.items():
        assert np.array_equal(v, np.asarray(ref[k]).astype(v.dtype)), (what, k)


@pytest.mark.parametrize("kind", so.KINDS)
def test_bucket_solve_then_scan(A, rig, handles, kind):
    """the buffered solve followed by pacx_bucket_scan with levels over the n_bytes it has just written"""
    import bucket_model as kb
    enc = handles()
    jobs, n_cf, n_ch = so.solve_jobs(kind), so.CURVE_CF, so.CURVE_CH
    ref = so.model_answers(kind, so.curve_material(kind, False))["bucket"]
    ptr = A.engine._ptr

    def prepare():
        import torch
        job = curve_job(enc, kind)
        job.sol = so.solve_outputs(enc, kind, n_cf, 4)
        job.level = torch.full((n_cf // n_ch,), -1, dtype=torch.int64, device=enc.device)
        job.scan = torch.full((len(kb.FIELDS),), -1, dtype=torch.int64, device=enc.device)
        return job

    def call(job):
        so.queue_solve(enc, kind, "solve_bucket", job.dev, n_cf, job.sol, limit=jobs["bucket_limit"],
                       bucket=jobs["bucket"], n_ch=n_ch)
        enc._call("pacx_bucket_scan", ctypes.c_int64(n_cf // n_ch), n_ch, ptr(job.sol["n_bytes"]),
                  ctypes.byref(A._lib.PacxBucket(*jobs["bucket"])), ptr(job.level), ptr(job.scan), enc._stream())

    def collect(job):
        return {**job.sol, "level": job.level, "scan": job.scan}

    def check(got, truth):
        for r in (truth, got):
            same_as_model(solved(r), ref, "solve")
            words = np.ascontiguousarray(r["result"][1:]).reshape(-1).view(np.int64)[:len(kb.FIELDS)]
            assert words.tolist() == ref["scan"].tolist() == r["scan"].tolist(), "the bucket's result"
            assert np.array_equal(r["level"], ref["level"]), "levels"
    on_every_stream(rig, enc, (prepare, call, collect), f"{kind} bucket", check)


@pytest.mark.parametrize("kind", so.KINDS)
def test_profile_then_profile_solve(A, rig, handles, kind):
    import profile_model as pm
    import rate_profile_model as rp
    enc = handles()
    limit = so.solve_jobs(kind)["limit"]
    c = so.curve_material(kind, False)
    prof = pm.profile(c, so.T_LO, so.T_HI) if kind == "band" else rp.profile(c, so.T_LO, so.T_HI)
    ref = pm.solve(prof, limit, so.T_LO, so.T_HI)
    ptr = A.engine._ptr

    def prepare():
        import torch
        job = curve_job(enc, kind)
        job.result = torch.full((1, 4), -1, dtype=torch.int32, device=enc.device)
        return job

    def call(job):
        job.profile = (enc.band_profile if kind == "band" else enc.rate_profile)(job.dev)
        enc._call_rate("pacx_profile_solve", ptr(job.profile), ctypes.c_int64(limit), ctypes.c_double(-30.0),
                       ctypes.c_double(30.0), ptr(job.result), enc._stream())

    def collect(job):
        return {"profile": job.profile, "result": job.result}

    def check(got, truth):
        for r in (truth, got):
            assert np.array_equal(r["profile"], prof), "profile"
            t, met, total = so.result_words(r["result"])
            assert (int(t[0]), int(met[0]), int(total[0])) == (ref["t"], ref["met"], ref["total"]), "solve"
    on_every_stream(rig, enc, (prepare, call, collect), f"{kind} profile", check)


@pytest.mark.parametrize("kind", so.KINDS)
def test_thresholds_then_pick(A, rig, handles, kind):
    import kept_model as km
    enc = handles()
    c = so.curve_material(kind, False)
    t = int(so.model_answers(kind, c)["plain"]["t"][0])
    kept = (km.band_thresholds if kind == "band" else km.rate_thresholds)(c, so.T_LO, so.T_HI)
    ref = (km.band_pick if kind == "band" else km.rate_pick)(kept, t)
    per = "bit_alloc" if kind == "band" else "budget"

    def prepare():
        return curve_job(enc, kind)

    def call(job):
        if kind == "band":
            job.kept = enc.band_thresholds(job.dev)
            job.pick = enc.band_pick_thresholds(job.kept, t / 64)
        else:
            job.kept = enc.rate_thresholds(job.dev)
            job.pick = enc.rate_pick_thresholds(job.kept, t / 64)

    def collect(job):
        return {"e": job.kept["e"], per: job.pick[per], "n_bytes": job.pick["n_bytes"], "capped": job.pick["capped"]}

    def check(got, truth):
        for r in (truth, got):
            assert np.array_equal(r["e"], kept["e"]), "thresholds"
            for k in (per, "n_bytes", "capped"):
                assert np.array_equal(r[k], np.asarray(ref[k]).astype(r[k].dtype)), k
    on_every_stream(rig, enc, (prepare, call, collect), f"{kind} thresholds", check)


def test_vq_band_curve_pick_second_pass(A, rig, handles):
    """vq_band_curve on the gain-shape handle -> band_pick on its scalar sibling -> encode_vq_alloc, on two hops"""
    enc = handles(BPS128, use_vq=True)
    sib = A.context.scalar_sibling(enc)
    at = 25 * HOP                                              # castanet: the stroke and the hop behind it
    mats = []
    for name, flags in (("castanet", [0, 4, 2, 1]), ("harpsichord", [4, 2, 1, 0])):
        pcm = so.excerpt(name)["pcm"][at:at + 2 * HOP]
        mats.append({"planar": so.planar_stream(pcm), "flags": np.array(flags, np.uint8), "n_frames": 4, "n_ch": 2})
    prepare, _, _ = encode_case(A, enc, *mats, vq=True)

    def call(job):
        job.curve = enc.vq_band_curve(job.view, job.flags, CAP_BPS)
        job.pick = sib.band_pick(job.curve, -12.0)
        enc.encode_vq_alloc(job.view, job.flags, job.pick["bit_alloc"], job.out)

    def collect(job):
        return {**{k: job.curve[k] for k in so.KEYS["band"]}, "pick": job.pick["bit_alloc"], "picked": job.pick["n_bytes"],
                **{k: job.out[k] for k in ("n_bytes", "payload", "status")}}

    def check(got, truth):
        assert (truth["n_bytes"] > 0).all() and truth["pick"].any()
        bad = so.same_arrays({k: got[k] for k in got if k != "payload"}, {k: truth[k] for k in truth if k != "payload"})
        assert not bad, bad
        assert not so.same_records(got, truth)
    on_every_stream(rig, enc, (prepare, call, collect), "vq band curve", check)


@pytest.mark.parametrize("kind", so.KINDS)
def test_the_pinned_staging_buffer(A, rig, handles, kind):
    """Two segmented solves with different limits and segment counts queued back to back on one handle behind the
    delay, a peak solve behind them: each gives its own model answer.  Without the wait on ev_seg in upload_segments the
    first would receive the second's table.  The second call is the one that may wait for the host (stream_order.MAY_BLOCK):
    validity is checked right before it."""
    enc = handles()
    jobs, n_cf = so.solve_jobs(kind), so.CURVE_CF
    ref = so.model_answers(kind, so.curve_material(kind, False))
    first_c, peaks, limit = jobs["peak"]
    n_a, n_b, n_c = len(jobs["segments_a"][1]), len(jobs["segments_b"][1]), len(peaks)

    def prepare():
        job = curve_job(enc, kind)
        job.a, job.b = so.solve_outputs(enc, kind, n_cf, n_a), so.solve_outputs(enc, kind, n_cf, n_b)
        job.c = so.solve_outputs(enc, kind, n_cf, n_c + 1 + (n_c + 3) // 4)
        return job

    def call(job):
        so.queue_solve(enc, kind, "solve_segments", job.dev, n_cf, job.a, seg_first=jobs["segments_a"][0],
                       limits=jobs["segments_a"][1])
        job.checkpoint(f"pacx_{kind}_solve_segments")
        so.queue_solve(enc, kind, "solve_segments", job.dev, n_cf, job.b, seg_first=jobs["segments_b"][0],
                       limits=jobs["segments_b"][1])
        so.queue_solve(enc, kind, "solve_peak", job.dev, n_cf, job.c, seg_first=first_c, limits=peaks, limit=limit)

    def collect(job):
        return {f"{n}_{k}": v for n, o in (("a", job.a), ("b", job.b), ("c", job.c)) for k, v in o.items()}

    def check(got, truth):
        for r in (truth, got):
            part = lambda n: {k[2:]: v for k, v in r.items() if k.startswith(n + "_")}       # noqa: E731
            same_as_model(solved(part("a"), n_a), ref["segments_a"], "the first segmented solve")
            same_as_model(solved(part("b"), n_b), ref["segments_b"], "the second segmented solve")
            c = part("c")
            same_as_model(solved(c, n_c), {k: ref["peak"][k] for k in ("t", "met", "total", "per_cf", "n_bytes", "capped")},
                          "the peak solve")
            t, met, total = so.result_words(c["result"][n_c:n_c + 1])
            assert [int(t[0]), int(met[0]), int(total[0])] == ref["peak"]["stream"].tolist(), "the peak solve's stream"
            assert c["result"][n_c + 1:].reshape(-1)[:n_c].tolist() == ref["peak"]["floor"].tolist(), "floors"
    on_every_stream(rig, enc, (prepare, call, collect), f"{kind} staging buffer", check)


def test_zz_report():
    """the figures DESIGN.md section 2 quotes, printed from this run (every run has asserted its own validity)"""
    runs = [r for r in so.LOG if not r["control"]]
    assert runs, "no delayed run was made"
    worst = max(runs, key=lambda r: r["host_ms"] / r["delay_ms"])
    print(f"\nstream order: {len(runs)} delayed runs; calibrated delays {min(r['delay_ms'] for r in runs):.1f} to "
          f"{max(r['delay_ms'] for r in runs):.1f} ms (held, by events: "
          f"{np.nanmin([r['held_ms'] for r in runs]):.1f} to {np.nanmax([r['held_ms'] for r in runs]):.1f} ms); dry pass "
          f"{np.nanmin([r['dry_ms'] for r in runs]):.3f} to {np.nanmax([r['dry_ms'] for r in runs]):.3f} ms; largest host "
          f"queue time {max(r['host_ms'] for r in runs):.3f} ms; smallest delay / host time {worst['delay_ms'] / worst['host_ms']:.1f} "
          f"({worst['what']})")
    print("negative control bit on:", sorted(k for k, v in BITES.items() if v), "not on:",
          sorted(k for k, v in BITES.items() if not v))
    for what, names, sentence in so.MAY_BLOCK:
        print(f"may block: {what} {names}: \"{sentence}\"")
