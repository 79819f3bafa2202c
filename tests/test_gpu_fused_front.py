"""The fused front end of an all-long step (k_front_long: the frame's MDCT in the wave that runs its side chain,
PACX_FUSE_FRONT=1) against the two separate kernels (PACX_FUSE_FRONT=0): every output of encode_pack must be the
same bits -- overall scales (all sub-block slots), scale factors, bit allocation, the 1024 line-indexed mantissa
codes per channel-frame (the proxy for the MDCT lines), status words, byte counts and payload bytes.

Batches: 2, 3, 2048 and 2050 channel-frames -- one wave per channel; an odd mono batch; the smallest batch that takes
the XCD-aware frame order (n_cf % 2048 == 0); plain order with a last partial group.  Spliced in: a hop of zeros, a
hop with the code -32768 (which counts as 0 and takes the fold's second pass) in every position class of the fold,
and a full-scale square wave.  The overrides are read when a handle is created, so every setting gets a fresh handle.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

OUTPUTS = ("overall", "scale_factor", "bit_alloc", "mantissa", "status", "n_bytes")
ENV = "PACX_FUSE_FRONT"


@pytest.fixture(scope="module")
def A():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import audio_codec_amd as a
    return a


@pytest.fixture
def fresh_handles(A):
    A.context.clear()
    yield
    A.context.clear()


def _set(A, monkeypatch, value):
    if value is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, value)
    A.context.clear()                              # encode_stream creates handles that read it


def _special_hops(base):
    """zeros; the code -32768 at hop positions 0, 511, 512, 1023 of every channel -- as the first half of one block
    these are its samples 0, 511, 512, 1023, as the second half of the block before 1024, 1535, 1536, 2047: every
    quarter of the fold, both ends; a +-32767 square wave (period 64 samples)"""
    zeros = np.zeros_like(base)
    low = base.copy()
    low[[0, 511, 512, 1023], :] = -32768
    square = np.where((np.arange(1024) // 32) % 2 == 0, 32767, -32767).astype(np.int16)
    square = np.repeat(square[:, None], base.shape[1], axis=1)
    return zeros, low, square


@pytest.fixture(scope="module")
def programme(A):
    """1025 stereo hops of the synthetic stream, made once; the batches below are slices and copies of it"""
    pcm = A.synth.stream(1025, 2)
    pcm.setflags(write=False)
    return pcm


def _batch(programme, name):
    if name == "stereo1":
        return programme[:1024].copy()
    if name == "mono3":
        pcm = programme[:3 * 1024, :1].copy()
        at = (0, 1, 2)
    elif name == "stereo1024":
        return programme[:1024 * 1024].copy()
    else:
        assert name == "stereo1025"
        pcm = programme.copy()
        at = (500, 501, 502)
    for h, hop in zip(at, _special_hops(pcm[at[1] * 1024:(at[1] + 1) * 1024])):
        pcm[h * 1024:(h + 1) * 1024] = hop
    if name == "stereo1025":                       # the last frame (the partial group) ends on codes -32768 as well
        pcm[1024 * 1024 + 512:1024 * 1024 + 520, 1] = -32768
        assert (pcm[501 * 1024 + 511] == -32768).all() and (pcm[500 * 1024:501 * 1024] == 0).all()
    return pcm


def _encode(A, enc, pcm, flags=None):
    """encode_pack into buffers prefilled with a pattern: what a path does not write is equal on both sides, what only
    one of them initialises is not"""
    import torch
    planar = torch.as_tensor(A.synth.planar_with_halo(pcm), device=enc.device)
    view = A.engine.PcmView.stream(planar)
    out = enc.alloc_outputs(view.n_cf, with_payload=True)
    for t in out.values():
        t.view(torch.uint8).fill_(0x5A)
    out = enc.encode_pack(view, flags, out, want_mantissa=True)
    torch.cuda.synchronize()
    used = torch.arange(out["payload"].shape[1], device=enc.device)[None, :] < out["n_bytes"][:, None]
    res = {k: out[k].clone() for k in OUTPUTS}
    res["payload"] = torch.where(used, out["payload"], torch.zeros_like(out["payload"]))
    return res


def _assert_same(got, want, what):
    import torch
    for k in OUTPUTS + ("payload",):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k)


def _reference(A, monkeypatch, cache, programme, name, guard=False):
    """outputs of the separate kernels (PACX_FUSE_FRONT=0), computed once per batch"""
    key = (name, guard)
    if key not in cache:
        _set(A, monkeypatch, "0")
        enc = A.engine.Encoder(48000, 128 / 48.0, guard=guard)
        try:
            cache[key] = _encode(A, enc, _batch(programme, name))
        finally:
            enc.close()
    return cache[key]


@pytest.fixture(scope="module")
def ref_cache():
    return {}


@pytest.mark.parametrize("name", ["stereo1", "mono3", "stereo1024", "stereo1025"])
def test_fused_front_same_bits(A, monkeypatch, fresh_handles, ref_cache, programme, name):
    """PACX_FUSE_FRONT=1 and the default against PACX_FUSE_FRONT=0, on a handle's default schedule"""
    want = _reference(A, monkeypatch, ref_cache, programme, name)
    pcm = _batch(programme, name)
    n_cf = pcm.shape[0] // 1024 * pcm.shape[1]
    assert want["status"].shape == (n_cf,)
    for value in ("1", None):
        _set(A, monkeypatch, value)
        enc = A.engine.Encoder(48000, 128 / 48.0)
        try:
            _assert_same(_encode(A, enc, pcm), want, (name, value))
        finally:
            enc.close()
    _set(A, monkeypatch, None)


@pytest.mark.parametrize("name", ["mono3", "stereo1025"])
def test_fused_front_guard_words(A, monkeypatch, fresh_handles, ref_cache, programme, name):
    """handles that compute PACX_ST_GUARD: the fused kernel writes the status word's guard bit itself"""
    want = _reference(A, monkeypatch, ref_cache, programme, name, guard=True)
    _set(A, monkeypatch, "1")
    enc = A.engine.Encoder(48000, 128 / 48.0, guard=True)
    try:
        _assert_same(_encode(A, enc, _batch(programme, name)), want, name)
    finally:
        enc.close()
    _set(A, monkeypatch, None)


def test_fused_front_in_a_pool(A, monkeypatch, fresh_handles, ref_cache, programme):
    """the 2048-cf batch on the handles of EncoderPool(2, ...): side fork switched on (it has no effect on the fused
    step), a stream that is not the default one"""
    want = _reference(A, monkeypatch, ref_cache, programme, "stereo1024")
    pcm = _batch(programme, "stereo1024")
    _set(A, monkeypatch, "1")
    pool = A.engine.EncoderPool(2, 48000, 128 / 48.0)
    try:
        for _ in range(2):
            k = pool.next()
            with pool.slot(k) as enc:
                got = _encode(A, enc, pcm)
            _assert_same(got, want, ("pool slot", k))
    finally:
        for e in pool.encs:
            e.close()
    _set(A, monkeypatch, None)


def test_flags_keep_the_separate_kernels(A, monkeypatch, fresh_handles, programme):
    """a per-frame flags tensor of zeros (every frame a long sine block, but a flagged batch) does not take the fused
    front end: visible only as the same outputs whatever the switch says"""
    import torch
    pcm = _batch(programme, "mono3")
    got = {}
    for value in ("0", "1"):
        _set(A, monkeypatch, value)
        enc = A.engine.Encoder(48000, 128 / 48.0)
        try:
            got[value] = _encode(A, enc, pcm, torch.zeros(3, dtype=torch.uint8, device=enc.device))
        finally:
            enc.close()
    _assert_same(got["1"], got["0"], "flags of zeros")
    _set(A, monkeypatch, None)


def test_excerpt_stream_same_bytes(A, monkeypatch, fresh_handles):
    """the committed harpsichord excerpt through encode_stream with long blocks: the .pac bytes of the default and of
    PACX_FUSE_FRONT=1 are those of PACX_FUSE_FRONT=0"""
    ex = np.load(os.path.join(GOLDEN, "excerpt_harpsichord.npz"))
    pcm, sr = ex["pcm"], int(ex["sr"])
    _set(A, monkeypatch, "0")
    want = A.pacfile.encode_stream(pcm, sr, 128, block_switching=False)
    for value in (None, "1"):
        _set(A, monkeypatch, value)
        assert A.pacfile.encode_stream(pcm, sr, 128, block_switching=False) == want, value
    _set(A, monkeypatch, None)
