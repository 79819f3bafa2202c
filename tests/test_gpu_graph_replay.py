"""A captured step, replayed, gives the bytes of the direct call (bench.py --graph; DESIGN.md 5.0 / 5.1 quote figures
from replayed steps, and nothing checked their output).

What is captured is what bench.py captures and what profiles/r02_bench_scalar128_graph.json and
r02_bench_bs128_graph.json show replaying: the scalar all-long step (encode_pack -> gather_body) and the block-switched
step (transient_flags -> encode_pack -> gather_body), one handle, after pacx_reserve and one direct run on the capture
stream, with torch.cuda.graph on a stream of the test's.  Three replays with the PCM buffer's contents replaced in
between -- real, decoy, real (tests/stream_order.py: the decoy is the other excerpt) -- each equal to the direct call on
the same contents and to the reference's .pac body of that excerpt.

Not captured: gain-shape steps (pacx_api.hip, pacx_encode_vq_batch: "bench.py does not capture gain-shape steps", the two
k_vq_frame launches do not overlap when replayed) and segmented or peak solves (include/pacx.h, pacx_rate_solve_segments:
"not meant for stream capture into a graph", they upload through a pinned buffer and may wait for the host).
"""
import ctypes

import numpy as np
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


@pytest.mark.parametrize("step", ["all_long", "block_switched"])
def test_a_replayed_step_gives_the_direct_calls_bytes(A, step):
    import torch
    ptr = A.engine._ptr
    variant = "long" if step == "all_long" else "bs"
    real, decoy = (so.scalar_material(n, variant) for n in so.PAIRS[variant])
    n_frames, n_ch = real["n_frames"], real["n_ch"]
    n_hops, n_cf = n_frames - 2, n_frames * n_ch
    enc = A.engine.Encoder(so.SR, 128 / 44.1)
    try:
        enc.reserve(n_cf)
        dev = enc.device
        contents = {"real": torch.as_tensor(real["planar"], device=dev), "decoy": torch.as_tensor(decoy["planar"], device=dev)}
        pcm = contents["decoy"].clone()
        view = A.engine.PcmView.stream(pcm)
        hop_view = A._lib.PacxPcm(pcm.data_ptr() + 2 * so.HOP, A._lib.PCM_I16, n_ch, n_hops, so.HOP, pcm.shape[1], 1)
        out = enc.alloc_outputs(n_cf, with_payload=True)
        cap = n_cf * (enc.payload_stride + 4)
        body = torch.zeros((cap,), dtype=torch.uint8, device=dev)
        total = torch.zeros((1,), dtype=torch.int64, device=dev)
        tr = torch.zeros((n_hops,), dtype=torch.uint8, device=dev)
        fl = torch.zeros((n_hops + 2,), dtype=torch.uint8, device=dev)
        results = (body, total, out["n_bytes"], fl)

        def part():
            """the kernels of one step: what a hipGraph of the step holds (bench.py, encode_part)"""
            if step == "block_switched":
                enc._call("pacx_transient_flags", ctypes.byref(hop_view), ptr(tr), ptr(fl), enc._stream())
            enc.encode_pack(view, fl if step == "block_switched" else None, out)
            enc._call("pacx_gather_body", ctypes.c_int64(n_cf), ptr(out["payload"]), ptr(out["n_bytes"]), ptr(body),
                      ctypes.c_int64(cap), ptr(total), enc._stream())

        def taken():
            torch.cuda.synchronize()
            n = int(total.item())
            got = (bytes(body[:n].cpu().numpy()), out["n_bytes"].cpu().numpy().copy(), fl.cpu().numpy().copy())
            for t in results:                                   # nothing of this run is left for the next to pass on
                t.fill_(0x5A if t.dtype == torch.uint8 else -1)
            torch.cuda.synchronize()
            return got

        want = {}
        for name, t in contents.items():                        # the direct call on either contents, default stream
            pcm.copy_(t)
            part()
            want[name] = taken()
        assert want["real"][0] == real["body"] and want["decoy"][0] == decoy["body"], "the direct call misses the reference"
        assert want["real"][0] != want["decoy"][0]
        if step == "block_switched":
            assert want["real"][2].tolist() == real["flags"].tolist() and want["decoy"][2].tolist() == decoy["flags"].tolist()

        s = torch.cuda.Stream(device=dev)
        pcm.copy_(contents["decoy"])
        torch.cuda.synchronize()
        with torch.cuda.stream(s):                              # one direct run on the capture stream
            part()
        assert taken()[0] == decoy["body"]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            part()
        torch.cuda.synchronize()
        for i, name in enumerate(("real", "decoy", "real")):
            pcm.copy_(contents[name])
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            got = taken()
            assert got[0] == want[name][0], f"replay {i} ({name}): the body differs from the direct call's"
            assert np.array_equal(got[1], want[name][1]), f"replay {i} ({name}): n_bytes"
            if step == "block_switched":
                assert np.array_equal(got[2], want[name][2]), f"replay {i} ({name}): flags"
        del g
    finally:
        torch.cuda.synchronize()
        enc.close()
