"""Decoding a .pac in chunks: the record index built on the device (pacx_index_body), the overlap-and-add
with a carried half-block (pacx_overlap_add_pcm), streaming.HostStreamDecoder and pacfile.iter_decode /
decode_stream(..., chunk_bytes=N) on top of them.  Everything is compared exactly: the index is integer
work and the overlap sum keeps the order of the one-batch path."""
import ctypes
import io
import os
import struct

import numpy as np
import pytest

import index_cases
from conftest import EXCERPTS, GOLDEN, load_excerpt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    return a


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def enc(A):
    return A.context.encoder(48000, 128 / 48.0)


# ------------------------------------------------------------------ the record index
def device_index(A, torch, enc, body, n_channels, final, max_records, lead=0):
    """pacx_index_body on `body` (placed `lead` bytes into its device buffer, so that its address takes every
    alignment) with canaries behind the arrays -> (offsets, sizes, result) as lists"""
    from audio_codec_amd.engine import _ptr
    dev = torch.frombuffer(bytearray(b"\xee" * lead + body + b"\xee" * 16), dtype=torch.uint8).to(enc.device)[lead:]
    offs = torch.full((max_records + 2,), -7, dtype=torch.int64, device=enc.device)
    sizes = torch.full((max_records + 2,), -7, dtype=torch.int32, device=enc.device)
    result = torch.full((3,), -99, dtype=torch.int64, device=enc.device)
    enc._call("pacx_index_body", _ptr(dev), ctypes.c_int64(len(body)), n_channels, final, ctypes.c_int64(max_records),
              _ptr(offs), _ptr(sizes), _ptr(result), enc._stream())
    result = result.cpu().tolist()
    n = result[0]
    assert 0 <= n <= max_records
    offs, sizes = offs.cpu().numpy(), sizes.cpu().numpy()
    assert np.all(offs[n:] == -7) and np.all(sizes[n:] == -7), "wrote past the records it returned"
    return offs[:n].tolist(), sizes[:n].tolist(), result


def test_index_body_equals_the_host_walk_on_every_case(A, torch, enc):
    assert enc.payload_stride == index_cases.MAX_RECORD
    n_cases = 0
    for i, (name, body, n_ch, final, max_records) in enumerate(index_cases.cases(A._lib.INDEX_SEGMENT)):
        want = index_cases.expected(A.pacfile.record_chain, body, n_ch, final, max_records)
        got = device_index(A, torch, enc, body, n_ch, final, max_records, lead=i % 4)
        assert got[2] == want[2], (name, got[2], want[2])
        assert got[0] == want[0], name
        assert got[1] == want[1], name
        n_cases += 1
    assert n_cases > 300


def _golden_pacs():
    for name in EXCERPTS:
        ex = load_excerpt(name)
        for tag in ("long", "bs"):
            yield f"{name}_{tag}", bytes(ex[f"pac_{tag}"]), f"decoded_{name}.npz", f"pcm_{tag}"
        gold = np.load(os.path.join(GOLDEN, f"excerpt_vq_{name}.npz"))
        for kbps in (96, 128):
            yield f"{name}_vq{kbps}", bytes(gold[f"pac_vq{kbps}"]), f"decoded_vq_{name}.npz", f"pcm_vq{kbps}"


def test_index_body_on_the_golden_excerpts(A, torch, enc):
    for tag, pac, _, _ in _golden_pacs():
        cp, pos = A.pacfile.parse_header(pac)
        body = pac[pos:]
        want = index_cases.expected(A.pacfile.record_chain, body, cp.nChannels, 1, len(body))
        assert want[2][2] == -1 and want[2][1] == len(body) and want[2][0] > 0
        for lead in range(4):
            assert device_index(A, torch, enc, body, cp.nChannels, 1, len(body) // 5, lead=lead) == want, tag
        # through the wrapper, on the file as it lies on the device (header in front)
        dev = torch.frombuffer(bytearray(pac), dtype=torch.uint8).to(enc.device)
        offs, sizes, result = enc.index_body(dev[pos:], cp.nChannels)
        n = int(result[0])
        assert result.cpu().tolist() == want[2]
        assert offs[:n].cpu().tolist() == want[0] and sizes[:n].cpu().tolist() == want[1]


# ------------------------------------------------------------------ overlap-and-add with a carried tail
def _castanet_blocks(A, torch):
    ex = load_excerpt("castanet")
    pac = bytes(ex["pac_bs"])
    cp, pos = A.pacfile.parse_header(pac)
    e = A.context.encoder_for_params(cp)
    offs, sizes = A.pacfile.record_chain(pac, pos, e.payload_stride)
    body = torch.frombuffer(bytearray(pac) + bytearray(8), dtype=torch.uint8).to(e.device)
    codes = e.unpack(body, torch.tensor(sizes, dtype=torch.int32, device=e.device),
                     torch.tensor(offs, dtype=torch.int64, device=e.device))
    blocks, pcm = e.decode(codes, cp.nChannels, want_blocks=True, want_pcm=True)
    return e, cp.nChannels, blocks, pcm


def test_overlap_add_zero_tail_and_flush_equals_decode(A, torch):
    e, n_ch, blocks, pcm = _castanet_blocks(A, torch)
    tail = torch.zeros((n_ch, 1024), dtype=torch.float64, device=e.device)
    got = e.overlap_add(blocks, tail, True)
    assert got.shape == pcm.shape and torch.equal(got, pcm)
    assert torch.equal(tail, blocks.view(-1, n_ch, 2048)[-1, :, 1024:])
    # no blocks: the tail stays, flush writes it out as one hop
    keep = tail.clone()
    assert e.overlap_add(blocks[:0], tail, False).shape[0] == 0 and torch.equal(tail, keep)
    assert torch.equal(e.overlap_add(blocks[:0], tail, True), pcm[-1024:]) and torch.equal(tail, keep)


def test_overlap_add_split_at_block_boundaries_equals_unsplit(A, torch):
    e, n_ch, blocks, pcm = _castanet_blocks(A, torch)
    n_blocks = blocks.shape[0] // n_ch
    cuts = [0, 1, n_blocks // 3, n_blocks - 2, n_blocks]                  # three boundaries inside the stream
    tail = torch.zeros((n_ch, 1024), dtype=torch.float64, device=e.device)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(e.overlap_add(blocks[a * n_ch:b * n_ch], tail, b == n_blocks))
    assert torch.equal(torch.cat(parts), pcm)


# ------------------------------------------------------------------ whole files in chunks
@pytest.mark.parametrize("item", list(range(16)))
def test_chunked_decode_equals_one_batch_and_the_reference(A, item):
    tag, pac, npz, key = list(_golden_pacs())[item]
    want = np.load(os.path.join(GOLDEN, npz))[key]
    whole = A.pacfile.decode_stream(pac)
    assert np.array_equal(whole, want), tag
    cp, _ = A.pacfile.parse_header(pac)
    smallest = cp.nChannels * (2192 + 4)
    for chunk_bytes, depth, max_blocks in ((smallest, 2, None), (smallest, 3, 3), (50021, 2, None), (50021, 3, 7),
                                           (len(pac) + 1000, 2, None), (len(pac) + 1000, 3, 5)):
        got = A.pacfile.decode_stream(pac, chunk_bytes=chunk_bytes, max_blocks=max_blocks, depth=depth)
        assert got.dtype == np.int16 and got.shape == want.shape, (tag, chunk_bytes, depth, max_blocks)
        assert np.array_equal(got, whole), (tag, chunk_bytes, depth, max_blocks)
        assert np.array_equal(got, want), (tag, chunk_bytes, depth, max_blocks)


def test_chunk_below_one_hop_of_longest_records_is_refused(A):
    pac = bytes(load_excerpt("castanet")["pac_long"])
    with pytest.raises(ValueError):
        A.pacfile.decode_stream(pac, chunk_bytes=2 * 2196 - 1)


def test_full_size_stream_in_chunks_of_one_mebibyte(A):
    """4096 stereo frames at 128 kb/s (the size of test_gpu_decode.py::test_full_size_round_trip)"""
    pcm = A.synth.stream(4096, 2)
    pac = A.pacfile.encode_stream(pcm, 48000, 128)
    whole = A.pacfile.decode_stream(pac)
    assert whole.shape == ((4096 + 3) * 1024, 2)
    got = A.pacfile.decode_stream(pac, chunk_bytes=1 << 20)
    assert np.array_equal(got, whole)
    parts = list(A.pacfile.iter_decode(io.BytesIO(pac), chunk_bytes=1 << 20, max_blocks=500))
    assert len(parts) > 4 and np.array_equal(np.concatenate(parts), whole)


# ------------------------------------------------------------------ malformed input
def _stream_and_pac(A, vq):
    ex = load_excerpt("castanet")
    pcm = ex["pcm"][:24 * 1024]
    return A.pacfile.encode_stream(pcm, int(ex["sr"]), 128, block_switching=True, use_vq=vq, use_sbr=False)


def _prefix_positions(pac, pos):
    out = []
    while pos < len(pac):
        out.append(pos)
        pos += 4 + struct.unpack_from("<L", pac, pos)[0]
    return out


@pytest.mark.parametrize("vq", [False, True])
def test_truncated_and_corrupt_pac_raise_in_chunks(A, torch, vq):
    """the cases of test_gpu_round2.py::test_truncated_and_corrupt_pac_raise through the chunked route, plus cuts
    that fall on a chunk end"""
    pac = _stream_and_pac(A, vq)
    cp, pos = A.pacfile.parse_header(pac)
    smallest = cp.nChannels * 2196
    good = A.pacfile.decode_stream(pac)
    for chunk_bytes in (smallest, 50021):
        assert np.array_equal(A.pacfile.decode_stream(pac, chunk_bytes=chunk_bytes), good)
        for cut in (len(pac) - 1, len(pac) - 200, len(pac) // 2 + 1):
            with pytest.raises(RuntimeError, match="partial block"):
                A.pacfile.decode_stream(pac[:cut], chunk_bytes=chunk_bytes)
        bad = bytearray(pac)
        bad[pos:pos + 4] = (len(pac)).to_bytes(4, "little")                    # a length that points past the file
        with pytest.raises(RuntimeError, match="partial block"):
            A.pacfile.decode_stream(bytes(bad), chunk_bytes=chunk_bytes)
        bad = bytearray(pac)
        first = pos + 4
        assert not ((bad[first] >> 5) & 2), "first block of the excerpt is a long block"
        bits = int.from_bytes(bad[first:first + 4], "big") | (0xFFF << (32 - 7 - 12))   # an impossible allocation
        bad[first:first + 4] = bits.to_bytes(4, "big")
        with pytest.raises(RuntimeError, match="partial block"):
            A.pacfile.decode_stream(bytes(bad), chunk_bytes=chunk_bytes)
    prefixes = _prefix_positions(pac, pos)
    assert len(prefixes) % cp.nChannels == 0
    # the body ends exactly where the first chunk ends, inside a record ...
    inside = next(p for p in prefixes if p - pos >= smallest) + 40
    with pytest.raises(RuntimeError, match="partial block"):
        A.pacfile.decode_stream(pac[:inside], chunk_bytes=inside - pos)
    # ... and inside a prefix
    for k in (1, 2, 3):
        at = next(p for p in prefixes if p - pos >= smallest) + k
        with pytest.raises(RuntimeError, match="partial block"):
            A.pacfile.decode_stream(pac[:at], chunk_bytes=at - pos)
    # a corrupt record in a later chunk: the chunks before it come out first
    later = next(p for p in prefixes if p - pos >= 3 * smallest)
    bad = bytearray(pac)
    bad[later:later + 4] = (0).to_bytes(4, "little")
    it = A.pacfile.iter_decode(bytes(bad), chunk_bytes=smallest)
    first_part = next(it)
    assert np.array_equal(first_part, good[:len(first_part)]) and len(first_part) > 0
    with pytest.raises(RuntimeError, match="partial block"):
        list(it)
    # cut between the channels of a hop: a record count that is not a multiple of the channel count
    odd = prefixes[len(prefixes) - 1]
    with pytest.raises(RuntimeError, match="partial block"):
        A.pacfile.decode_stream(pac[:odd], chunk_bytes=smallest)
    with pytest.raises(RuntimeError, match="partial block"):
        A.pacfile.decode_stream(pac[:odd])
    # cut between two hops: a shorter stream, not an error
    even = prefixes[len(prefixes) - cp.nChannels]
    assert np.array_equal(A.pacfile.decode_stream(pac[:even], chunk_bytes=smallest), A.pacfile.decode_stream(pac[:even]))
    # a header and nothing else
    assert np.array_equal(A.pacfile.decode_stream(pac[:pos], chunk_bytes=smallest), A.pacfile.decode_stream(pac[:pos]))


# ------------------------------------------------------------------ bounded memory
class _RecordingFile(io.BytesIO):
    def __init__(self, data):
        super().__init__(data)
        self.sizes = []

    def read(self, n=-1):
        self.sizes.append(n)
        return super().read(n)


def test_file_object_is_read_in_pieces_of_at_most_one_chunk(A):
    pac = A.pacfile.encode_stream(A.synth.stream(256, 2), 48000, 128)
    whole = A.pacfile.decode_stream(pac)
    chunk_bytes = 20000
    f = _RecordingFile(pac)
    it = A.pacfile.iter_decode(f, chunk_bytes=chunk_bytes)
    parts = [next(it)]
    assert f.tell() <= 200 + 3 * chunk_bytes, "read more than one buffer ahead of the chunk handed out"
    parts += list(it)
    assert np.array_equal(np.concatenate(parts), whole)
    assert len(parts) > 5
    assert all(0 <= n <= chunk_bytes for n in f.sizes), max(f.sizes)


def test_device_memory_does_not_grow_with_the_stream(A, torch):
    from audio_codec_amd.streaming import HostStreamDecoder
    n_hops, chunk_bytes, max_blocks = 96, 24000, 16
    pcm = A.synth.stream(4 * n_hops, 2)
    pacs = [A.pacfile.encode_stream(pcm[:n * 1024], 48000, 128) for n in (n_hops, 4 * n_hops)]
    cp, pos = A.pacfile.parse_header(pacs[0])
    e = A.context.encoder_for_params(cp)
    peaks, chunks = [], []
    for rounds in range(2):                                     # the first pass grows the handle's own workspaces
        peaks, chunks = [], []
        for pac in pacs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            hs = HostStreamDecoder(e, cp.nChannels, chunk_bytes, max_blocks, timing=True)
            assert hs.max_cf == max_blocks * cp.nChannels
            got = np.concatenate([p.copy() for p in hs.decode(A.pacfile._reader(pac[pos:]))])
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated())
            assert np.array_equal(got, A.pacfile.decode_stream(pac))
            records = [n for n, _, _ in hs.timing]
            assert max(records) <= hs.max_cf                    # what the handle's workspaces are sized by
            chunks.append(len(records))
            del hs
    assert chunks[0] >= 4 and chunks[1] >= 4 * chunks[0] - 4
    assert peaks[1] == peaks[0], peaks


def test_two_decodes_side_by_side_do_not_share_buffers(A):
    """two iter_decode generators with the same chunk sizes, advanced in turn"""
    pacs = [A.pacfile.encode_stream(A.synth.stream(n, 2), 48000, 128) for n in (40, 56)]
    whole = [A.pacfile.decode_stream(p) for p in pacs]
    its = [A.pacfile.iter_decode(p, chunk_bytes=8192, max_blocks=6) for p in pacs]
    parts = [[], []]
    live = [0, 1]
    while live:
        for i in list(live):
            try:
                parts[i].append(next(its[i]))
            except StopIteration:
                live.remove(i)
    for i in (0, 1):
        assert len(parts[i]) > 3 and np.array_equal(np.concatenate(parts[i]), whole[i])
