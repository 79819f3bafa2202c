"""Bodies for the record index (pacx_index_body, csrc/body_index.h), shared by the CPU model test
(tests/test_index_model.py) and the GPU test (tests/test_gpu_decode_stream.py).  Seeded, no tests here.

cases(segment) yields (name, body, n_channels, final, max_records); expected(record_chain, ...) is the
host walk they are compared with: pacfile.record_chain wrapped to report where it raised, followed by
the limits of the call (max_records, whole frames of n_channels records, final)."""
import re
import struct

import numpy as np

MAX_RECORD = 2192


def rec(n, rng=None, fill=None):
    """one record of n payload bytes: random bytes (not zeros), or `fill` repeated"""
    if fill is not None:
        pay = (fill * (n // len(fill) + 1))[:n]
    else:
        pay = rng.integers(1, 256, n, dtype=np.uint8).tobytes()
    return struct.pack("<L", n) + pay


def _ordinary(rng, n_records):
    return b"".join(rec(int(rng.integers(200, 481)), rng) for _ in range(n_records))


def _prefix_filled(rng, n_records):
    """every payload is a run of valid-looking prefixes ('<L 1..2192' repeated)"""
    out = []
    for _ in range(n_records):
        n = int(rng.integers(40, 600))
        fill = b"".join(struct.pack("<L", int(v)) for v in rng.integers(1, MAX_RECORD + 1, 8))
        out.append(rec(n, fill=fill))
    return b"".join(out)


def _straddle(rng, segment, split):
    """a prefix whose bytes fall `split` before and 4 - split after a segment boundary, then more records"""
    head = b""
    while len(head) < segment - split - 700:
        head += rec(int(rng.integers(200, 481)), rng)
    gap = segment - split - len(head) - 4              # one record that ends exactly `split` bytes before the boundary
    head += rec(gap, rng)
    assert len(head) == segment - split and 1 <= gap <= MAX_RECORD
    return head + _ordinary(rng, 30)


def bases(segment):
    """(name, body) without cuts: the whole-chain shapes"""
    rng = np.random.default_rng(20240611)
    out = [
        ("ordinary", _ordinary(rng, 90)),                                  # several segments
        ("one_byte_records", b"".join(rec(1, rng) for _ in range(2 * segment // 5 + 7))),
        ("max_records", b"".join(rec(MAX_RECORD, rng) for _ in range(12))),
        ("prefix_filled", _prefix_filled(rng, 80)),
        ("mixed_sizes", b"".join(rec(int(rng.choice([1, 1, 2, 5, MAX_RECORD, 300])), rng) for _ in range(300))),
        ("exact_segment", b"".join(rec(segment // 8 - 4, rng) for _ in range(16))),      # ends on a segment boundary
        ("many_segments", _ordinary(rng, 70 * segment // 344)),                           # more than one group of 64
    ]
    assert len(out[5][1]) == 2 * segment and len(out[6][1]) > 64 * segment
    for split in range(4):
        out.append((f"straddle_{split}", _straddle(rng, segment, split)))
    return out


def _replace_len(body, index, value):
    """the length prefix of record `index` on the chain set to `value`"""
    pos = 0
    for _ in range(index):
        pos += 4 + struct.unpack_from("<L", body, pos)[0]
    return body[:pos] + struct.pack("<L", value) + body[pos + 4:]


def cases(segment):
    rng = np.random.default_rng(7)
    all_bases = bases(segment)
    for name, body in all_bases:
        for final in (0, 1):
            yield f"{name}/whole/final{final}", body, 1, final, len(body)
            if name == "many_segments":
                cuts = (1, 3, 6)                                          # a long body: a few cuts are enough
            else:
                cuts = range(1, 9)
            for cut in cuts:                                              # every one of the last 8 bytes
                yield f"{name}/cut{cut}/final{final}", body[:len(body) - cut], 1, final, len(body)
            # inside a prefix: the last record's prefix cut after 1, 2 and 3 bytes
            pos = last = 0
            while pos < len(body):
                last = pos
                pos += 4 + struct.unpack_from("<L", body, pos)[0]
            for k in (1, 2, 3):
                yield f"{name}/prefix_cut{k}/final{final}", body[:last + k], 1, final, len(body)
    small = all_bases[0][1]
    two_seg = all_bases[5][1]
    for value in (0, MAX_RECORD + 1, 0xFFFFFFFF):
        for where, body in (("first", _replace_len(small, 0, value)), ("mid", _replace_len(small, 41, value)),
                            ("last", _replace_len(small, 89, value)), ("segment_start", _replace_len(two_seg, 8, value))):
            for final in (0, 1):
                yield f"bad_len_{value}_on_chain/{where}/final{final}", body, 1, final, len(body)
    # the same values OFF the chain: inside payloads, they mean nothing
    for value in (0, MAX_RECORD + 1):
        body = b"".join(rec(int(rng.integers(200, 481)), fill=struct.pack("<L", value)) for _ in range(60))
        for final in (0, 1):
            yield f"bad_len_{value}_off_chain/final{final}", body, 1, final, len(body)
    # channel counts with a record count that is not a multiple
    for n_ch in (1, 2, 5):
        for n_rec in (5 * 7 + 3, 5 * 12 + 1, 4):
            body = _ordinary(rng, n_rec)
            for final in (0, 1):
                yield f"channels{n_ch}/records{n_rec}/final{final}", body, n_ch, final, len(body)
                yield f"channels{n_ch}/records{n_rec}/cut/final{final}", body[:-5], n_ch, final, len(body)
                yield f"channels{n_ch}/records{n_rec}/max7/final{final}", body, n_ch, final, 7
    # max_records smaller than the chain (and equal, and zero), also in front of an error
    for max_records in (0, 1, 10, 89, 90, 91):
        for final in (0, 1):
            yield f"max_records{max_records}/final{final}", small, 1, final, max_records
            yield f"max_records{max_records}/two_channels/final{final}", small, 2, final, max_records
    yield "max_records_before_error", _replace_len(small, 41, 0), 1, 1, 41
    yield "max_records_after_error", _replace_len(small, 41, 0), 1, 1, 42
    for final in (0, 1):
        yield f"empty/final{final}", b"", 1, final, 4
        yield f"empty/two_channels/final{final}", b"", 2, final, 0
        for n in (1, 2, 3, 4, 5):
            yield f"tiny{n}/final{final}", struct.pack("<L", 1)[:n] + b"\x07"[:max(0, n - 4)], 1, final, 4


def host_walk(record_chain, body):
    """record_chain(body, 0, MAX_RECORD) made to report where it raised:
    -> (offsets, sizes, position of the first prefix not walked, 'end' | 'bad' | 'incomplete')"""
    try:
        offs, sizes = record_chain(body, 0, MAX_RECORD)
        return offs, sizes, len(body), "end"
    except RuntimeError as e:
        m = re.search(r"at offset (\d+)", str(e))
        if m:
            at = int(m.group(1))
        else:                                          # a prefix cut short: it starts in the last three bytes
            at = next(len(body) - k for k in (1, 2, 3) if _walks(record_chain, body[:len(body) - k]))
    offs, sizes = record_chain(body[:at], 0, MAX_RECORD)          # the records before it
    n = struct.unpack_from("<L", body, at)[0] if at + 4 <= len(body) else None
    kind = "incomplete" if n is None or 1 <= n <= MAX_RECORD else "bad"
    return offs, sizes, at, kind


def _walks(record_chain, body):
    try:
        record_chain(body, 0, MAX_RECORD)
        return True
    except RuntimeError:
        return False


def expected(record_chain, body, n_channels, final, max_records):
    """-> (offsets, sizes, [records returned, bytes consumed, error position or -1])"""
    offs, sizes, at, kind = host_walk(record_chain, body)
    error_at = -1
    n = len(offs)
    if n >= max_records:
        n = max_records                                # the walk stops here, whatever follows
    elif kind == "bad" or (kind == "incomplete" and final):
        error_at = at
    n -= n % n_channels
    consumed = at if n == len(offs) else offs[n] - 4
    return offs[:n], sizes[:n], [n, consumed, error_at]
