"""CPU check of audio-codec_amd/csrc/body_index.h (the record index behind pacx_index_body): the
header is built for the host with g++ (tests/hostcheck/index_check.cpp runs the three phases with
loops in place of lanes) and compared with the sequential walk, pacfile.record_chain, on every body
of tests/index_cases.py.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import index_cases
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostcheck", "index_check.cpp")
INC = os.path.join(ROOT, "audio-codec_amd", "csrc")


@pytest.fixture(scope="module")
def ixc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("indexcheck") / "libindexcheck.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-I", INC, SRC, "-o", out])
    lib = ctypes.CDLL(out)
    lib.ixc_index_body.restype = ctypes.c_longlong
    lib.ixc_index_body.argtypes = [ctypes.c_char_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    return a


def model_index(ixc, body, n_channels, final, max_records):
    """offsets, sizes, result of the host build; the arrays carry a canary past max_records"""
    offs = np.full(max_records + 2, -7, dtype=np.int64)
    sizes = np.full(max_records + 2, -7, dtype=np.int32)
    result = np.full(3, -99, dtype=np.int64)
    ixc.ixc_index_body(body, len(body), n_channels, final, max_records, offs.ctypes.data, sizes.ctypes.data,
                       result.ctypes.data)
    n = int(result[0])
    assert 0 <= n <= max_records
    assert np.all(offs[n:] == -7) and np.all(sizes[n:] == -7), "wrote past the records it returned"
    return offs[:n].tolist(), sizes[:n].tolist(), result.tolist()


def test_constants_agree_with_the_binding(ixc, A):
    assert ixc.ixc_segment_bytes() == A._lib.INDEX_SEGMENT
    assert ixc.ixc_max_record() == index_cases.MAX_RECORD == 2192


def test_model_equals_the_sequential_walk_on_every_case(ixc, A):
    n_cases = 0
    for name, body, n_ch, final, max_records in index_cases.cases(ixc.ixc_segment_bytes()):
        want = index_cases.expected(A.pacfile.record_chain, body, n_ch, final, max_records)
        got = model_index(ixc, body, n_ch, final, max_records)
        assert got[2] == want[2], (name, got[2], want[2])
        assert got[0] == want[0], name
        assert got[1] == want[1], name
        n_cases += 1
    assert n_cases > 300


def test_random_bodies_with_cuts_and_corruptions(ixc, A):
    """short records of every size class, truncations and single-byte corruptions: the chain the model
    returns is the sequential walk's, whatever the bytes"""
    rng = np.random.default_rng(3)
    for trial in range(400):
        k = int(rng.integers(0, 60))
        body = b"".join(index_cases.rec(int(rng.choice([1, 1, 2, 2192, int(rng.integers(1, 2193))])), rng)
                        for _ in range(k))
        mode = rng.random()
        if mode < 0.3 and len(body) > 3:
            body = body[:int(rng.integers(1, len(body)))]
        elif mode < 0.6 and body:
            b = bytearray(body)
            b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
            body = bytes(b)
        n_ch = int(rng.choice([1, 2, 5]))
        final = int(rng.integers(0, 2))
        max_records = int(rng.choice([k + 5, max(k - 3, 0), 3]))
        want = index_cases.expected(A.pacfile.record_chain, body, n_ch, final, max_records)
        got = model_index(ixc, body, n_ch, final, max_records)
        assert got == (want[0], want[1], want[2]), trial
