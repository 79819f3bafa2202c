"""Writes tests/golden/vq_code_streams.npz: what the REFERENCE's own reader and decoder make of four of the drawn
gain-shape streams of tests/vq_code_streams.py -- records no encoder writes from audio (negative gains, angle index 0
throughout, omitted bands coded one by one).

Only runs in the build container (needs /root/reference).  Nothing of the reference is copied: its PACFile reader and
PCMFile writer are imported and run on the bytes of vq_code_streams.fixture_case(name) -- the cases `mixed`,
`gain_edges`, `theta_zero` and `sbr_partial` drawn with no leaf above K = 4096, because the reference's codebook layer
is linear in K -- and the int16 PCM it writes is stored, or the class name of the exception where it raises:

    pcm_<case>  int16 [n, nCh]      error_<case>  str ('' where it finished)      crc_<case>  crc32 of the .pac bytes

Run from the repository root:  python tests/golden/make_vq_code_streams.py   (about a minute)
tests/test_vq_code_streams.py asserts that the oracle with pvq_model's leaves gives that PCM sample for sample.
"""
import os
import sys
import tempfile
import time
import zlib

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import vq_code_streams as vs       # noqa: E402

np.int = int      # noqa  (the reference predates NumPy 1.24)
np.float = float  # noqa
_work = tempfile.mkdtemp(prefix="pacref_vqcs_")
os.chdir(_work)
sys.path.insert(0, os.path.join(REF, "coder"))

import bitpack      # noqa: E402
import pacfile      # noqa: E402
import pcmfile      # noqa: E402

FIXTURE = os.path.join(HERE, "vq_code_streams.npz")


def ref_decode(pac_bytes, tag):
    """the reference's decode loop (coder/pacfile.py:745-757) on the bytes -> int16 [n, nCh].  Shim as in
    make_golden.py: PackedBits keeps `bytes` (NumPy-2 uint8 overflow in ReadBits)"""
    def keep_bytes(self, data):
        self.nBytes = len(data)
        self.data = bytes(data)
    bitpack.PackedBits.SetPackedData = keep_bytes
    pac_path, wav_path = os.path.join(_work, tag + ".pac"), os.path.join(_work, tag + ".wav")
    open(pac_path, "wb").write(pac_bytes)
    src = pacfile.PACFile(pac_path)
    dst = pcmfile.PCMFile(wav_path)
    cp = src.OpenForReading()
    cp.bitsPerSample = 16
    dst.OpenForWriting(cp)
    while True:
        data = src.ReadDataBlock(cp)
        if not data:
            break
        dst.WriteDataBlock(data, cp)
    src.Close(cp)
    dst.Close(cp)
    raw = open(wav_path, "rb").read()
    return np.frombuffer(raw[44:], dtype="<i2").reshape(-1, cp.nChannels).copy()


def main():
    sys.setrecursionlimit(12000)                         # the reference's N(L, K) recurses over L + K, as in make_golden.py
    out = {}
    for name in vs.FIXTURE_CASES:
        t0 = time.time()
        c = vs.fixture_case(name)
        out["crc_" + name] = np.uint32(zlib.crc32(c.pac))
        try:
            pcm = ref_decode(c.pac, name)
            err = ""
        except Exception as e:                           # recorded, not hidden: the test asserts the class name
            pcm = np.zeros((0, c.n_ch), np.int16)
            err = type(e).__name__
            print(name, "raises", err, e)
        out["pcm_" + name] = pcm
        out["error_" + name] = np.array(err)
        print(f"{name}: {pcm.shape} {err!r} {time.time() - t0:.1f} s")
    np.savez_compressed(FIXTURE, **out)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
