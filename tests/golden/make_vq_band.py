"""Writes tests/golden/vq_band.npz: the gain-shape band curve of tests/vq_band_model.py for one small stream.

The model codes every band of every unit at every size through the oracle's gain-shape coder and decoder in NumPy --
about 2.6 s for a long unit -- so the curve of the test stream is computed once, here, and committed:

    stream   vq_band_model.STREAM: 4 hops of a golden excerpt with block switching, stereo -> the 6 blocks the driver
             writes, 12 channel-frames, of which at least one is short-coded and one long-coded and none is dropped
    nmr      float64 [12, band_stride, 16]     cap  int32 [12, 8]     cap_alloc  int32 [12, band_stride]
    written  int64 [12, band_stride, 16]: the bits every band wrote at every size (a.lines, or 0 for an all-zero band)

Run from the repository root:  python tests/golden/make_vq_band.py   (about half a minute)
tests/test_vq_band_model.py recomputes two units of it and checks the rest of its properties.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rate_model as rm            # noqa: E402
import vq_band_model as vm         # noqa: E402


def main():
    t0 = time.time()
    pcm, sr = vm.fixture_stream()
    a = rm.analysis(pcm, sr, True)
    cur = [bool(f[1]) for f in a["flags"]]
    assert len(cur) == 6 and any(cur) and not all(cur) and not any(a["dropped"]), (cur, a["dropped"])
    c = vm.curve(a, vm.CAP_KBPS)
    np.savez_compressed(vm.FIXTURE, excerpt=vm.STREAM[0], stream=np.array(vm.STREAM[1:]), cap_kbps=vm.CAP_KBPS,
                        nmr=c["nmr"], cap=c["cap"], cap_alloc=c["cap_alloc"], written=c["written"])
    print(f"{vm.FIXTURE}: {os.path.getsize(vm.FIXTURE)} bytes, flags {a['flags']}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
