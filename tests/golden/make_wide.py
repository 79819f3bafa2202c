"""Writes tests/golden/wide.part*.npz: the oracle's streams, decoded PCM and transient decisions for the ten cases of
tests/wide_cases.py (4 to 8 channels, 64 to 192 kHz), and the rate-control models' arrays for the four cases of
wide_cases.RATE_CONTROL.  The layout is in tests/wide_cases.py.

NumPy and the oracle only: it runs wherever the CPU tests run.  Every case is checked for what makes it worth having
(tests/test_wide_cases.check_case) before anything is written; tests/test_wide_cases.py makes two of the cases again
and compares.

Run from the repository root:  python tests/golden/make_wide.py           (about two minutes)
                               python tests/golden/make_wide.py --check   (the same work, compared with the committed
                                                                           arrays instead of written)
"""
import os
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import golden_io                   # noqa: E402
import wide_cases as wc            # noqa: E402


def main():
    sys.setrecursionlimit(12000)                         # the reference's N(L, K) recurses over L + K
    t0 = time.time()
    out = {"cases": np.array([wc.tag_of(c) for c in wc.CASES])}
    for case in wc.CASES:
        t1 = time.time()
        arrays = wc.case_arrays(case)
        out.update(arrays)
        print(f"{wc.tag_of(case)}: {sum(a.nbytes for a in arrays.values())} bytes, {time.time() - t1:.1f} s", flush=True)
    for case in wc.RATE_CONTROL:
        t1 = time.time()
        arrays = {f"{k}_{wc.tag_of(case)}": v for k, v in wc.rate_arrays(case).items()}
        out.update(arrays)
        print(f"{wc.tag_of(case)} models: {sum(a.nbytes for a in arrays.values())} bytes, {time.time() - t1:.1f} s",
              flush=True)
    wc._fixture = out                                    # the checks read the arrays just made
    import test_wide_cases as tw
    for case in wc.CASES:
        tw.check_case(case)
    for case in wc.RATE_CONTROL:
        tw.check_rate_case(case)
    if "--check" in sys.argv:
        have = golden_io.load_npz(wc.FIXTURE)
        assert sorted(have) == sorted(out), (sorted(have), sorted(out))
        for k, v in out.items():
            v = np.asarray(v)
            assert v.dtype == have[k].dtype and np.array_equal(v, have[k], equal_nan=v.dtype.kind == "f"), k
        print(f"wide: {len(out)} arrays equal to the committed ones, {time.time() - t0:.0f} s")
        return
    golden_io.save_npz(wc.FIXTURE, out)
    sizes = [os.path.getsize(p) for p in golden_io.part_paths(wc.FIXTURE)]
    print(f"wide: {len(out)} arrays, {sizes} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
