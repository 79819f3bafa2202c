"""Writes tests/golden/widths.part*.npz: the REFERENCE's own encoder and decoder at field widths other than
nScaleBits = 4 / nMantSizeBits = 12, on the six-hop stream and the cases of tests/widths_cases.py.

Only runs in the build container (needs /root/reference).  Nothing of the reference is copied: its PCMFile -> PACFile
loop and its decoder are imported and run as tests/golden/make_golden.py runs them, with the two widths set on its
CodingParams, and the bytes and int16 PCM it writes are stored (the layout is in tests/widths_cases.py).  Every case is
checked for what makes it worth having (widths_cases.check_case) before anything is written.

Also stored: vq_band_model.curve of the first two hops at 4 / 3 (this project's NumPy model over the oracle), which
tests/test_gpu_widths.py compares the GPU's gain-shape band curve with.

Run from the repository root:  python tests/golden/make_widths.py           (about half a minute)
                               python tests/golden/make_widths.py --check   (the same work, compared with the committed
                                                                             arrays instead of written)
"""
import importlib.util
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
import widths_cases as wc          # noqa: E402

_argv, sys.argv = sys.argv, sys.argv[:1]
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)       # imports the reference with make_golden.py's shims and a writable working directory
sys.argv = _argv


def ref_encode(wav, case, block_switching, out_path, widths=None):
    """make_golden.ref_encode_file's loop with the widths of the case on the reference's CodingParams"""
    coder, ns, nm, kbps = case
    ns, nm = (ns, nm) if widths is None else widths
    src = mg.pcmfile.PCMFile(wav)
    dst = mg.pacfile.PACFile(out_path)
    cp = src.OpenForReading()
    cp.nMDCTLines = cp.nSamplesPerBlock = 1024
    cp.nScaleBits, cp.nMantSizeBits = ns, nm
    cp.targetBitsPerSample = kbps / (cp.sampleRate / 1000)
    cp.useVQ, cp.useSBR = wc.is_vq(case), wc.uses_sbr(case)
    dst.OpenForWriting(cp)
    look = np.zeros((cp.nChannels, 2048))
    cur = last = False
    flags = []
    while True:
        data = src.ReadDataBlock(cp)
        if not data:
            nxt = False
        else:
            look = np.concatenate((np.copy(data), look[:, 1024:]), axis=1)
            nxt = mg.parTransientDetect(look) if block_switching else False
        flags.append((int(bool(last)), int(bool(cur)), int(bool(nxt))))
        dst.WriteDataBlock(look[:, :1024], cp, lastTrans=last, curTrans=cur, nextTrans=nxt)
        last, cur = cur, nxt
        if not data:
            break
    src.Close(cp)
    dst.Close(cp)
    return open(out_path, "rb").read(), flags


def vq_curve():
    import rate_model as rm
    import vq_band_model as vm
    pcm, sr = wc.stream()
    a = rm.analysis(pcm[:wc.VQ_CURVE["hops"] * 1024], sr, True, *wc.VQ_CURVE["widths"])
    assert any(f[1] for f in a["flags"]) and not all(f[1] for f in a["flags"]) and not any(a["dropped"])
    c = vm.curve(a, wc.VQ_CURVE["cap_kbps"])
    return {"vqcurve_nmr": c["nmr"], "vqcurve_cap": c["cap"], "vqcurve_cap_alloc": c["cap_alloc"],
            "vqcurve_written": c["written"]}


def main():
    sys.setrecursionlimit(12000)                         # the reference's N(L, K) recurses over L + K
    t0 = time.time()
    pcm, sr = wc.stream()
    wav = os.path.join(mg._work, "widths.wav")
    open(wav, "wb").write(mg.wav_bytes(sr, pcm))
    out = {"pcm": pcm, "sr": np.array(sr), "cases": np.array([wc.tag_of(c) for c in wc.CASES])}
    for case in wc.CASES:
        tag = wc.tag_of(case)
        t1 = time.time()
        pac_path = os.path.join(mg._work, tag + ".pac")
        pac, flags = ref_encode(wav, case, True, pac_path)
        dec = mg.ref_decode_file(pac_path, os.path.join(mg._work, tag + "_dec.wav"))
        base_key = "base_%s_%d" % (case[0], case[3])
        if base_key not in out:
            base, _ = ref_encode(wav, case, True, os.path.join(mg._work, base_key + ".pac"), widths=(4, 12))
            out[base_key] = np.frombuffer(base, dtype=np.uint8)
        assert flags == wc.FLAGS, flags
        wc.check_case(case, pac, bytes(out[base_key]), flags)
        out["pac_bs_" + tag] = np.frombuffer(pac, dtype=np.uint8)
        out["dec_bs_" + tag] = dec.astype(np.int16)
        out["flags_" + tag] = np.array(flags, dtype=np.uint8)
        if not wc.is_vq(case):
            long_pac, long_flags = ref_encode(wav, case, False, os.path.join(mg._work, tag + "_long.pac"))
            assert not np.any(long_flags)
            out["pac_long_" + tag] = np.frombuffer(long_pac, dtype=np.uint8)
        print(f"{tag}: {len(pac)} bytes, decoded {dec.shape}, {time.time() - t1:.1f} s", flush=True)
    out.update(vq_curve())
    if "--check" in sys.argv:
        have = golden_io.load_npz("widths")
        assert sorted(have) == sorted(out), (sorted(have), sorted(out))
        for k, v in out.items():
            assert np.asarray(v).dtype == have[k].dtype and np.array_equal(v, have[k], equal_nan=v.dtype.kind == "f"), k
        print(f"widths: {len(out)} arrays equal to the committed ones, {time.time() - t0:.0f} s")
        return
    golden_io.save_npz("widths", out)
    sizes = [os.path.getsize(p) for p in golden_io.part_paths("widths")]
    print(f"widths: {sizes} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
