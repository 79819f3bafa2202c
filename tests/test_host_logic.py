"""CPU checks of the host side: the C-ABI library loads and exports every symbol
include/pacx.h declares (no compute calls: no GPU here), the product fails
loudly without a GPU, and the host-side glue (band tables, flags, WAV contract,
header) agrees with the oracle / golden fixtures."""
import os
import re
import struct

import numpy as np
import pytest

from conftest import EXCERPTS, ROOT, load_excerpt
from oracle import pac_oracle as po


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    if not os.path.exists(a._lib.LIB_PATH):
        import importlib
        importlib.import_module("audio_codec_amd.build").build(verbose=False)
    return a


def test_library_exports_every_declared_symbol(A):
    lib = A.load()
    header = open(os.path.join(ROOT, "include", "pacx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 19
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in pacx.h but not exported"
    assert set(A._lib.SIGNATURES) == declared
    assert lib.pacx_abi_version() == A._lib.PACX_ABI_VERSION == 7


def test_no_cpu_fallback(A):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(A.PacxError):
        A.engine.Encoder(48000, 128 / 48.0)
    with pytest.raises(A.PacxError):
        A.quantize.ScaleFactor(0.5)


def test_product_does_not_import_oracle():
    """Nothing under audio-codec_amd/ (nor the import alias) may import, load or
    execute anything under oracle/ (comments may mention it)."""
    pkg = os.path.join(ROOT, "audio-codec_amd")
    bad = re.compile(r"(^|\n)\s*(import|from)\s+[\w.]*oracle|pac_oracle|oracle[/\\]|oracle\.")
    paths = [os.path.join(ROOT, "audio_codec_amd.py")]
    for dirpath, _, files in os.walk(pkg):
        paths += [os.path.join(dirpath, f) for f in files if f.endswith((".py", ".hip", ".h", ".cpp"))]
    for path in paths:
        assert not bad.search(open(path, errors="ignore").read()), path
    # development aids and the C example stay clear of it too
    for sub in ("tools", "examples"):
        for f in os.listdir(os.path.join(ROOT, sub)):
            if f.endswith((".py", ".c", ".cpp")):
                path = os.path.join(ROOT, sub, f)
                assert not bad.search(open(path, errors="ignore").read()), path
    # bench.py: the oracle only as the CPU baseline and as the checker of the timed run's
    # output (outside the timed regions) -- never inside main()'s timing code
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    allowed = {"_cpu_worker", "cpu_baseline", "cpu_baseline_bs", "verify_against_oracle"}
    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        for node in ast.walk(fn):
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                names = [a.name for a in node.names] + [getattr(node, "module", "") or ""]
                if any("oracle" in n for n in names):
                    assert fn.name in allowed, f"bench.py: oracle imported in {fn.name}()"
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not any("oracle" in (getattr(n, "module", "") or "") or any("oracle" in a.name for a in n.names) for n in top)


@pytest.mark.parametrize("sr", [48000, 44100, 32000, 96000, 22050])
@pytest.mark.parametrize("n", [1024, 128, 512])
def test_default_bands_in_c(A, sr, n):
    """pacx_default_bands (the band layout for hosts without NumPy) against the oracle's
    AssignMDCTLinesFromFreqLimits + ScaleFactorBands; runs on the CPU (no handle)."""
    import ctypes
    lib = A.load()
    out = (ctypes.c_int32 * 25)()
    nb = ctypes.c_int32(0)
    assert lib.pacx_default_bands(sr, n, out, ctypes.byref(nb)) == 0
    try:
        want = po.band_table(n, sr).nLines.tolist()
    except Exception:
        pytest.skip("the reference's ScaleFactorBands fails for this rate / size")
    assert list(out[:nb.value]) == want


def test_record_chain_rejects_truncated_and_oversized(A):
    """decode side: sizes read from a file are checked before anything reaches the GPU
    (coder/pacfile.py:200-205 raises on a short read)."""
    import struct as st
    rec = lambda n: st.pack("<L", n) + bytes(n)
    good = rec(10) + rec(300) + rec(1)
    offs, sizes = A.pacfile.record_chain(good, 0, 2192)
    assert sizes == [10, 300, 1] and offs == [4, 18, 322]
    for bad in (good[:-1], good + b"\x01\x02", rec(10) + st.pack("<L", 5000) + bytes(5000),
                rec(10) + st.pack("<L", 0), good[:16]):
        with pytest.raises(RuntimeError, match="partial block"):
            A.pacfile.record_chain(bad, 0, 2192)


@pytest.mark.parametrize("sr", [48000, 44100])
def test_band_tables_match_golden(A, tables, sr):
    for n in (1024, 128):
        b = A.psychoac.ScaleFactorBands(A.psychoac.AssignMDCTLinesFromFreqLimits(n, sr))
        assert b.nLines.tolist() == tables[f"bands_{n}_{sr}_nLines"].tolist()
        assert b.lowerLine.tolist() == tables[f"bands_{n}_{sr}_lower"].tolist()
        assert b.upperLine.tolist() == tables[f"bands_{n}_{sr}_upper"].tolist()
        f = A.tables.line_freqs(n, sr)
        assert np.array_equal(A.tables.bark(f), tables[f"bark_{n}_{sr}"])
        assert np.array_equal(A.tables.thresh(f), tables[f"thresh_{n}_{sr}"])


def test_window_tables_match_golden(A, tables):
    w = A.tables.long_windows(2048)
    for k, name in enumerate(("sine", "start", "stop", "startstop")):
        assert np.array_equal(w[k], tables[f"win_{name}_2048"])
    assert np.array_equal(A.tables.sine(256), tables["win_sine_256"])
    assert np.array_equal(A.tables.hann(2048), tables["win_hann_2048"])
    assert np.array_equal(A.tables.hann(256), tables["win_hann_256"])
    assert A.tables.fft_norm(2048) == 4 / (2048 ** 2 * np.mean(np.hanning(2048) ** 2))
    assert np.array_equal(A.tables.fft_freq_step(2048, 44100) * np.arange(1025),
                          np.fft.rfftfreq(2048, d=1 / 44100))


def test_pcm_fraction_contract(A, tables):
    got = A.pcmfile.codes_to_fraction(np.arange(-32768, 32768))
    assert np.array_equal(got, tables["pcm_all_fraction"])
    assert np.array_equal(np.signbit(got), np.signbit(tables["pcm_all_fraction"]))


def test_wav_effective_stream_and_header(A, tmp_path):
    """The reference keeps reading past the data chunk (PCMFile shares the
    numSamples that PACFile's header writer inflates); a WAV with a trailing
    chunk exercises it."""
    rng = np.random.default_rng(1)
    pcm = rng.integers(-3000, 3000, (5 * 1024 + 700, 2)).astype("<i2")
    data = pcm.tobytes()
    tail = b"LIST" + struct.pack("<L", 26) + b"INFOISFT" + struct.pack("<L", 14) + b"Lavf58.29.100\0"
    raw = struct.pack("<4sL4s4sLHHLLHH4sL", b"RIFF", 36 + len(data) + len(tail), b"WAVE", b"fmt ", 16, 1, 2,
                      44100, 44100 * 4, 4, 16, b"data", len(data)) + data + tail
    path = tmp_path / "t.wav"
    path.write_bytes(raw)
    sr, eff, declared = A.pcmfile.wav_effective_stream(str(path))
    sr2, eff2, declared2 = po.wav_effective_stream(raw)
    assert (sr, declared) == (sr2, declared2) == (44100, len(pcm))
    assert np.array_equal(eff, eff2)
    assert len(eff) == 6 * 1024 and np.array_equal(eff[:len(pcm)], pcm)
    assert eff[len(pcm):].any()                       # the LIST chunk became samples
    cp = A.audiofile.CodingParams()
    cp.sampleRate, cp.nChannels, cp.numSamples = 44100, 2, declared
    cp.nMDCTLines, cp.nScaleBits, cp.nMantSizeBits = 1024, 4, 12
    cp.useSBR = cp.useVQ = False
    assert A.pacfile.header_bytes(cp) == po.pac_header(po.make_params(44100, 2, 128), declared)
    # PCMFile.ReadDataBlock hands out the reference's fractions
    f = A.pcmfile.PCMFile(str(path))
    p = f.OpenForReading()
    p.nSamplesPerBlock = 1024
    blk = f.ReadDataBlock(p)
    assert np.array_equal(blk[1], po.pcm16_to_fraction(pcm[:1024, 1]))


def test_synth_stream_is_deterministic(A, stages):
    a = A.synth.stream(6, 2)
    tags = [str(t) for t in stages["long_tag"]]
    i = tags.index("synth:h2:c1")
    assert np.array_equal(a[1024:3072, 1], stages["long_x_i16"][i])


def _functions_calling(src, ident):
    """names of the top-level functions of a C++ source whose bodies mention `ident` (comments stripped)"""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names, depth, head_start, name = set(), 0, 0, None
    for m in re.finditer(r"[{};]|\b%s\b" % ident, src):
        t = m.group()
        if t == "{":
            if depth == 0:
                head = src[head_start:m.start()].rstrip()
                # the identifier in front of the parameter list (the '(' that matches the last ')')
                i, d = len(head) - 1, 0
                while i >= 0:
                    d += {")": 1, "(": -1}.get(head[i], 0)
                    if d == 0 and head[i] == "(":
                        break
                    i -= 1
                found = re.search(r"(\w+)\s*$", head[:i]) if head.endswith(")") else None
                name = found.group(1) if found else head
            depth += 1
        elif t == "}":
            depth -= 1
            if depth == 0:
                head_start = m.end()
        elif t == ";":
            if depth == 0:
                head_start = m.end()
        else:
            names.add(name if depth else "<file scope>")
    return names


def test_environment_is_read_in_one_function():
    """the library reads its environment in ONE function (the path overrides, once per handle in pacx_create):
    a getenv anywhere else in csrc/ -- a per-call read on an encode path, say -- fails here"""
    csrc = os.path.join(ROOT, "audio-codec_amd", "csrc")
    where = set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".cpp")):
            where |= {(f, n) for n in _functions_calling(open(os.path.join(csrc, f)).read(), "getenv")}
    assert len(where) == 1, sorted(where)
    # the scanner itself: a second function with a read, and a read at file scope, are told apart
    assert _functions_calling("static int a(int x)\n{\n    return getenv(\"A\") != 0;\n}\n"
                              "__global__ __launch_bounds__(64) void b(int *p) { if (1) { p[0] = getenv(\"B\"); } }\n"
                              "static const char *c = getenv(\"C\");\n", "getenv") == {"a", "b", "<file scope>"}
