"""The NumPy statement of the gain-shape band curve (tests/vq_band_model.py) and its fixture
(tests/golden/vq_band.npz, written by tests/golden/make_vq_band.py), on the CPU.

  - two units of the fixture, a long block and a short sub-block, recomputed from the model: integers equal, NMRs
    within 1e-9 dB (the same NumPy arithmetic; the bar allows another build's log10 its last place);
  - every band that is not all zero writes exactly a x lines bits at every size (what makes the scalar length formula
    the gain-shape record's), an all-zero band writes nothing, holds -inf and gets allocation 0;
  - the record lengths predicted from the curve (band_model's pick) are the ones the model encoder writes;
  - the library exports the two new entry points and its ABI is still 7.
"""
import os
import re

import numpy as np

import band_model as bm
import nmr_model as nm
import rate_model as rm
import vq_band_model as vm
from oracle import pac_oracle_vq as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("pacx_vq_band_curve_batch", "pacx_encode_vq_alloc_batch")
RECOMPUTED = ((0, 0), (2, 3))                # (cf, sb): block 0 is long-coded, block 1 (cf 2, 3) short-coded

_A = {}


def analysis():
    if not _A:
        pcm, sr = vm.fixture_stream()
        _A["a"] = rm.analysis(pcm, sr, True)
        _A["pcm"] = pcm
    return _A["a"]


def test_fixture_shape_and_rules():
    F = vm.load_fixture()
    a = analysis()
    cur = [bool(f[1]) for f in a["flags"]]
    assert len(cur) == 6 and any(cur) and not all(cur) and not any(a["dropped"])
    assert os.path.getsize(vm.FIXTURE) < 100_000
    unit, lines = bm.layout(F)
    live = unit >= 0
    n_cand = F["n_cand"]
    assert F["nmr"].shape == (12, F["band_stride"], 16) and n_cand == 16
    assert np.isnan(F["nmr"][~live]).all() and not np.isnan(F["nmr"][live]).any()
    short = F["cap"][:, 1] >= 0
    assert np.array_equal(short, np.repeat(cur, 2))
    assert (F["cap"][~short, 1:] == -1).all() and (F["cap"][:, 0] >= 0).all()
    # bits written: a x lines for every band that is not all zero, at every size; nothing for candidate 0
    zero = np.isneginf(F["nmr"][:, :, 1]) & live
    want = bm.BITS[None, None, :] * lines[:, :, None]
    assert np.array_equal(F["written"][live & ~zero], want[live & ~zero])
    assert not F["written"][zero].any() and not F["written"][~live].any()
    assert np.isneginf(F["nmr"][zero]).all() and not F["cap_alloc"][zero].any()
    assert np.isfinite(F["nmr"][live & ~zero]).all()             # no candidate at which the oracle fails on this stream
    assert not F["cap_alloc"][~live].any()
    # the noise falls by tens of dB over the sizes, though not monotonically
    fall = F["nmr"][live & ~zero][:, 1] - F["nmr"][live & ~zero][:, 15]
    assert fall.min() > 20.0, fall.min()


def test_two_units_recomputed():
    F = vm.load_fixture()
    a = analysis()
    c = vm.curve(a, vm.CAP_KBPS, only=set(RECOMPUTED))
    assert not a["flags"][0][1] and a["flags"][1][1]
    for cf, sb in RECOMPUTED:
        nb = len(F["lines_short"]) if F["cap"][cf, 1] >= 0 else len(F["lines_long"])
        at = slice(sb * nb, (sb + 1) * nb)
        assert c["cap"][cf, sb] == F["cap"][cf, sb] >= 0
        assert np.array_equal(c["cap_alloc"][cf, at], F["cap_alloc"][cf, at])
        assert np.array_equal(c["written"][cf, at], F["written"][cf, at])
        fin = np.isfinite(F["nmr"][cf, at])
        assert np.array_equal(np.isfinite(c["nmr"][cf, at]), fin)
        assert np.array_equal(c["nmr"][cf, at][~fin], F["nmr"][cf, at][~fin])
        assert np.abs(c["nmr"][cf, at][fin] - F["nmr"][cf, at][fin]).max() <= 1e-9


def test_predicted_lengths_are_the_encoders():
    """pick on the fixture's curve -> the model encoder writes records of exactly the predicted lengths, at a target
    that caps nothing and at one so low that units go over their cap and take cap_alloc"""
    F = vm.load_fixture()
    a = analysis()
    for target in (-3.0, -60.0):
        _, alloc, n_bytes, capped = bm.evaluate(F, int(target * bm.GRID))
        assert capped.any() == (target == -60.0)
        data, final, written = vm.encode_stream_alloc(a, alloc, len(_A["pcm"]))
        assert np.array_equal(written, n_bytes)
        recs, (sr, n_ch, use_sbr, use_vq) = nm.records(data)
        assert use_vq and not use_sbr and np.array_equal([n for _, n in recs], n_bytes)
        assert recs[-1][0] + recs[-1][1] == len(data)
        unit, _ = bm.layout(F)
        zero = np.isneginf(F["nmr"][:, :, 1]) & (unit >= 0)
        assert np.array_equal(final[~zero], alloc[~zero]) and not final[zero].any()
        pcm = pv.decode_stream_vq(data)                         # every record parses; the oracle decodes the stream
        assert pcm.shape == (len(_A["pcm"]) + 3 * 1024, 2)


def test_silence_codes_nothing():
    """digital silence: every band all zero -> -inf everywhere, cap_alloc 0, and any allocation codes to the minimum"""
    pcm = np.zeros((1024, 1), np.int16)
    a = rm.analysis(pcm, 48000, False)
    c = vm.curve(a, vm.CAP_KBPS)
    unit, _ = bm.layout(c)
    live = unit >= 0
    assert live.any() and np.isneginf(c["nmr"][live]).all() and not c["cap_alloc"].any() and not c["written"].any()
    _, alloc, n_bytes, capped = bm.evaluate(c, 0)
    assert not alloc.any() and not capped.any()
    nb = len(c["lines_long"])
    least = (4 + nb * (12 + 4) + 4 + 7) >> 3
    assert (n_bytes == least).all()
    data, final, written = vm.encode_stream_alloc(a, np.full_like(alloc, 9), len(pcm))
    assert not final.any() and (written == least).all()


def test_library_exports_the_entry_points():
    """fails on a tree without the feature"""
    import audio_codec_amd as a
    lib = a.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pacx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in pacx.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in a._lib.SIGNATURES, name
    assert lib.pacx_abi_version() == 7                 # additive: no caller breaks
    for name in ("vq_band_curve", "encode_vq_alloc"):
        assert hasattr(a.engine.Encoder, name)
    for mod, names in ((a.pacfile, ("encode_stream_vq_nmr", "encode_stream_vq_abr")),
                       (a.quality, ("encode_stream_vq_to_nmr", "encode_stream_vq_to_rate"))):
        for name in names:
            assert callable(getattr(mod, name))


def test_vq_band_kernels_use_no_scratch():
    """the compiler's resource report of the new kernels: no scratch, no spilled registers"""
    import importlib
    res = importlib.import_module("audio_codec_amd.build").resources()
    mine = {k: v for k, v in res.items() if v["source"] == "k_vq_band.hip"}
    want = {"k_vq_band_cap", "k_vq_band_fill", "k_vq_band_store", "k_vq_band_zero"}
    assert {n for n in want if any(n in k for k in mine)} == want
    for name, r in mine.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
