"""CPU checks of the constant-quality mode: the C ABI carries its two entry points, and the NumPy statement of the
budget search (tests/rate_model.py), which the GPU tests compare against, is consistent with itself."""
import os
import re

import numpy as np
import pytest

import nmr_model as nm
import rate_model as rm
from conftest import ROOT, load_excerpt
from oracle import pac_oracle as po

NEW = ("pacx_encode_pack_nmr_batch", "pacx_encode_pack_budget_batch")


def test_abi_has_the_two_entry_points():
    import audio_codec_amd as A
    lib = A.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pacx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pacx_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in pacx.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in A._lib.SIGNATURES
    assert "PACX_ST_RATE_CAP" in header and A._lib.ST_RATE_CAP == 128 and A._lib.RATE_STEP == rm.STEP == 32
    assert lib.pacx_abi_version() == 7                 # additive: no caller breaks


@pytest.fixture(scope="module")
def cut():
    """6 hops of castanet's attack, stereo, block switching on: long, start / stop and short-coded blocks"""
    ex = load_excerpt("castanet")
    pcm = ex["pcm"][24 * 1024:30 * 1024]
    assert pcm.shape[1] == 2
    return pcm, int(ex["sr"]), rm.analysis(pcm, int(ex["sr"]), True)


def units_of(a):
    for row in a["units"]:
        if row is not None:
            for us in row:
                yield from us


def test_search_is_consistent(cut):
    """every uncapped unit passes ok at its budget and failed at the last budget the bisection tried below it"""
    _, _, a = cut
    assert any(u.short for u in units_of(a)) and any(not u.short for u in units_of(a))
    n_path = 0
    for target in (0.0, -6.0):
        for u in units_of(a):
            trace = []
            budget, capped, margin = rm.search_unit(a, u, target, 320, trace)
            j = rm.cap_steps(a, u, 320)
            assert trace[0][0] == rm.STEP * j and budget % rm.STEP == 0 and 0 <= budget <= rm.STEP * j
            assert len(trace) <= 1 + int(np.ceil(np.log2(j + 1)))
            assert margin == min(abs(w - target) for _, w in trace)
            assert not capped                          # 320 kb/s is never reached on this material
            assert rm.worst_nmr(a["p"], u, budget) <= target
            below = [(b, w) for b, w in trace if b < budget]
            if below:                                  # the bisection's path below the result ends in a failure
                b, w = max(below)
                assert w > target and b == max(bb for bb, _ in trace if bb < budget)
                n_path += 1
            else:
                assert budget == 0
    assert n_path > 0


def test_cap_path(cut):
    """48 kb/s at -6 dB: units miss the target with the whole cap budget, and are coded with it"""
    _, _, a = cut
    budget, capped, margin, live = rm.search(a, -6.0, 48)
    assert capped.any() and not capped[~live].any()
    for f, row in enumerate(a["units"]):
        if row is None:
            continue
        for ch, us in enumerate(row):
            for j, u in enumerate(us):
                if capped[f, ch, j]:
                    assert budget[f, ch, j] == rm.STEP * rm.cap_steps(a, u, 48)
                    assert rm.worst_nmr(a["p"], u, budget[f, ch, j]) > -6.0
    assert not budget[~live].any()


def test_stream_decodes(cut):
    """the model's stream is an ordinary scalar .pac: the oracle's decoder takes it, and at the cap budgets of a
    constant rate it is the constant-rate stream"""
    pcm, sr, a = cut
    budget = rm.search(a, 0.0, 320)[0]
    data = rm.encode(a, budget, len(pcm))
    recs, (hsr, n_ch, use_sbr, use_vq) = nm.records(data)
    assert (hsr, n_ch, use_sbr, use_vq) == (sr, 2, False, False)
    assert len(recs) == 2 * sum(row is not None for row in a["units"])
    out = po.decode_stream(data)
    assert out.dtype == np.int16 and out.shape[1] == 2 and len(out) >= len(pcm)
    assert 0.0 < rm.kbps_per_channel(a, data) < 320.0
    # budgets that are the constant-rate rule's own reproduce the oracle's constant-rate stream
    p = po.make_params(sr, 2, 128)
    cbr = np.zeros_like(budget, dtype=np.float64)
    for f, row in enumerate(a["units"]):
        if row is not None:
            for ch, us in enumerate(row):
                for j, u in enumerate(us):
                    p.nMDCTLines = rm.SHORT if u.short else rm.HOP
                    cbr[f, ch, j] = po.bit_budget(p, *u.flags)
    assert rm.encode(a, cbr, len(pcm)) == po.encode_stream(pcm, sr, 128, block_switching=True)
