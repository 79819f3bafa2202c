"""The twenty Encoder methods on a rate curve or a band curve against the transcript recorded before they were folded
onto one implementation per operation (tests/golden/curve_calls.json, written by tests/golden/make_curve_calls.py; how
it is taken: tests/curve_calls.py): the C call of every method with every argument, what it returns and every refusal
word for word.  On the CPU with a library that only records; and the prototypes of the twenty calls, written out."""
import ctypes
import json
import os

import pytest

import curve_calls

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = json.load(open(os.path.join(HERE, "golden", "curve_calls.json")))
OPS = ("solve", "solve_segments", "solve_peak", "profile", "profile_segments", "pick", "pick_segments", "thresholds",
       "pick_thresholds", "pick_thresholds_segments")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    return a


@pytest.mark.parametrize("kind", ["rate", "band"])
def test_calls_returns_and_refusals_are_the_recorded_ones(A, kind):
    want = RECORDED[kind]
    seen, methods = set(), set()
    for label, m, inputs in curve_calls.cases(kind):
        got = json.loads(json.dumps(curve_calls.transcript(A, f"{kind}_{m}", inputs)))
        assert got == want[label], (kind, label)
        seen.add(label)
        methods.add(m)
        if ":" not in label or label.endswith(": list"):
            got = curve_calls.transcript(A, f"{kind}_{m}", inputs, rc=A._lib.E_UNSUPPORTED)
            assert json.loads(json.dumps(got)) == want["unsupported: " + m], (kind, label)
            assert got["raises"][0] == "NotImplementedError"
            seen.add("unsupported: " + m)
    assert seen == set(want) and methods == set(OPS)


def test_the_record_covers_what_it_should():
    for kind in ("rate", "band"):
        rec = RECORDED[kind]
        for m in OPS:
            plain = rec[m if m in rec else m + ": list"]
            assert [c["name"] for c in plain["calls"]] == [f"pacx_{kind}_{m}"] and "returns" in plain
        raised = {label: r["raises"] for label, r in rec.items() if "raises" in r and not label.startswith("unsupported")}
        assert all(r["calls"] == [] for label, r in rec.items() if label in raised)
        assert all(t == "ValueError" for t, _ in raised.values())
        for part in ("wrong dtype", "wrong shape", "kept e wrong", "range off the grid", "range over PROFILE_MAX",
                     "seg_cf 0", "first_off = seg_cf", "target_t too long", "not contiguous", "negative segment limit",
                     "negative limit_bytes"):
            assert any(part in label for label in raised), part
        # the two early returns: no call at all
        assert rec["profile_segments: no frame, no segment"]["calls"] == []
        assert rec["profile_segments: no frame, no segment, out"]["returns"] == "= out"


def test_signatures_of_the_twenty(A):
    P, I64, I32, D, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_int
    want = {
        "pacx_rate_solve": (I, [P, I64, I32, I32, P, P, P, I64, D, D, P, P, P, P, P]),
        "pacx_band_solve": (I, [P, I64, P, P, P, I64, D, D, P, P, P, P, P]),
        "pacx_rate_solve_segments": (I, [P, I64, I32, I32, P, P, P, I64, P, P, D, D, P, P, P, P, P]),
        "pacx_band_solve_segments": (I, [P, I64, P, P, P, I64, P, P, D, D, P, P, P, P, P]),
        "pacx_rate_solve_peak": (I, [P, I64, I32, I32, P, P, P, I64, P, P, I64, D, D, P, P, P, P, P, P, P]),
        "pacx_band_solve_peak": (I, [P, I64, P, P, P, I64, P, P, I64, D, D, P, P, P, P, P, P, P]),
        "pacx_rate_profile": (I, [P, I64, I32, I32, P, P, P, D, D, P, P]),
        "pacx_band_profile": (I, [P, I64, P, P, P, D, D, P, P]),
        "pacx_rate_profile_segments": (I, [P, I64, I32, I32, P, P, P, I64, I64, D, D, P, P]),
        "pacx_band_profile_segments": (I, [P, I64, P, P, P, I64, I64, D, D, P, P]),
        "pacx_rate_pick": (I, [P, I64, I32, I32, P, P, P, D, P, P, P, P]),
        "pacx_band_pick": (I, [P, I64, P, P, P, D, P, P, P, P]),
        "pacx_rate_pick_segments": (I, [P, I64, I32, I32, P, P, P, I64, I64, P, P, P, P, P]),
        "pacx_band_pick_segments": (I, [P, I64, P, P, P, I64, I64, P, P, P, P, P]),
        "pacx_rate_thresholds": (I, [P, I64, I32, I32, P, P, P, D, D, P, P, P, P]),
        "pacx_band_thresholds": (I, [P, I64, P, P, P, D, D, P, P, P, P]),
        "pacx_rate_pick_thresholds": (I, [P, I64, I32, I32, P, P, P, D, D, D, P, P, P, P]),
        "pacx_band_pick_thresholds": (I, [P, I64, P, P, P, D, D, D, P, P, P, P]),
        "pacx_rate_pick_thresholds_segments": (I, [P, I64, I32, I32, P, P, P, I64, I64, D, D, P, P, P, P, P]),
        "pacx_band_pick_thresholds_segments": (I, [P, I64, P, P, P, I64, I64, D, D, P, P, P, P, P]),
    }
    assert set(want) == {f"pacx_{kind}_{m}" for kind in ("rate", "band") for m in OPS}
    assert {k: A._lib.SIGNATURES[k] for k in want} == want
    assert len(A._lib.SIGNATURES) == 73
