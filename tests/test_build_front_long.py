"""CPU gate on the fused front end of the all-long step (k_front_long, csrc/k_psy.hip), from the compiler's resource
report (build/resources.json, see tests/test_build_resources.py): it takes the place of k_side_long<0, true> in
the step and must fit where that kernel fits -- no scratch, three waves per SIMD (at most 168 registers) and no more
LDS, so that twelve waves share a CU beside the other step's kernels."""
import importlib

import pytest


@pytest.fixture(scope="module")
def res():
    import audio_codec_amd  # noqa: F401
    return importlib.import_module("audio_codec_amd.build").resources()


def _one(res, prefix):
    hits = [v for k, v in res.items() if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, len(hits))
    return hits[0]


def test_front_long_fits_where_the_side_chain_fits(res):
    front, side = _one(res, "k_front_long("), _one(res, "void k_side_long<0, true>(")
    assert front["scratch"] == 0 and front["vgpr_spill"] == 0, front
    assert front["vgprs"] + front["agprs"] <= 168 and front["occupancy"] >= 3, front
    assert front["lds"] <= side["lds"], (front["lds"], side["lds"])
