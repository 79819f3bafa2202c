"""The conditions tests/test_gpu_stream_order.py rests on, checked on the CPU against the reference's fixtures, the oracle
and the models (no GPU): a kernel that read the DECOY anywhere shows up only if the decoy's result differs from the real
one in every output row -- every channel-frame's record, every decoded hop, every solve's target -- and the small
shapes must still take the forks they are there for.  No exceptions: a pair that fails here is replaced, not excused.
"""
import numpy as np
import pytest

import mixed_batches as mb
import stream_order as so


@pytest.mark.parametrize("variant", ["long", "bs"])
def test_scalar_excerpts_differ_in_every_record(variant):
    real, decoy = (so.scalar_material(n, variant) for n in so.PAIRS[variant])
    assert real["planar"].shape == decoy["planar"].shape == (2, 67 * so.HOP) and real["planar"].dtype == np.int16
    assert real["n_frames"] == decoy["n_frames"] == 66 and len(real["records"]) == len(decoy["records"]) == 132
    assert all(a != b for a, b in zip(real["records"], decoy["records"]))           # n_bytes or payload, every row
    # the bodies end where their records end, and both fit the slot a handle gives a record
    assert all(0 < len(r) <= 2192 for m in (real, decoy) for r in m["records"])
    assert real["body"] != decoy["body"]
    if variant == "bs":
        assert real["flags"].shape == decoy["flags"].shape == (66,)
        assert not np.array_equal(real["flags"], decoy["flags"])                   # the flag set, taken as a whole
        for m in (real, decoy):                                                     # both frame lists are in use
            short = int(((m["flags"] & 2) != 0).sum())
            assert 0 < short < 66, short
    else:
        assert real["flags"] is None and decoy["flags"] is None


@pytest.mark.parametrize("kbps", [128, 96])
def test_gain_shape_excerpts_differ_in_every_record(kbps):
    real, decoy = (so.vq_material(n, kbps) for n in so.PAIRS["bs"])
    assert real["planar"].shape == decoy["planar"].shape == (2, 27 * so.HOP)
    assert real["n_frames"] == decoy["n_frames"] == 26 and len(real["records"]) == len(decoy["records"]) == 52
    assert all(a != b for a, b in zip(real["records"], decoy["records"]))
    assert not np.array_equal(real["flags"], decoy["flags"])
    for m in (real, decoy):
        assert 0 < int(((m["flags"] & 2) != 0).sum()) < 26                          # long and short frames: the fork runs


@pytest.mark.parametrize("tag", ["long", "bs", "vq128", "vq96"])
def test_decoded_pcm_differs_in_every_hop(tag):
    a, b = so.decoded("castanet", tag), so.decoded("harpsichord", tag)
    hops = 27 if tag.startswith("vq") else 67
    assert a.shape == b.shape == (hops * so.HOP, 2) and a.dtype == np.int16
    a, b = a.reshape(hops, -1), b.reshape(hops, -1)
    assert all(not np.array_equal(x, y) for x, y in zip(a, b))
    # the records the decode cases index: as many in either body, so one record count serves both
    if tag.startswith("vq"):
        m = [so.vq_material(n, int(tag[2:])) for n in ("castanet", "harpsichord")]
    else:
        m = [so.scalar_material(n, tag) for n in ("castanet", "harpsichord")]
    assert len(m[0]["records"]) == len(m[1]["records"]) == 2 * (hops - 1)
    x, y = so.padded_bodies(m[0]["body"], m[1]["body"])
    assert x.shape == y.shape and not x[-8:].any() and not y[-8:].any()


@pytest.mark.parametrize("name", sorted(so.FLAGGED))
def test_flagged_batches_have_an_empty_list_and_differ_in_every_record(name):
    real, decoy = so.flagged_material(name, False), so.flagged_material(name, True)
    assert real["blocks"].shape == decoy["blocks"].shape == (64, 2, 2048)
    for m in (real, decoy):
        short = (m["flags"] & 2) != 0
        assert short.all() if name == "no_long" else not short.any()                # one of the two lists is empty
        assert len(set(m["flags"].tolist())) == 4                                   # every flag byte of its kind
    assert not np.array_equal(real["flags"], decoy["flags"])
    assert (real["items"] // 8 != decoy["items"] // 8).all()                        # never the same atom in a frame
    a, b = so.flagged_records(real), so.flagged_records(decoy)
    assert len(a) == len(b) == 128 and all(r is not None and len(r) > 0 for r in a + b)      # no dropped hop
    assert all(x != y for x, y in zip(a, b))
    assert mb.N_ITEMS == 88


@pytest.mark.parametrize("kind", so.KINDS)
def test_solves_differ_in_every_target(kind):
    real, decoy = so.model_answers(kind, so.curve_material(kind, False)), so.model_answers(kind, so.curve_material(kind, True))
    jobs = so.solve_jobs(kind)
    assert len(jobs["segments_a"][1]) == 4 and len(jobs["segments_b"][1]) == 2 and len(jobs["peak"][1]) == 3
    for name in ("plain", "segments_a", "segments_b", "peak", "bucket"):
        r, d = real[name], decoy[name]
        assert (r["t"] != d["t"]).all(), (name, r["t"], d["t"])                     # every solve's (segment's) target
        assert (r["met"] == 1).all() and (r["t"] > so.T_LO).all() and (r["t"] < so.T_HI).all(), (name, r["t"], r["met"])
        assert not np.array_equal(r["n_bytes"], d["n_bytes"]) and not np.array_equal(r["per_cf"], d["per_cf"])
    # the two segmented solves would not give each other's answer: their tables differ in length and in every limit
    assert len(real["segments_a"]["t"]) != len(real["segments_b"]["t"])
    assert not np.array_equal(real["segments_a"]["per_cf"], real["segments_b"]["per_cf"])
    # the bucket decided: the plain solve with the buffered one's limit would stop lower
    assert real["bucket"]["scan"][3] == -1 and real["bucket"]["t"][0] > so.T_LO
    assert not np.array_equal(real["bucket"]["level"], decoy["bucket"]["level"])


def test_the_table_of_calls_that_may_block_quotes_the_header():
    import os
    text = " ".join(open(os.path.join(so.HERE, "..", "include", "pacx.h")).read().replace("*", " ").split())
    for what, names, sentence in so.MAY_BLOCK:
        assert " ".join(sentence.split()) in text, what
        assert names
