"""CPU gate on what the compiler made of the kernels: every kernel a default entry point
launches must run without scratch memory and without spilled vector registers
(`hipcc -Rpass-analysis=kernel-resource-usage`, recorded per kernel by
audio-codec_amd/build.py in build/resources.json at compile time).

Round 1's k_mask<1024> silently kept a 32-double array in scratch (272 B per lane,
150 MB of HBM writes per launch) because one reduction helper indexed it with a run-time
value; this test is what keeps that from coming back unnoticed."""
import importlib
import re

import pytest


@pytest.fixture(scope="module")
def res():
    import audio_codec_amd  # noqa: F401
    return importlib.import_module("audio_codec_amd.build").resources()


def _find(res, pattern):
    hits = {k: v for k, v in res.items() if re.search(pattern, k)}
    assert hits, f"no kernel matches {pattern!r}"
    return hits


# (regex on the demangled name, max VGPRs or None, min waves/SIMD or None)
HOT = [
    (r"^void k_mdct_long_x2p<8, 2, false>\(", 256, 2),   # headline MDCT kernel, stand-alone launches (the roofline figure)
    (r"^void k_mdct_long_x2p<8, 2, true>\(", 256, 2),    # ... and as the step launches it
    (r"^k_mdct_long_v2\(", 256, 2),                     # batches with block-switching flags
    (r"^void k_mdct_short<0, true>\(", 128, 3),
    (r"^void k_side_long<0, true>\(", 168, 3),           # int16 fast path, compact LDS (SBR handles too)
    (r"^void k_side_short<0, true>\(", 168, 3),
    (r"^void k_mask<1024, true>\(", 168, 3),            # mask + BitAlloc + quantise + pack, long frames
    (r"^void k_mask<1024, false>\(", 168, 3),
    (r"^void k_mask<128, false>\(", 96, 5),
    (r"^k_tail_long\(", 128, 4),
    (r"^k_tail_short\(", 72, 7),
    (r"^k_gather_small\(", None, None),
    (r"^void k_vq_frame<(false|true)>\(", 102, 5),                          # gain-shape coder: five workgroups per CU is what it runs on
    (r"^k_vq\(", 128, 4),                                # ... its fallback for trees beyond the node store
    (r"^k_vq_redo\(", 152, 3),                           # ... the same body behind k_vq_frame, on the default path: 146 today, granule 8
    (r"^k_vq_join\(", None, None),
    (r"^k_vq_dec_frame\(", 102, 5),                      # gain-shape decoder: five workgroups per CU
    (r"^k_vq_dec\(", 168, 3),                            # ... its fallback
    (r"^k_unpack\(", None, None),
    (r"^k_imdct_long\(", None, None),
    (r"^k_imdct_short\(", None, None),
    (r"^k_transient\(", None, None),
    (r"::k_band_profile\(", 128, 4),                     # 1024 threads: 128 registers are all a workgroup may have
    (r"::k_band_profile_seg\(", 128, 4),
    (r"::k_rate_profile<true>\(", None, 8),
    # the bucket scans (bucket_dev.h), 1024 threads each: past 128 registers, or with a spill, they do not launch at
    # all.  84 is the largest today; 88 is the next allocation granule of 8 above it
    (r"::k_bucket_scan\(", 88, None),
    (r"::k_bucket_step\(", 88, None),
    (r"::k_bucket_through\(", 88, None),
    (r"::k_pin_step\(", 88, None),
    (r"::k_pin_freeze\(", 88, None),
    (r"::k_pin_finish\(", 88, None),
]


@pytest.mark.parametrize("pattern,max_vgprs,min_occ", HOT)
def test_hot_kernel_has_no_scratch(res, pattern, max_vgprs, min_occ):
    for name, r in _find(res, pattern).items():
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B/lane of scratch"
        assert r["vgpr_spill"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs"
        if max_vgprs is not None:
            assert r["vgprs"] + r["agprs"] <= max_vgprs, (name, r)
        if min_occ is not None:
            assert r["occupancy"] >= min_occ, (name, r)


def test_every_kernel_is_reported(res):
    """the report covers the library: a kernel that lost its remark (renamed flag, new
    compiler) must not pass the gate by being absent"""
    assert len(res) >= 40
    for name, r in res.items():
        for key in ("vgprs", "agprs", "scratch", "vgpr_spill", "occupancy", "lds", "source"):
            assert key in r, (name, key)


def test_only_listed_kernels_use_scratch(res):
    """anything else with scratch is a function-level mirror off the hot path, named here"""
    allowed = {"k_bitalloc_generic"}        # serial reference-shaped BitAlloc (bitalloc.BitAlloc mirror), one lane per call
    for name, r in res.items():
        if r["scratch"] or r["vgpr_spill"]:
            assert any(a in name for a in allowed), f"{name}: scratch {r['scratch']}, spilled {r['vgpr_spill']}"


def test_vq_frame_lds_allows_five_workgroups(res):
    """k_vq_frame is bound by dependency chains, so workgroups per CU are its throughput: its dynamic LDS (the
    launcher's VQF_SMEM) plus its static arrays must fit five times into a CU's 160 KB."""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "audio-codec_amd", "csrc", "k_vq.hip")).read()
    def macro(name):
        m = re.search(r"#define\s+%s\s+\(?([^/\n]+?)\)?\s*(/\*|\n)" % name, src)
        assert m, name
        return m.group(1).strip()
    ncap, nlv = int(macro("VQF_NCAP")), int(macro("VQF_NLV"))
    fixed = int(macro("VQF_FIXED"))
    buf = eval(macro("VQF_BUF").replace("PACX_M_LONG", "1024"))
    smem = fixed + 2 * buf * 8 + ncap * 8 + 6 * ncap * 2 + 4 * ncap + 2 * nlv * 2 + 128 + 64
    static_lds = max(v["lds"] for k, v in res.items() if k.startswith("void k_vq_frame<false>("))   # its static arrays
    assert 5 * (smem + static_lds) <= 160 * 1024 - 5 * 512, (smem, static_lds)
