"""The order in which the entry points that take a pacx_pcm answer bad arguments (include/pacx.h documents part of
it, callers see all of it): for every entry point one call per check of its chain, in chain order.  Each call
satisfies every earlier check and violates the one under test and, where it can, the later ones as well, so the
return code and the fragment of pacx_last_error name the check that answered.

No call here reaches a kernel: every one is refused or is an empty batch.  The views are the smallest there are, a
planar int16 frame of one channel, the same with n_frames = 0, and a nine-channel hop view for pacx_transient_flags.

The record bound of the two band curves (a record at the cap rate that would not fit pacx_payload_stride) cannot be
reached with the default widths and layouts: 16 bits x 128 lines x 8 sub-blocks are 2048 bytes and the headers of at
most 8 short bands at nScaleBits 4, nMantSizeBits 12 add 133.  The `wide` handles have nMantSizeBits 16 and seven
short bands of 13 lines: pacx_create counts the 91 covered lines (1601 bytes), the bound counts all 128 and gives
8 x (4 + 7 x 20 + 2048) + 4 bits = 2193 bytes against a slot of 2192.
"""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

OK, E_ARG, E_UNSUPPORTED = 0, -1, -2
KINDS = ("scalar", "vq", "vq_sbr")
NOT_SCALAR = "scalar handles only (created without use_vq, use_sbr)"
NOT_VQ_PLAIN = "gain-shape handles without SBR only"
WITH_VQ = "created with use_vq (call"
WITHOUT_VQ = "created without use_vq"
CAP = "max_bits_per_sample must lie in (0, 16]"
DTYPE = "pcm dtype must be"
NO_FIT = "a record at this cap rate would not fit pacx_payload_stride"
NAN = float("nan")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return a


class World:
    pass


@pytest.fixture(scope="module")
def w(A):
    """handles by kind, the views, one device buffer that every non-null pointer points into"""
    import torch
    E, L = A.engine.Encoder, A._lib
    assert (L.E_ARG, L.E_UNSUPPORTED) == (E_ARG, E_UNSUPPORTED)
    sr, bps = 48000, 128 / 48.0
    short7 = A.psychoac.ScaleFactorBands([13] * 7)
    assert short7.nBands == 7
    w = World()
    w.L = L
    w.handles = {"scalar": E(sr, bps), "vq": E(sr, bps, use_vq=True), "vq_sbr": E(sr, bps, use_vq=True, use_sbr=True),
                 "wide": E(sr, bps, n_mant_size_bits=16, sf_bands_short=short7),
                 "wide_vq": E(sr, bps, n_mant_size_bits=16, sf_bands_short=short7, use_vq=True)}
    w.lib = w.handles["scalar"].lib
    dev = w.handles["scalar"].device
    w.pcm = torch.zeros((9, 2048), dtype=torch.int16, device=dev)
    w.buf = torch.zeros((1 << 16,), dtype=torch.uint8, device=dev)
    w.D = ctypes.c_void_p(w.buf.data_ptr())
    p, bad_dtype = w.pcm.data_ptr(), 7
    w.one = L.PacxPcm(p, L.PCM_I16, 1, 1, 1024, 2048, 1)            # one frame of one channel, planar
    w.empty = L.PacxPcm(p, L.PCM_I16, 1, 0, 1024, 2048, 1)          # the same view without a frame
    w.bad = L.PacxPcm(p, bad_dtype, 1, 1, 1024, 2048, 1)            # the view check refuses the dtype
    w.bad_empty = L.PacxPcm(p, bad_dtype, 1, 0, 1024, 2048, 1)
    w.hops9 = L.PacxPcm(p, L.PCM_I16, 9, 1, 1024, 2048, 1)          # one hop of nine channels
    w.hops9_f64 = L.PacxPcm(p, L.PCM_F64, 9, 1, 1024, 2048, 1)
    w.hops9_bad = L.PacxPcm(p, bad_dtype, 9, 1, 1024, 2048, 1)
    w.hops0 = L.PacxPcm(p, L.PCM_I16, 1, 0, 1024, 2048, 1)
    row, sub = ctypes.c_int32(0), ctypes.c_int32(0)
    assert w.lib.pacx_rate_curve_layout(w.handles["scalar"].h, 7.0, ctypes.byref(row), ctypes.byref(sub)) == OK
    w.row = row.value
    assert w.row > 0
    torch.cuda.synchronize()
    yield w
    torch.cuda.synchronize()
    for e in w.handles.values():
        e.close()


def expect(w, kind, name, args, rc, fragment=None):
    """one call on the handle of this kind (None: a null handle); fragment: what pacx_last_error must hold"""
    h = w.handles[kind].h if kind else None
    got = getattr(w.lib, name)(h, *args)
    assert got == rc, (name, kind, got, w.lib.pacx_last_error(h))
    if fragment is not None:
        msg = w.lib.pacx_last_error(h).decode()
        assert fragment in msg, (name, kind, msg)


ref = ctypes.byref


def test_mdct_smr_nmr(w):
    """null handle -> view -> empty batch is OK -> null pointers (mdct: then KBD with flags or PREWINDOWED)"""
    D, L = w.D, w.L
    # name, the arguments behind the view with every pointer p, the fragment of the null-pointer check
    calls = (("pacx_mdct_batch", lambda p: (p, 0, p, p, None), "pacx_mdct_batch: lines is null"),
             ("pacx_smr_batch", lambda p: (p, 0, p, p, p, None), "pacx_smr_batch: lines or smr is null"),
             ("pacx_nmr_batch", lambda p: (p, p, p, p, p, p, p, None), "pacx_nmr_batch: null pointer"))
    for name, rest, null_msg in calls:
        expect(w, None, name, (ref(w.bad), *rest(None)), E_ARG)
        for kind in KINDS:
            expect(w, kind, name, (ref(w.bad), *rest(None)), E_ARG, DTYPE)
            expect(w, kind, name, (ref(w.bad_empty), *rest(None)), E_ARG, DTYPE)
            expect(w, kind, name, (ref(w.empty), *rest(None)), OK)
            expect(w, kind, name, (ref(w.one), *rest(None)), E_ARG, null_msg)
    kbd_pre = L.MDCT_KBD | L.MDCT_PREWINDOWED
    for kind in KINDS:
        # without lines the null check answers before the mode check
        expect(w, kind, "pacx_mdct_batch", (ref(w.one), None, kbd_pre, None, None, None), E_ARG, "lines is null")
        expect(w, kind, "pacx_mdct_batch", (ref(w.one), None, kbd_pre, D, None, None), E_ARG, "PACX_MDCT_KBD takes no")
        expect(w, kind, "pacx_mdct_batch", (ref(w.one), D, L.MDCT_KBD, D, None, None), E_ARG, "PACX_MDCT_KBD takes no")


def test_encode_and_encode_pack(w):
    """view -> empty is OK -> null outputs E_ARG -> use_vq handle E_UNSUPPORTED; pacx_encode_pack_batch first refuses a
    non-empty batch without payload or n_bytes"""
    D = w.D
    enc = lambda view, p: (ref(view), None, p, p, p, p, p, None)                      # noqa: E731
    pack = lambda view, p, q: (ref(view), None, p, p, p, p, p, q, q, None)            # noqa: E731
    expect(w, None, "pacx_encode_batch", enc(w.bad, None), E_ARG)
    expect(w, None, "pacx_encode_pack_batch", pack(w.bad, None, None), E_ARG)
    for kind in KINDS:
        # the packing form alone: payload and n_bytes, before the view is looked at (only n_frames is)
        expect(w, kind, "pacx_encode_pack_batch", pack(w.bad, None, None), E_ARG, "payload and n_bytes are required")
        expect(w, kind, "pacx_encode_pack_batch", (ref(w.bad), None, None, None, None, None, None, D, None, None), E_ARG,
               "payload and n_bytes are required")
        expect(w, kind, "pacx_encode_batch", enc(w.bad, None), E_ARG, DTYPE)
        expect(w, kind, "pacx_encode_pack_batch", pack(w.bad, None, D), E_ARG, DTYPE)
        expect(w, kind, "pacx_encode_pack_batch", pack(w.bad_empty, None, None), E_ARG, DTYPE)
        # an empty batch: nothing is needed, and a gain-shape handle is not refused
        expect(w, kind, "pacx_encode_batch", enc(w.empty, None), OK)
        expect(w, kind, "pacx_encode_pack_batch", pack(w.empty, None, None), OK)
        expect(w, kind, "pacx_encode_batch", enc(w.one, None), E_ARG, "pacx_encode_batch: null output pointer")
        expect(w, kind, "pacx_encode_pack_batch", pack(w.one, None, D), E_ARG, "pacx_encode_pack_batch: null output pointer")
    for kind in ("vq", "vq_sbr"):
        expect(w, kind, "pacx_encode_batch", enc(w.one, D), E_UNSUPPORTED, WITH_VQ)
        expect(w, kind, "pacx_encode_pack_batch", pack(w.one, D, D), E_UNSUPPORTED, WITH_VQ)


def test_encode_vq(w):
    """view -> empty is OK -> null outputs -> entries arguments -> scalar handle E_UNSUPPORTED"""
    D = w.D
    call = lambda view, p, ent, cnt, per: (ref(view), None, p, p, p, p, p, ent, cnt, per, None)        # noqa: E731
    expect(w, None, "pacx_encode_vq_batch", call(w.bad, None, D, None, 0), E_ARG)
    for kind in KINDS:
        expect(w, kind, "pacx_encode_vq_batch", call(w.bad, None, D, None, 0), E_ARG, DTYPE)
        expect(w, kind, "pacx_encode_vq_batch", call(w.empty, None, D, None, 0), OK)
        expect(w, kind, "pacx_encode_vq_batch", call(w.empty, None, None, None, 0), OK)
        expect(w, kind, "pacx_encode_vq_batch", call(w.one, None, D, None, 0), E_ARG, "null output pointer")
        expect(w, kind, "pacx_encode_vq_batch", call(w.one, D, D, None, 4), E_ARG, "entries need entry_count")
        expect(w, kind, "pacx_encode_vq_batch", call(w.one, D, D, D, 0), E_ARG, "entries need entry_count")
        expect(w, kind, "pacx_encode_vq_batch", call(w.one, D, None, D, 4), E_ARG, "entries need entry_count")
    expect(w, "scalar", "pacx_encode_vq_batch", call(w.one, D, None, None, 0), E_UNSUPPORTED, WITHOUT_VQ)
    expect(w, "scalar", "pacx_encode_vq_batch", call(w.one, D, D, D, 4), E_UNSUPPORTED, WITHOUT_VQ)


def test_transient_flags(w):
    """view -> dtype or null transient -> more than 8 channels E_UNSUPPORTED; no empty-batch return"""
    D = w.D
    expect(w, None, "pacx_transient_flags", (ref(w.hops9_bad), None, None, None), E_ARG)
    for kind in KINDS:
        expect(w, kind, "pacx_transient_flags", (ref(w.hops9_bad), None, None, None), E_ARG, DTYPE)
        expect(w, kind, "pacx_transient_flags", (ref(w.hops9_f64), D, None, None), E_ARG, "int16 hops and a transient buffer")
        expect(w, kind, "pacx_transient_flags", (ref(w.hops9), None, None, None), E_ARG, "int16 hops and a transient buffer")
        # no hops, every output null: the transient buffer is asked for all the same
        expect(w, kind, "pacx_transient_flags", (ref(w.hops0), None, None, None), E_ARG, "int16 hops and a transient buffer")
        expect(w, kind, "pacx_transient_flags", (ref(w.hops9), D, D, None), E_UNSUPPORTED, "at most 8 channels")
        # no hops and no flags wanted: the launcher has nothing to launch
        expect(w, kind, "pacx_transient_flags", (ref(w.hops0), D, None, None), OK)


def budgeted(w, name, view, p, cap_rate=7.0, target=-3.0):
    """the arguments of one of the three budgeted encodes with every pointer p (the optional mantissa stays null)"""
    outs = (p, p, p, None, p, p, p)
    if name == "pacx_encode_pack_nmr_batch":
        return (ref(view), None, target, cap_rate, *outs, p, None)
    return (ref(view), None, p, *outs, None)


def test_encode_pack_nmr_budget_alloc(w):
    """handle kind -> for the nmr form, finite target then cap range -> view -> null pointers also for an empty batch ->
    empty is OK"""
    D = w.D
    for name in ("pacx_encode_pack_nmr_batch", "pacx_encode_pack_budget_batch", "pacx_encode_pack_alloc_batch"):
        expect(w, None, name, budgeted(w, name, w.bad, None, 0.0, NAN), E_ARG)
        for kind in ("vq", "vq_sbr"):
            expect(w, kind, name, budgeted(w, name, w.bad, None, 0.0, NAN), E_UNSUPPORTED, NOT_SCALAR)
            expect(w, kind, name, budgeted(w, name, w.empty, D), E_UNSUPPORTED, NOT_SCALAR)
        if name == "pacx_encode_pack_nmr_batch":
            for target in (NAN, float("inf")):
                expect(w, "scalar", name, budgeted(w, name, w.bad, None, 0.0, target), E_ARG, "target_nmr_db is not finite")
            for cap_rate in (0.0, -1.0, NAN, 16.5):
                expect(w, "scalar", name, budgeted(w, name, w.bad, None, cap_rate), E_ARG, CAP)
        expect(w, "scalar", name, budgeted(w, name, w.bad, None), E_ARG, DTYPE)
        expect(w, "scalar", name, budgeted(w, name, w.bad_empty, None), E_ARG, DTYPE)
        expect(w, "scalar", name, budgeted(w, name, w.empty, None), E_ARG, name + ": null pointer")
        expect(w, "scalar", name, budgeted(w, name, w.one, None), E_ARG, name + ": null pointer")
        expect(w, "scalar", name, budgeted(w, name, w.empty, D), OK)


def test_rate_curve_and_band_curve(w):
    """handle kind -> cap range -> view -> null pointers also when empty -> band: record bound E_UNSUPPORTED / rate: row
    too small -> empty is OK"""
    D = w.D
    rate = lambda view, p, cap_rate=7.0, row=0: (ref(view), None, cap_rate, row, p, p, p, None)       # noqa: E731
    band = lambda view, p, cap_rate=7.0: (ref(view), None, cap_rate, p, p, p, None)                   # noqa: E731
    for name, call in (("pacx_rate_curve_batch", rate), ("pacx_band_curve_batch", band)):
        expect(w, None, name, call(w.bad, None, 0.0), E_ARG)
        for kind in ("vq", "vq_sbr"):
            expect(w, kind, name, call(w.bad, None, 0.0), E_UNSUPPORTED, NOT_SCALAR)
            expect(w, kind, name, call(w.empty, D), E_UNSUPPORTED, NOT_SCALAR)
        for cap_rate in (0.0, -1.0, NAN, 16.5):
            expect(w, "scalar", name, call(w.bad, None, cap_rate), E_ARG, CAP)
        expect(w, "scalar", name, call(w.bad, None), E_ARG, DTYPE)
        expect(w, "scalar", name, call(w.bad_empty, None), E_ARG, DTYPE)
        expect(w, "scalar", name, call(w.empty, None), E_ARG, name + ": null pointer")
        expect(w, "scalar", name, call(w.one, None), E_ARG, name + ": null pointer")
    # the record bound of the band curve: null pointers still answer first, then the bound, for an empty batch too
    expect(w, "wide", "pacx_band_curve_batch", band(w.empty, None, 16.0), E_ARG, "null pointer")
    expect(w, "wide", "pacx_band_curve_batch", band(w.empty, D, 16.0), E_UNSUPPORTED, NO_FIT)
    expect(w, "wide", "pacx_band_curve_batch", band(w.one, D, 16.0), E_UNSUPPORTED, NO_FIT)
    expect(w, "wide", "pacx_band_curve_batch", band(w.empty, D, 7.0), OK)
    # the row of the rate curve
    expect(w, "scalar", "pacx_rate_curve_batch", rate(w.empty, D, 7.0, 0), E_ARG, "row is smaller than pacx_rate_curve_layout's")
    expect(w, "scalar", "pacx_rate_curve_batch", rate(w.one, D, 7.0, w.row - 1), E_ARG,
           "row is smaller than pacx_rate_curve_layout's (%d)" % w.row)
    expect(w, "scalar", "pacx_rate_curve_batch", rate(w.empty, D, 7.0, w.row), OK)
    expect(w, "scalar", "pacx_band_curve_batch", band(w.empty, D), OK)


def test_vq_band_curve(w):
    """handle kind -> cap range -> view -> record bound -> empty is OK -> null pointers (the order include/pacx.h
    documents)"""
    D, name = w.D, "pacx_vq_band_curve_batch"
    call = lambda view, p, cap_rate=7.0: (ref(view), None, cap_rate, p, p, p, None)                   # noqa: E731
    expect(w, None, name, call(w.bad, None, 0.0), E_ARG)
    for kind in ("scalar", "vq_sbr", "wide"):
        expect(w, kind, name, call(w.bad, None, 0.0), E_UNSUPPORTED, NOT_VQ_PLAIN)
        expect(w, kind, name, call(w.empty, D), E_UNSUPPORTED, NOT_VQ_PLAIN)
    for kind in ("vq", "wide_vq"):
        for cap_rate in (0.0, -1.0, NAN, 16.5):
            expect(w, kind, name, call(w.bad, None, cap_rate), E_ARG, CAP)
        expect(w, kind, name, call(w.bad, None, 16.0), E_ARG, DTYPE)
        expect(w, kind, name, call(w.bad_empty, None, 16.0), E_ARG, DTYPE)
    expect(w, "wide_vq", name, call(w.empty, None, 16.0), E_UNSUPPORTED, NO_FIT)
    expect(w, "wide_vq", name, call(w.one, None, 16.0), E_UNSUPPORTED, NO_FIT)
    for kind in ("vq", "wide_vq"):
        expect(w, kind, name, call(w.empty, None), OK)             # nothing to write: the outputs may be null
        expect(w, kind, name, call(w.one, None), E_ARG, name + ": null pointer")
    expect(w, "vq", name, call(w.one, None, 16.0), E_ARG, name + ": null pointer")    # the default widths always fit


def test_encode_vq_alloc(w):
    """handle kind -> view -> empty is OK -> null pointers"""
    D, name = w.D, "pacx_encode_vq_alloc_batch"
    call = lambda view, p: (ref(view), None, p, p, p, p, p, p, None)                  # noqa: E731
    expect(w, None, name, call(w.bad, None), E_ARG)
    for kind in ("scalar", "vq_sbr"):
        expect(w, kind, name, call(w.bad, None), E_UNSUPPORTED, NOT_VQ_PLAIN)
        expect(w, kind, name, call(w.empty, D), E_UNSUPPORTED, NOT_VQ_PLAIN)
    expect(w, "vq", name, call(w.bad, None), E_ARG, DTYPE)
    expect(w, "vq", name, call(w.bad_empty, None), E_ARG, DTYPE)
    expect(w, "vq", name, call(w.empty, None), OK)
    expect(w, "vq", name, call(w.one, None), E_ARG, name + ": null pointer")
